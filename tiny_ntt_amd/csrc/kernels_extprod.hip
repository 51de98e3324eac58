// kernels_extprod.hip — the external product RGSW x RLWE (polydot_extprod_kernel) with its launcher: both output components
// from the digits of ALL input polynomials of a ciphertext in one launch.  A translation unit of its own, with its own
// dynamic-LDS symbol: a kernel that shares the family's symbol changes the register allocation of its neighbours.
#include "fused_kernels.h"

namespace tn {

// ============================================================================
// External product: c[row][o] = sum_{i < ins} sum_{j < terms} digit_j(a[row][i]) * b[SHARED ? 0 : row][o][i][j], o < 2
// ============================================================================
// polydot_extprod_kernel: polydot_gadget2_kernel's row (kernels_gadget.hip, where the reasons for its form are given) with a
// run-time loop over the `ins` input polynomials of the output row around the term loop.  The two sums are cleared once per
// output row and stay in registers across the inputs; every input polynomial is read and made canonical once (gadget_canon),
// XL of its words per thread put away in the thread-private LDS slots, the carry mask cleared (balanced carries never run
// from one polynomial into the next); every digit is cut and transformed ONCE and multiplied into both sums (component 0
// through dot_product_into, the digit row left as it is; component 1 in place).  Two inverses and two stores follow the last
// term of the last input, as in the pair kernel: ins * terms + 2 transforms per output row, nothing but a read and c written.
// a is [batch][ins][n], bhat [sets][2][ins][terms][n] (component o of a set is a set of ins * terms rows of the dot product:
// the digit rows of input i are terms i * terms .. of it), c [batch][2][n].  The sums stay canonical (dot_accumulate_one), so
// ins * terms terms need no bound schedule of their own.
// Registers: the two sums, the term in flight and one prepared row, as in the pair kernel.  The one request the pair kernel
// does not have is the words of the NEXT input polynomial of the same row.  They are requested behind the last in-place
// product of the input before (the term in flight and the prepared row are dead there: the two sums and these words are all
// that is live) and consumed at once, in the same block: one round trip for the words stays exposed once per extra input
// (ins - 1 per output row), covered only by the other resident workgroups.  Anything earlier is a fifth live row during a
// transform or a product.  The form decides the registers (DESIGN.md 3.2g has the three reports): with the input's first
// prepared row requested behind its words (so that its latency lay under theirs) twelve 64-bit instantiations spilled; with
// the words consumed at the top of the next pass of a loop over the inputs (loaded at the bottom of one pass, live into the
// next) eight; with inputs and terms in one counted loop eighteen.  This form, the loop over the inputs left in its
// middle, between the term loop and the request, spills nowhere and holds no more registers than the pair kernel in any shape.
// The first input's words of the next output row are requested inside the second inverse, as in the pair kernel.
// The barrier and the read of the next output row stand behind the forward transform of the last term of the last input:
// both loop counters and both limits are kernel arguments, so the condition is workgroup-uniform.
// No address depends on data: prepared rows are indexed from row * 2 * ins * terms, rows of a from row * ins + i, 32-bit
// both (tn_poly_external_product_prepared_dev).
template <typename E, int LOGN, int LPT, bool LAZY, bool BC, bool SHARED, int XL>
__global__ void __launch_bounds__((1 << (LOGN - LPT)), (dot_waves<E, LOGN, LPT, LAZY>()))
polydot_extprod_kernel(const Arith<E> ar, const typename TwOf<E>::type* __restrict__ tab_fwd,
                       const typename TwOf<E>::type* __restrict__ tab_inv, const E* __restrict__ a, const E* __restrict__ bhat,
                       E* __restrict__ c, u32 batch, u32 ins, u32 terms, u32 base_log, u32 balanced, u32* sched, u32 chunk) {
  typedef FusedCfg<E, LOGN, LPT> Cfg;
  typedef Policy<E, LAZY> Pol;
  typedef typename TwOf<E>::type Tw;
  static_assert(Cfg::PHASES >= 2, "the last phase's twiddles are requested during the phase before it");
  static_assert(Cfg::R <= 32, "one carry bit per word of the thread in a 32-bit mask");
  static_assert(XL >= 0 && XL <= Cfg::R, "words of a per thread kept in LDS");
  extern __shared__ __attribute__((aligned(16))) unsigned char tn_smem_extprod[];
  const u32 tau = threadIdx.x;
  // LDS: [transpose image][XL * THREADS words of a][staged twiddles, forward][... inverse][next-row slot]
  E* lds = reinterpret_cast<E*>(tn_smem_extprod);
  E* lds_xw = lds + Cfg::lds_elems() + tau;                                   // word r of this thread at [r * THREADS]
  Tw* lds_fwd = reinterpret_cast<Tw*>(lds + Cfg::lds_elems() + XL * Cfg::THREADS);
  Tw* lds_inv = lds_fwd + Cfg::lds_tw_count();
  u32* lds_next = reinterpret_cast<u32*>(lds_inv + Cfg::lds_tw_count());      // output row this workgroup takes next
  for (u32 i = tau; i < (u32)Cfg::lds_tw_count(); i += Cfg::THREADS) {
    lds_fwd[i] = tab_fwd[Cfg::lds_tw_lo() + i];
    lds_inv[i] = tab_inv[Cfg::lds_tw_lo() + i];
  }
  __syncthreads();
  E acc0[Cfg::R], acc1[Cfg::R], xw[Cfg::R];  // the sums of the two components, then their results; xw: the words of the input polynomial
  u32 row = blockIdx.x * chunk;
  u32 taken = 1;                            // rows taken from the current chunk           (both workgroup-uniform: scalar registers)
  u32 chunk_id = blockIdx.x;                // fixed-stride mode: the chunk being processed
  if (row < batch) {
#pragma unroll
    for (int r = 0; r < Cfg::R; ++r) xw[r] = ld_operand<E, Cfg>(a, row * ins, tau, r);
  }
  constexpr int PRE_END = Cfg::LOGN;        // no resident last-stage twiddles (polydot_prepared_kernel)
  Tw prf[Cfg::NPRE];
  constexpr bool KARG = TN_KARG_ARITH != 0;
  const u32 comp = ins * terms;             // prepared rows of one component of a set
  u32 prev = row;
  bool have_c = false;
#pragma unroll
  for (int r = 0; r < Cfg::R; ++r) acc1[r] = 0;
  while (row < batch) {
    // one thread determines the next output row now; everyone reads the answer after the last term's transform
    const bool in_chunk = taken != chunk;
    taken = in_chunk ? taken + 1 : 1;
    chunk_id = in_chunk ? chunk_id : chunk_id + gridDim.x;
    if (tau == 0) *lds_next = in_chunk ? row + 1 : (sched ? gridDim.x + atomicAdd(&sched[0], 1u) : chunk_id) * chunk;
    // row of a per-set bhat of this output row's first term of component 0; component 1 follows ins * terms rows later
    // (< 2^31: tn_poly_external_product_prepared_dev)
    const u32 brow = row * 2u * comp;
    E xa[Cfg::R], xb[Cfg::R];                // the term in flight and the prepared row of the component being multiplied
    u32 tl = opaque_copy(tau);               // thread index for global addressing (see opaque_copy)
    // register r of prepared row t of component o (t = i * terms + j)
    auto request1 = [&](u32 o, u32 t, u32 th, int r) {
      xb[r] = SHARED ? ld_prepared<E, Cfg, false>(bhat, o * comp + t, th, r) : ld_prepared<E, Cfg, true>(bhat, brow + o * comp + t, th, r);
    };
    const Tw* zeta = prf + Cfg::pre_off(Cfg::LOGN - 1);      // (the base case's zeta records came with prf)
    u32 next = 0;
    u32 t = 0;                               // the term of the component's sum: i * terms + j
    // an input's words made canonical once, XL of them put away
    auto put_away = [&]() {
#pragma unroll
      for (int r = 0; r < Cfg::R; ++r) {
        xw[r] = gadget_canon<E, Pol>(xw[r], ar);
        if (r < XL) lds_xw[r * Cfg::THREADS] = xw[r];
      }
      sched_fence();
    };
    // consume the first input's words first (only their loads are in flight here: the wait is exact); then issue the stores of
    // the previous row's second component (the first iteration writes zeros to this row's own slot, which the same thread
    // overwrites one iteration later) and clear the sums, once per output row
    put_away();
    st_result<E, Cfg>(c, 2u * prev + 1u, tl, acc1);
#pragma unroll
    for (int r = 0; r < Cfg::R; ++r) { acc0[r] = 0; acc1[r] = 0; }
    for (u32 i = 0;;) {
      u32 carries = 0;                       // bit r: the carry of word r into its next digit (balanced mode); per input polynomial
      for (u32 j = 0; j < terms; ++j, ++t) {
        tl = opaque_copy(tau);
        // component 0's prepared row, before the forward's first phase
#pragma unroll
        for (int r = 0; r < Cfg::R; ++r) request1(0u, t, tl, r);
        sched_fence();
        const u32 shift = j * base_log;      // < 64 (tn_poly_external_product_prepared_dev)
        u32 next_carries = 0;
#pragma unroll
        for (int r = 0; r < Cfg::R; ++r) {
          u32 cy = (carries >> r) & 1u;
          const E w = r < XL ? (lds + Cfg::lds_elems())[r * Cfg::THREADS + tl] : xw[r];
          xa[r] = gadget_digit<E>(w, shift, base_log, balanced != 0, cy, ar.q);
          next_carries |= cy << r;
        }
        carries = next_carries;
        const TwRefs<E> twf = {tab_fwd, lds_fwd, prf, nullptr, opaque_zero()};
        forward_range<E, Cfg, Pol, 0, Cfg::PHASES, KARG, PRE_END, BC>(xa, tau, twf, ar, lds, true, tl);
        if (t + 1 == comp) {                 // everyone reads the next output row behind the last term of the last input
          __syncthreads();
          next = wave_uniform(*lds_next);
        }
        // component 0's product, the transformed digit row left as it is; component 1's prepared row goes pair by pair into
        // the registers that product has finished with (a thread index of its own: polydot_gadget2_kernel)
        dot_product_into<E, Cfg, Pol, BC>(acc0, xa, xb, zeta, ar, [&](auto i_) {
          constexpr int r = 2 * decltype(i_)::value;
          const u32 th = opaque_copy(tau);
          request1(1u, t, th, r);
          request1(1u, t, th, r + 1);
          sched_fence();
        });
        if constexpr (BC) basecase<Cfg, Pol>(xa, xb, zeta, ar);      // component 1's product may overwrite the digit row
        else pointwise<E, Cfg, Pol>(xa, xb, ar);
        dot_accumulate<E, Cfg, Pol>(acc1, xa, ar);
        sched_fence();
      }
      if (++i == ins) break;
      // the words of the next input polynomial of this row, requested and consumed here (see above)
      tl = opaque_copy(tau);
#pragma unroll
      for (int r = 0; r < Cfg::R; ++r) xw[r] = ld_operand<E, Cfg>(a, row * ins + i, tl, r);
      sched_fence();
      put_away();
    }
    // the private twiddles the first inverse starts with (behind the loops: requested inside them they are live across them)
    Tw pre[Cfg::NPRE], pre1[Cfg::NPRE];
    if constexpr (BC) tw_prefetch_stages<E, Cfg, Cfg::stage_begin(Cfg::PHASES - 1), Cfg::LOGN - 1>(pre, tl, tab_inv);
    else tw_prefetch<E, Cfg>(pre, tl, tab_inv);
    sched_fence();
    const TwRefs<E> twi0 = {tab_inv, lds_inv, pre, nullptr, opaque_zero()};
    inverse_all<E, Cfg, Pol, KARG, BC>(acc0, opaque_copy(tau), twi0, ar, lds, [&]() {});
    // the first result leaves its registers here; then the second inverse's private twiddles, through a thread index of their own
    tl = opaque_copy(tau);
    st_result<E, Cfg>(c, 2u * row, tl, acc0);
    sched_fence();
    if constexpr (BC) tw_prefetch_stages<E, Cfg, Cfg::stage_begin(Cfg::PHASES - 1), Cfg::LOGN - 1>(pre1, tl, tab_inv);
    else tw_prefetch<E, Cfg>(pre1, tl, tab_inv);
    sched_fence();
    const TwRefs<E> twi1 = {tab_inv, lds_inv, pre1, nullptr, opaque_zero()};
    inverse_all<E, Cfg, Pol, KARG, BC>(acc1, opaque_copy(tau), twi1, ar, lds, [&]() {
      // the first input polynomial of the next output row, requested after the inverse's own vector loads have been consumed
      // (inverse_all); this row's last digits have been taken.  Unconditional: after the last row this row's is read again and dropped.
      const u32 nrow = next < batch ? next : row;
#pragma unroll
      for (int r = 0; r < Cfg::R; ++r) xw[r] = ld_operand<E, Cfg>(a, nrow * ins, tl, r);
    });
    prev = row;
    have_c = true;
    row = next;
  }
  if (have_c) st_result<E, Cfg>(c, 2u * prev + 1u, tau, acc1);
  rearm_row_counters(sched, tau);
}

template <typename Sh>
static hipError_t launch_extprod_t(const tn_plan* p, const void* a, const void* bhat, bool shared, void* c, size_t batch, size_t ins, size_t terms,
                                   u32 base_log, bool balanced, hipStream_t s) {
  typedef typename Sh::E E;
  typedef typename Sh::Cfg Cfg;
  constexpr int LOGN = Sh::LOGN, LPT = Sh::LPT, XL = gadget2_lds_words<Sh>();
  constexpr bool LAZY = Sh::LAZY;
  const FusedProductLaunch<Sh> L(p);
  const u32 b32 = (u32)batch, i32 = (u32)ins, t32 = (u32)terms, bal = balanced ? 1u : 0u;
  constexpr size_t lds_bytes = fused_lds_bytes<Sh>(2, (size_t)XL * Cfg::THREADS);
  auto kern = shared ? polydot_extprod_kernel<E, LOGN, LPT, LAZY, false, true, XL> : polydot_extprod_kernel<E, LOGN, LPT, LAZY, false, false, XL>;
  if constexpr (L.HAS_BC) {
    if (L.use_bc) kern = shared ? polydot_extprod_kernel<E, LOGN, LPT, LAZY, true, true, XL> : polydot_extprod_kernel<E, LOGN, LPT, LAZY, true, false, XL>;
  }
  // Rows are planned as the dot kernel's with ins * terms operand rows: an output row is ins * terms forward transforms and two
  // inverses between two atomics.
  return launch_persistent(p, s, reinterpret_cast<const void*>(kern), Cfg::THREADS, lds_bytes, dot_row_bytes(Cfg::N * sizeof(E), ins * terms), batch,
                           FUSED_ROWS, [&](u32 grid, u32* sched, u32 chunk) {
    hipLaunchKernelGGL(kern, dim3(grid), dim3(Cfg::THREADS), lds_bytes, s, L.su.ar, L.fwd(), L.inv(),
                       (const E*)a, (const E*)bhat, (E*)c, b32, i32, t32, base_log, bal, sched, chunk);
    return hipGetLastError();
  });
}

hipError_t launch_polydot_extprod(const tn_plan* p, const void* a, const void* bhat, bool shared, void* c, size_t batch, size_t ins, size_t terms,
                                  u32 base_log, bool balanced, hipStream_t s) {
  if (batch == 0) return hipSuccess;
  return dispatch_fused_shape(p, [&](auto sh) { return launch_extprod_t<decltype(sh)>(p, a, bhat, shared, c, batch, ins, terms, base_log, balanced, s); });
}

}  // namespace tn
