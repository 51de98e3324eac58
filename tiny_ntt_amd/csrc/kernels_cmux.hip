// kernels_cmux.hip — the monomial product X^e * a with an exponent per batch item (monomial_mul_kernel: every plan) and the
// CMux rotation step of a blind rotation, c = a + RGSW ⊡ ((X^e - 1) * a), from one launch (polydot_cmux_kernel: fused plans),
// with their launchers.  A translation unit of its own, with its own dynamic-LDS symbol: a kernel that shares the family's
// symbol changes the register allocation of its neighbours.  The per-word code is cmux_core.h's.
#include "fused_kernels.h"
#include "cmux_core.h"

namespace tn {

// ============================================================================
// Monomial product: out[item][g] = X^e * a[item][g] (or (X^e - 1) * a[item][g]), e = exps[item] & (2n - 1), g < group
// ============================================================================
// Element-wise: a workgroup takes rows at a grid stride, its threads the words of the row at unit stride.  The exponent is read
// from the DEVICE array once per row (the row index is workgroup-uniform: a scalar load), so a captured launch sees the
// exponents that are in the buffer at replay time.  Stores are unit-stride; the rotated loads are unit-stride apart from the
// one wrap; the own word (minus_one) is the unit-stride load.  The index is masked to the row (monomial_index): no content of
// exps addresses a word outside a.
constexpr u32 MONOMIAL_THREADS = 256;
template <typename E>
__global__ void __launch_bounds__(MONOMIAL_THREADS)
monomial_mul_kernel(const Arith<E> ar, const E* __restrict__ a, const u32* __restrict__ exps, E* __restrict__ out, u32 rows, u32 group, u32 logn,
                    u32 minus_one) {
  const u32 n = 1u << logn;
  for (u32 row = blockIdx.x; row < rows; row += gridDim.x) {
    const u32 e = wave_uniform(exps[row / group]) & (2u * n - 1u);
    const E* __restrict__ src = a + ((size_t)row << logn);
    E* __restrict__ dst = out + ((size_t)row << logn);
    for (u32 t = threadIdx.x; t < n; t += MONOMIAL_THREADS) {
      const u32 v = (t - e) & (2u * n - 1u);
      const E rot = src[monomial_index(v, logn)];
      const E own = minus_one ? src[t] : (E)0;
      __builtin_nontemporal_store(monomial_word<E>(own, rot, monomial_negated(v, logn), minus_one != 0, ar), dst + t);
    }
  }
}

template <typename E>
static hipError_t launch_monomial_t(const tn_plan* p, const void* a, const uint32_t* exps, void* out, size_t rows, size_t group, bool minus_one, hipStream_t s) {
  const size_t resident = (size_t)p->num_cus * 8;                    // 8 workgroups of 4 waves fill a CU's wave slots
  const u32 grid = (u32)(rows < resident ? rows : resident);
  hipLaunchKernelGGL(monomial_mul_kernel<E>, dim3(grid), dim3(MONOMIAL_THREADS), 0, s, plan_arith<E>(p), (const E*)a, exps, (E*)out, (u32)rows, (u32)group,
                     p->logn, minus_one ? 1u : 0u);
  return hipGetLastError();
}

// batch * group rows, below 2^31 (check_monomial)
hipError_t launch_monomial_mul(const tn_plan* p, const void* a, const uint32_t* exps, void* out, size_t batch, size_t group, bool minus_one, hipStream_t s) {
  if (batch == 0) return hipSuccess;
  return p->elem_bytes == 8 ? launch_monomial_t<u64>(p, a, exps, out, batch * group, group, minus_one, s)
                            : launch_monomial_t<u32>(p, a, exps, out, batch * group, group, minus_one, s);
}

// ============================================================================
// CMux rotation step: c[row][o] = a[row][o] + sum_{i < 2} sum_{j < terms} digit_j((X^e - 1) * a[row][i]) * b[SHARED ? 0 : row][o][i][j], o < 2
// ============================================================================
// polydot_cmux_kernel: polydot_extprod_kernel's row (kernels_extprod.hip, where the reasons for its form are given) with two
// input polynomials and three changes.
//   Exponent.  e = exps[row] & (2n - 1) is read where the row's words are requested: workgroup-uniform, a scalar load and a
//     scalar register (wave_uniform).  The next row's is read behind the second inverse, where that row's rotated words are
//     requested, and this row's again at the top of the row, where their signs are applied.
//   Input words.  An input polynomial's words are cmux_word(own word, rotated word, sign): the canonical residue of
//     (X^e - 1) * a, which is what tn_monomial_mul_dev writes, so the digits are the explicit route's.  The rotated word of
//     register r of thread tau lies at (jidx(0, tau, r) - e) & (n - 1) of the same row, its sign is bit log2 n of the
//     difference: lanes stay consecutive, the access is coalesced but not aligned and wraps once per row.  The row is read
//     twice (the own words through the streaming load, the rotated words through a plain load that may hit in L2).  The
//     second polynomial's own and rotated words are requested and consumed together behind the first's last product, as the
//     external product requests its next input; the next ROW's own words ride inside the second inverse and its rotated words
//     are requested behind that inverse and its add-in: inside it they are a fourth row of live words and cost waves per SIMD
//     in 18 instantiations instead of 4 (DESIGN.md 3.2h has the forms that were compiled).
//   Add-in.  a[row][o] is requested again inside inverse o (after_first: behind the inverse's own vector loads) and added to
//     the inverse's output with one conditional subtraction (cmux_add_in) before the result is stored or, for component 1,
//     before it waits for the store at the top of the next row.  During an inverse two rows are live (the sum being
//     inverted and, in the first, the other sum; in the second, the next row's words), so these words fit there.
// Everything else is polydot_extprod_kernel's: the LDS layout and the words put away (gadget2_lds_words), the row hand-out, the
// position of the barrier, two inverses and two stores.  2 * terms + 2 transforms per output row.
// No address depends on data except through the masked exponent: the rotated index is taken & (n - 1) of the row the own
// words come from, whatever exps holds.
template <typename E, int LOGN, int LPT, bool LAZY, bool BC, bool SHARED, int XL>
__global__ void __launch_bounds__((1 << (LOGN - LPT)), (dot_waves<E, LOGN, LPT, LAZY>()))
polydot_cmux_kernel(const Arith<E> ar, const typename TwOf<E>::type* __restrict__ tab_fwd, const typename TwOf<E>::type* __restrict__ tab_inv,
                    const E* __restrict__ a, const u32* __restrict__ exps, const E* __restrict__ bhat, E* __restrict__ c, u32 batch, u32 terms,
                    u32 base_log, u32 balanced, u32* sched, u32 chunk) {
  typedef FusedCfg<E, LOGN, LPT> Cfg;
  typedef Policy<E, LAZY> Pol;
  typedef typename TwOf<E>::type Tw;
  static_assert(Cfg::PHASES >= 2, "the last phase's twiddles are requested during the phase before it");
  static_assert(Cfg::R <= 32, "one carry bit per word of the thread in a 32-bit mask");
  static_assert(XL >= 0 && XL <= Cfg::R, "words of a per thread kept in LDS");
  static_assert(Cfg::jidx(0, 1, 0) == 1 && Cfg::jidx(0, 0, 1) == (u32)Cfg::THREADS, "phase 0: word r of thread tau is r * THREADS + tau");
  extern __shared__ __attribute__((aligned(16))) unsigned char tn_smem_cmux[];
  const u32 tau = threadIdx.x;
  // LDS: [transpose image][XL * THREADS words of a][staged twiddles, forward][... inverse][next-row slot]
  E* lds = reinterpret_cast<E*>(tn_smem_cmux);
  E* lds_xw = lds + Cfg::lds_elems() + tau;                                   // word r of this thread at [r * THREADS]
  Tw* lds_fwd = reinterpret_cast<Tw*>(lds + Cfg::lds_elems() + XL * Cfg::THREADS);
  Tw* lds_inv = lds_fwd + Cfg::lds_tw_count();
  u32* lds_next = reinterpret_cast<u32*>(lds_inv + Cfg::lds_tw_count());      // output row this workgroup takes next
  for (u32 i = tau; i < (u32)Cfg::lds_tw_count(); i += Cfg::THREADS) {
    lds_fwd[i] = tab_fwd[Cfg::lds_tw_lo() + i];
    lds_inv[i] = tab_inv[Cfg::lds_tw_lo() + i];
  }
  __syncthreads();
  constexpr u32 EMASK = 2u * (u32)Cfg::N - 1u;
  E acc0[Cfg::R], acc1[Cfg::R], xw[Cfg::R], xr[Cfg::R];  // the two sums, then their results; xw, xr: an input polynomial's own and rotated words
  u32 row = blockIdx.x * chunk;
  u32 taken = 1;                            // rows taken from the current chunk           (both workgroup-uniform: scalar registers)
  u32 chunk_id = blockIdx.x;                // fixed-stride mode: the chunk being processed
  // own and rotated words of row `arow` of a ([batch * 2][n]) under exponent e (masked), thread index th
  auto request_own = [&](u32 arow, u32 th) {
#pragma unroll
    for (int r = 0; r < Cfg::R; ++r) xw[r] = ld_operand<E, Cfg>(a, arow, th, r);
  };
  auto request_rotated = [&](u32 arow, u32 e, u32 th) {
    const u32 t0 = (th - e) & EMASK;
#pragma unroll
    for (int r = 0; r < Cfg::R; ++r) xr[r] = ld_rotated<E, Cfg>(a, arow, t0 + (u32)r * Cfg::THREADS);
  };
  if (row < batch) {
    request_own(2u * row, tau);
    request_rotated(2u * row, wave_uniform(exps[row]) & EMASK, tau);
  }
  constexpr int PRE_END = Cfg::LOGN;        // no resident last-stage twiddles (polydot_prepared_kernel)
  Tw prf[Cfg::NPRE];
  constexpr bool KARG = TN_KARG_ARITH != 0;
  const u32 comp = 2u * terms;              // prepared rows of one component of a set
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
    const u32 e = wave_uniform(exps[row]) & EMASK;       // this row's exponent: the signs of the words requested under it
    // row of a per-set bhat of this output row's first term of component 0; component 1 follows 2 * terms rows later
    // (< 2^31: tn_poly_cmux_rotate_prepared_dev)
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
    // an input's words: (X^e - 1) * a as canonical residues, once, XL of them put away
    auto put_away = [&](u32 th) {
      const u32 t0 = (th - e) & EMASK;
#pragma unroll
      for (int r = 0; r < Cfg::R; ++r) {
        xw[r] = cmux_word<E, Pol>(xw[r], xr[r], monomial_negated(t0 + (u32)r * Cfg::THREADS, Cfg::LOGN), ar);
        if (r < XL) lds_xw[r * Cfg::THREADS] = xw[r];
      }
      sched_fence();
    };
    // consume the first input's words first (only their loads are in flight here: the wait is exact); then issue the stores of
    // the previous row's second component (the first iteration writes zeros to this row's own slot, which the same thread
    // overwrites one iteration later) and clear the sums, once per output row
    put_away(tl);
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
        const u32 shift = j * base_log;      // < 64 (tn_poly_cmux_rotate_prepared_dev)
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
      if (++i == 2u) break;
      // the words of the second input polynomial of this row, requested and consumed here (polydot_extprod_kernel)
      tl = opaque_copy(tau);
      request_own(2u * row + 1u, tl);
      request_rotated(2u * row + 1u, e, tl);
      sched_fence();
      put_away(tl);
    }
    // the private twiddles the first inverse starts with (behind the loops: requested inside them they are live across them)
    Tw pre[Cfg::NPRE], pre1[Cfg::NPRE];
    if constexpr (BC) tw_prefetch_stages<E, Cfg, Cfg::stage_begin(Cfg::PHASES - 1), Cfg::LOGN - 1>(pre, tl, tab_inv);
    else tw_prefetch<E, Cfg>(pre, tl, tab_inv);
    sched_fence();
    E ad[Cfg::R];                            // the words of a[row][o] again, for the add-in behind inverse o
    const TwRefs<E> twi0 = {tab_inv, lds_inv, pre, nullptr, opaque_zero()};
    inverse_all<E, Cfg, Pol, KARG, BC>(acc0, opaque_copy(tau), twi0, ar, lds, [&]() {
#pragma unroll
      for (int r = 0; r < Cfg::R; ++r) ad[r] = ld_operand<E, Cfg>(a, 2u * row, tl, r);
    });
#pragma unroll
    for (int r = 0; r < Cfg::R; ++r) acc0[r] = cmux_add_in<E, Pol>(acc0[r], ad[r], ar);
    // the first result leaves its registers here; then the second inverse's private twiddles, through a thread index of their own
    tl = opaque_copy(tau);
    st_result<E, Cfg>(c, 2u * row, tl, acc0);
    sched_fence();
    if constexpr (BC) tw_prefetch_stages<E, Cfg, Cfg::stage_begin(Cfg::PHASES - 1), Cfg::LOGN - 1>(pre1, tl, tab_inv);
    else tw_prefetch<E, Cfg>(pre1, tl, tab_inv);
    sched_fence();
    const TwRefs<E> twi1 = {tab_inv, lds_inv, pre1, nullptr, opaque_zero()};
    const u32 nrow = next < batch ? next : row;
    inverse_all<E, Cfg, Pol, KARG, BC>(acc1, opaque_copy(tau), twi1, ar, lds, [&]() {
      // this row's second polynomial for the add-in, then the own words of the first input polynomial of the next output row,
      // requested after the inverse's own vector loads have been consumed (inverse_all); this row's last digits have been
      // taken.  Unconditional: after the last row this row's is read again and dropped.
#pragma unroll
      for (int r = 0; r < Cfg::R; ++r) ad[r] = ld_operand<E, Cfg>(a, 2u * row + 1u, tl, r);
      request_own(2u * nrow, tl);
    });
#pragma unroll
    for (int r = 0; r < Cfg::R; ++r) acc1[r] = cmux_add_in<E, Pol>(acc1[r], ad[r], ar);
    // ... and its rotated words under that row's exponent, behind the add-in: a fourth row of words inside the inverse costs
    // waves per SIMD; the row's own words were requested an inverse ago, so these may hit in L2
    sched_fence();
    request_rotated(2u * nrow, wave_uniform(exps[nrow]) & EMASK, opaque_copy(tau));
    sched_fence();
    prev = row;
    have_c = true;
    row = next;
  }
  if (have_c) st_result<E, Cfg>(c, 2u * prev + 1u, tau, acc1);
  rearm_row_counters(sched, tau);
}

template <typename Sh>
static hipError_t launch_cmux_t(const tn_plan* p, const void* a, const uint32_t* exps, const void* bhat, bool shared, void* c, size_t batch, size_t terms,
                                u32 base_log, bool balanced, hipStream_t s) {
  typedef typename Sh::E E;
  typedef typename Sh::Cfg Cfg;
  constexpr int LOGN = Sh::LOGN, LPT = Sh::LPT, XL = gadget2_lds_words<Sh>();
  constexpr bool LAZY = Sh::LAZY;
  const FusedProductLaunch<Sh> L(p);
  const u32 b32 = (u32)batch, t32 = (u32)terms, bal = balanced ? 1u : 0u;
  constexpr size_t lds_bytes = fused_lds_bytes<Sh>(2, (size_t)XL * Cfg::THREADS);
  auto kern = shared ? polydot_cmux_kernel<E, LOGN, LPT, LAZY, false, true, XL> : polydot_cmux_kernel<E, LOGN, LPT, LAZY, false, false, XL>;
  if constexpr (L.HAS_BC) {
    if (L.use_bc) kern = shared ? polydot_cmux_kernel<E, LOGN, LPT, LAZY, true, true, XL> : polydot_cmux_kernel<E, LOGN, LPT, LAZY, true, false, XL>;
  }
  // Rows are planned as the external product's with two inputs: an output row is 2 * terms forward transforms and two
  // inverses between two atomics.
  return launch_persistent(p, s, reinterpret_cast<const void*>(kern), Cfg::THREADS, lds_bytes, dot_row_bytes(Cfg::N * sizeof(E), 2 * terms), batch,
                           FUSED_ROWS, [&](u32 grid, u32* sched, u32 chunk) {
    hipLaunchKernelGGL(kern, dim3(grid), dim3(Cfg::THREADS), lds_bytes, s, L.su.ar, L.fwd(), L.inv(),
                       (const E*)a, exps, (const E*)bhat, (E*)c, b32, t32, base_log, bal, sched, chunk);
    return hipGetLastError();
  });
}

hipError_t launch_polydot_cmux(const tn_plan* p, const void* a, const uint32_t* exps, const void* bhat, bool shared, void* c, size_t batch, size_t terms,
                               u32 base_log, bool balanced, hipStream_t s) {
  if (batch == 0) return hipSuccess;
  return dispatch_fused_shape(p, [&](auto sh) { return launch_cmux_t<decltype(sh)>(p, a, exps, bhat, shared, c, batch, terms, base_log, balanced, s); });
}

}  // namespace tn
