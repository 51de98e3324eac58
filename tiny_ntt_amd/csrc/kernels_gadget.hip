// kernels_gadget.hip — gadget decomposition (gadget_decompose_kernel) and the dot product with a prepared b that cuts a into
// its digits itself (polydot_gadget_kernel), with their launchers.
#include "fused_kernels.h"

namespace tn {

// ============================================================================
// Gadget product: c[row] = sum_j digit_j(a[row]) * b[SHARED ? 0 : row][j], b given in prepared form
// ============================================================================
// digit_j(a): every coefficient of a, taken mod q, cut into base-2^w digits (gadget_canon / gadget_digit, fused_core.h;
// include/tinyntt.h has the definition): unsigned, or balanced in [-B/2, B/2) with the carry running up the digits.
//
// gadget_decompose_kernel writes the digit polynomials out: digits[row][j][i] = digit j of a[row][i].  Element-wise, one
// thread per coefficient and its `terms` digits, for every plan (the canonicalisation is the canonical policy's, as in
// pointwise_kernel).  It is the definition on the device and the baseline of the kernel below.
template <typename E>
__global__ void gadget_decompose_kernel(PlanView<E> pv, const E* __restrict__ a, E* __restrict__ digits, size_t total, u32 terms, u32 w, u32 balanced) {
  const Arith<E> ar = pv.ar;
  const u32 logn = pv.logn;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const E x = mul_tw(a[i], ar.one, ar.q);
    const size_t row = i >> logn, col = i & (((size_t)1 << logn) - 1);
    E* out = digits + ((row * terms) << logn) + col;
    u32 carry = 0;
    for (u32 j = 0; j < terms; ++j) out[(size_t)j << logn] = gadget_digit<E>(x, j * w, w, balanced != 0, carry, ar.q);
  }
}

hipError_t launch_gadget_decompose(const tn_plan* p, const void* a, void* digits, size_t batch, size_t terms, u32 base_log, bool balanced, hipStream_t s) {
  if (batch == 0) return hipSuccess;
  const size_t total = batch * p->n;
  const u32 blocks = (u32)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
  if (p->elem_bytes == 8)
    hipLaunchKernelGGL(gadget_decompose_kernel<u64>, dim3(blocks), dim3(256), 0, s, make_view<u64>(p), (const u64*)a, (u64*)digits, total, (u32)terms, base_log,
                       balanced ? 1u : 0u);
  else
    hipLaunchKernelGGL(gadget_decompose_kernel<u32>, dim3(blocks), dim3(256), 0, s, make_view<u32>(p), (const u32*)a, (u32*)digits, total, (u32)terms, base_log,
                       balanced ? 1u : 0u);
  return hipGetLastError();
}

// polydot_gadget_kernel: polydot_prepared_kernel's row loop with the digits cut out of the row of a in registers.  The fourth
// live row of that kernel (the next term's a) holds the words of a for the whole output row instead: they are requested once
// per output row (inverse_all's callback, as the dot kernel requests the next row's first term), made canonical once at the top
// of the row (gadget_canon: exact for any word) and every term's input is gadget_digit of them, so a is read once per output
// row instead of `terms` times, the digits never exist in memory and the only memory request left per term is the prepared row.
// The digits are canonical residues, below every bound the forward schedules start from (a folded word in the low half of
// the registers, any word in the rest: load_reduce), and the schedules are monotone in those bounds (the argument DESIGN.md
// 3.2a makes for prepared words), so the forward runs on them without load_reduce and no bound schedule changes.
// Balanced mode is a run-time, workgroup-uniform flag; the carry of each of the thread's R words into its next digit is one
// bit of a 32-bit mask.  Registers: the sum, the term in flight, its prepared row and the words of a: the dot kernel's four
// rows, built for the same waves per SIMD (dot_waves).  Everything else (issue points, opaque_copy for the inverse's thread
// index, no resident last-stage twiddles) is polydot_prepared_kernel's, where the reasons are given.
template <typename E, int LOGN, int LPT, bool LAZY, bool BC, bool SHARED>
__global__ void __launch_bounds__((1 << (LOGN - LPT)), (dot_waves<E, LOGN, LPT, LAZY>()))
polydot_gadget_kernel(const Arith<E> ar, const typename TwOf<E>::type* __restrict__ tab_fwd,
                      const typename TwOf<E>::type* __restrict__ tab_inv, const E* __restrict__ a, const E* __restrict__ bhat,
                      E* __restrict__ c, u32 batch, u32 terms, u32 base_log, u32 balanced, u32* sched, u32 chunk) {
  typedef FusedCfg<E, LOGN, LPT> Cfg;
  typedef Policy<E, LAZY> Pol;
  typedef typename TwOf<E>::type Tw;
  static_assert(Cfg::PHASES >= 2, "the last phase's twiddles are requested during the phase before it");
  static_assert(Cfg::R <= 32, "one carry bit per word of the thread in a 32-bit mask");
  extern __shared__ __attribute__((aligned(16))) unsigned char tn_smem[];
  const u32 tau = threadIdx.x;
  E* lds = reinterpret_cast<E*>(tn_smem);
  Tw* lds_fwd = reinterpret_cast<Tw*>(lds + Cfg::lds_elems());
  Tw* lds_inv = lds_fwd + Cfg::lds_tw_count();
  u32* lds_next = reinterpret_cast<u32*>(lds_inv + Cfg::lds_tw_count());      // output row this workgroup takes next
  for (u32 i = tau; i < (u32)Cfg::lds_tw_count(); i += Cfg::THREADS) {
    lds_fwd[i] = tab_fwd[Cfg::lds_tw_lo() + i];
    lds_inv[i] = tab_inv[Cfg::lds_tw_lo() + i];
  }
  __syncthreads();
  E acc[Cfg::R], xw[Cfg::R];                // acc: the sum of this row's products, then its result; xw: the words of a of this row
  u32 row = blockIdx.x * chunk;
  u32 taken = 1;                            // rows taken from the current chunk           (both workgroup-uniform: scalar registers)
  u32 chunk_id = blockIdx.x;                // fixed-stride mode: the chunk being processed
  if (row < batch) {
#pragma unroll
    for (int r = 0; r < Cfg::R; ++r) xw[r] = ld_operand<E, Cfg>(a, row, tau, r);
  }
  constexpr int PRE_END = Cfg::LOGN;        // no resident last-stage twiddles (polydot_prepared_kernel)
  Tw prf[Cfg::NPRE];
  constexpr bool KARG = TN_KARG_ARITH != 0;
  u32 prev = row;
  bool have_c = false;
#pragma unroll
  for (int r = 0; r < Cfg::R; ++r) acc[r] = 0;
  while (row < batch) {
    // one thread determines the next output row now; everyone reads the answer after the last term's transform
    const bool in_chunk = taken != chunk;
    taken = in_chunk ? taken + 1 : 1;
    chunk_id = in_chunk ? chunk_id : chunk_id + gridDim.x;
    if (tau == 0) *lds_next = in_chunk ? row + 1 : (sched ? gridDim.x + atomicAdd(&sched[0], 1u) : chunk_id) * chunk;
    const u32 brow = row * terms;            // row of a per-set bhat of this output row's first term (< 2^31: tn_poly_gadget_dot_prepared_dev)
    E xa[Cfg::R], xb[Cfg::R];                // the term in flight and its prepared row
    u32 tl = opaque_copy(tau);               // thread index for global addressing (see opaque_copy)
    // consume this row's words first (only their loads are in flight here: the wait is exact) and make them canonical once;
    // then issue the stores of the previous row (the first iteration writes zeros to this row's own slot, which the same
    // thread overwrites one iteration later)
#pragma unroll
    for (int r = 0; r < Cfg::R; ++r) xw[r] = gadget_canon<E, Pol>(xw[r], ar);
    sched_fence();
    st_result<E, Cfg>(c, prev, tl, acc);
#pragma unroll
    for (int r = 0; r < Cfg::R; ++r) acc[r] = 0;
    u32 carries = 0;                         // bit r: the carry of word r into its next digit (balanced mode)
    for (u32 j = 0;; ++j) {
      tl = opaque_copy(tau);
      // the term's only memory request: its prepared row, before the forward's first phase
#pragma unroll
      for (int r = 0; r < Cfg::R; ++r) xb[r] = SHARED ? ld_prepared<E, Cfg, false>(bhat, j, tl, r) : ld_prepared<E, Cfg, true>(bhat, brow + j, tl, r);
      sched_fence();
      const u32 shift = j * base_log;        // < 64 (tn_poly_gadget_dot_prepared_dev)
      u32 next_carries = 0;
#pragma unroll
      for (int r = 0; r < Cfg::R; ++r) {
        u32 cy = (carries >> r) & 1u;
        xa[r] = gadget_digit<E>(xw[r], shift, base_log, balanced != 0, cy, ar.q);
        next_carries |= cy << r;
      }
      carries = next_carries;
      const TwRefs<E> twf = {tab_fwd, lds_fwd, prf, nullptr, opaque_zero()};
      forward_range<E, Cfg, Pol, 0, Cfg::PHASES, KARG, PRE_END, BC>(xa, tau, twf, ar, lds, true, tl);
      if (j + 1 == terms) break;             // the last term's product follows the request of the inverse's twiddles, below
      if constexpr (BC) basecase<Cfg, Pol>(xa, xb, prf + Cfg::pre_off(Cfg::LOGN - 1), ar);       // (the zeta records came with prf)
      else pointwise<E, Cfg, Pol>(xa, xb, ar);
      dot_accumulate<E, Cfg, Pol>(acc, xa, ar);
      sched_fence();
    }
    __syncthreads();
    const u32 next = wave_uniform(*lds_next);
    const u32 zero = opaque_zero();
    Tw pre[Cfg::NPRE];
    dot_last_term<E, Cfg, Pol, BC>(acc, xa, xb, prf + Cfg::pre_off(Cfg::LOGN - 1), pre, tl, tab_inv, ar);
    const TwRefs<E> twi = {tab_inv, lds_inv, pre, nullptr, zero};
    inverse_all<E, Cfg, Pol, KARG, BC>(acc, opaque_copy(tau), twi, ar, lds, [&]() {
      // the next output row's words of a, requested after the inverse's own vector loads have been consumed (inverse_all); this
      // row's last digits have been taken.  Unconditional: after the last row this row's words are read again and dropped.
      const u32 nrow = next < batch ? next : row;
#pragma unroll
      for (int r = 0; r < Cfg::R; ++r) xw[r] = ld_operand<E, Cfg>(a, nrow, tl, r);
    });
    prev = row;
    have_c = true;
    row = next;
  }
  if (have_c) st_result<E, Cfg>(c, prev, tau, acc);
  rearm_row_counters(sched, tau);
}

template <typename Sh>
static hipError_t launch_gadget_t(const tn_plan* p, const void* a, const void* bhat, bool shared, void* c, size_t batch, size_t terms, u32 base_log,
                                  bool balanced, hipStream_t s) {
  typedef typename Sh::E E;
  typedef typename Sh::Cfg Cfg;
  constexpr int LOGN = Sh::LOGN, LPT = Sh::LPT;
  constexpr bool LAZY = Sh::LAZY;
  const FusedProductLaunch<Sh> L(p);
  const u32 b32 = (u32)batch, t32 = (u32)terms, bal = balanced ? 1u : 0u;
  constexpr size_t lds_bytes = fused_lds_bytes<Sh>(2);
  auto kern = shared ? polydot_gadget_kernel<E, LOGN, LPT, LAZY, false, true> : polydot_gadget_kernel<E, LOGN, LPT, LAZY, false, false>;
  if constexpr (L.HAS_BC) {
    if (L.use_bc) kern = shared ? polydot_gadget_kernel<E, LOGN, LPT, LAZY, true, true> : polydot_gadget_kernel<E, LOGN, LPT, LAZY, true, false>;
  }
  // Bytes per row: one output row is `terms` forward transforms and one inverse, the work of a row of the prepared dot product,
  // although only one row of a is read for it.  Rows are handed out to keep the rate of atomics on the one counter low against
  // the WORK between them, so the row is planned as the dot kernel's: dot_row_bytes, `terms` operand rows.
  return launch_persistent(p, s, reinterpret_cast<const void*>(kern), Cfg::THREADS, lds_bytes, dot_row_bytes(Cfg::N * sizeof(E), terms), batch, FUSED_ROWS,
                           [&](u32 grid, u32* sched, u32 chunk) {
    hipLaunchKernelGGL(kern, dim3(grid), dim3(Cfg::THREADS), lds_bytes, s, L.su.ar, L.fwd(), L.inv(),
                       (const E*)a, (const E*)bhat, (E*)c, b32, t32, base_log, bal, sched, chunk);
    return hipGetLastError();
  });
}

// terms == 1 runs the same kernel: one digit, then the prepared product
hipError_t launch_polydot_gadget(const tn_plan* p, const void* a, const void* bhat, bool shared, void* c, size_t batch, size_t terms, u32 base_log,
                                 bool balanced, hipStream_t s) {
  if (batch == 0) return hipSuccess;
  return dispatch_fused_shape(p, [&](auto sh) { return launch_gadget_t<decltype(sh)>(p, a, bhat, shared, c, batch, terms, base_log, balanced, s); });
}

// ============================================================================
// Gadget product with two output components: c[row][o] = sum_j digit_j(a[row]) * b[SHARED ? 0 : row][o][j], o < 2
// ============================================================================
// polydot_gadget2_kernel: polydot_gadget_kernel's row loop with ONE forward transform per term for both components (a key
// switch against `terms` pairs (b_j, a_j)): a is read and made canonical once per output row, every digit is cut and
// transformed once, and the transformed digit row is multiplied into two sums (dot_product_into, fused_core.h: pair by pair
// into temporaries, the digit row left as it is).  Two inverses follow; the first result is stored right behind its inverse
// (its registers are free before the second inverse needs them), the second rides to the top of the next row as the gadget
// kernel's one result does.  bhat is [sets][2][terms][n]; c is [batch][2][n].
// Registers: the two sums, the term in flight and ONE prepared row are the four rows of 128 registers.  The prepared row of
// component 0 is requested before the forward, as in the gadget kernel; the row of component 1 goes pair by pair into the
// registers component 0's product has finished with (polydot_hat_kernel's base case does the same).  The words of a, the
// gadget kernel's fourth row, stay in LDS, thread-private at [r * THREADS + tau], and are read back once per term at the
// digit cut: XL words per thread there, the rest in registers (gadget2_lds_words, fused_kernels.h: as many as the CU's LDS holds
// without a resident workgroup fewer than the gadget kernel's).
// The inverse's private twiddles: the first inverse's are requested behind the term loop, the second inverse's behind the
// first result's stores, the next row's words of a inside the second inverse (inverse_all's callback).  Requests that could be
// formed from one thread index go through copies of their own (opaque_copy): formed from the term's, the addresses of
// component 1's row and the second inverse's records (which ARE the first inverse's) were kept in registers across the
// transforms, 16 - 32 of them.  Everything else is polydot_gadget_kernel's.  All 50 instantiations hold 128 registers without
// scratch at the gadget kernel's waves per SIMD (DESIGN.md 3.2e has the report).
template <typename E, int LOGN, int LPT, bool LAZY, bool BC, bool SHARED, int XL>
__global__ void __launch_bounds__((1 << (LOGN - LPT)), (dot_waves<E, LOGN, LPT, LAZY>()))
polydot_gadget2_kernel(const Arith<E> ar, const typename TwOf<E>::type* __restrict__ tab_fwd,
                       const typename TwOf<E>::type* __restrict__ tab_inv, const E* __restrict__ a, const E* __restrict__ bhat,
                       E* __restrict__ c, u32 batch, u32 terms, u32 base_log, u32 balanced, u32* sched, u32 chunk) {
  typedef FusedCfg<E, LOGN, LPT> Cfg;
  typedef Policy<E, LAZY> Pol;
  typedef typename TwOf<E>::type Tw;
  static_assert(Cfg::PHASES >= 2, "the last phase's twiddles are requested during the phase before it");
  static_assert(Cfg::R <= 32, "one carry bit per word of the thread in a 32-bit mask");
  static_assert(XL >= 0 && XL <= Cfg::R, "words of a per thread kept in LDS");
  // A dynamic-LDS symbol of this kernel's own.  On the family's tn_smem the optimiser orders the address arithmetic of EVERY kernel in
  // the file by all uses of the symbol: with this kernel on it, seven instantiations of polydot_gadget_kernel came out 1 - 4
  // registers apart from the parent's.
  extern __shared__ __attribute__((aligned(16))) unsigned char tn_smem_pair[];
  const u32 tau = threadIdx.x;
  // LDS: [transpose image][XL * THREADS words of a][staged twiddles, forward][... inverse][next-row slot]
  E* lds = reinterpret_cast<E*>(tn_smem_pair);
  E* lds_xw = lds + Cfg::lds_elems() + tau;                                   // word r of this thread at [r * THREADS]
  Tw* lds_fwd = reinterpret_cast<Tw*>(lds + Cfg::lds_elems() + XL * Cfg::THREADS);
  Tw* lds_inv = lds_fwd + Cfg::lds_tw_count();
  u32* lds_next = reinterpret_cast<u32*>(lds_inv + Cfg::lds_tw_count());      // output row this workgroup takes next
  for (u32 i = tau; i < (u32)Cfg::lds_tw_count(); i += Cfg::THREADS) {
    lds_fwd[i] = tab_fwd[Cfg::lds_tw_lo() + i];
    lds_inv[i] = tab_inv[Cfg::lds_tw_lo() + i];
  }
  __syncthreads();
  E acc0[Cfg::R], acc1[Cfg::R], xw[Cfg::R];  // the sums of the two components, then their results; xw: the words of a of this row
  u32 row = blockIdx.x * chunk;
  u32 taken = 1;                            // rows taken from the current chunk           (both workgroup-uniform: scalar registers)
  u32 chunk_id = blockIdx.x;                // fixed-stride mode: the chunk being processed
  if (row < batch) {
#pragma unroll
    for (int r = 0; r < Cfg::R; ++r) xw[r] = ld_operand<E, Cfg>(a, row, tau, r);
  }
  constexpr int PRE_END = Cfg::LOGN;        // no resident last-stage twiddles (polydot_prepared_kernel)
  Tw prf[Cfg::NPRE];
  constexpr bool KARG = TN_KARG_ARITH != 0;
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
    // row of a per-set bhat of this output row's first term of component 0; component 1 follows `terms` rows later
    // (< 2^31: tn_poly_gadget_multidot_prepared_dev)
    const u32 brow = row * 2u * terms;
    E xa[Cfg::R], xb[Cfg::R];                // the term in flight and the prepared row of the component being multiplied
    u32 tl = opaque_copy(tau);               // thread index for global addressing (see opaque_copy)
    // consume this row's words first (only their loads are in flight here: the wait is exact), make them canonical once and
    // put XL of them away; then issue the stores of the previous row's second component (the first iteration writes zeros to
    // this row's own slot, which the same thread overwrites one iteration later)
#pragma unroll
    for (int r = 0; r < Cfg::R; ++r) {
      xw[r] = gadget_canon<E, Pol>(xw[r], ar);
      if (r < XL) lds_xw[r * Cfg::THREADS] = xw[r];
    }
    sched_fence();
    st_result<E, Cfg>(c, 2u * prev + 1u, tl, acc1);
#pragma unroll
    for (int r = 0; r < Cfg::R; ++r) { acc0[r] = 0; acc1[r] = 0; }
    u32 carries = 0;                         // bit r: the carry of word r into its next digit (balanced mode)
    // register r of the prepared row of component o, term j
    auto request1 = [&](u32 o, u32 j, u32 t, int r) {
      xb[r] = SHARED ? ld_prepared<E, Cfg, false>(bhat, o * terms + j, t, r) : ld_prepared<E, Cfg, true>(bhat, brow + o * terms + j, t, r);
    };
    // component 0's product of term j, the transformed digit row left as it is; then component 1's prepared row into the
    // registers that product has finished with
    const Tw* zeta = prf + Cfg::pre_off(Cfg::LOGN - 1);      // (the base case's zeta records came with prf)
    auto product0 = [&](u32 j) {
      dot_product_into<E, Cfg, Pol, BC>(acc0, xa, xb, zeta, ar, [&](auto i_) {
        constexpr int r = 2 * decltype(i_)::value;
        // (a thread index of its own: with the term's, the addresses of this row are formed beside component 0's and live
        //  across the forward transform; all R requests at once want R address registers at the product's peak)
        const u32 t = opaque_copy(tau);
        request1(1u, j, t, r);
        request1(1u, j, t, r + 1);
        sched_fence();
      });
    };
    // A counted loop with ONE copy of the two products, the last term's included: with the gadget kernel's form (the loop left
    // before the last term's product, which then stands a second time behind it) every 64-bit instantiation spilled at 128
    // registers (DESIGN.md 3.2e has the figures), and this form none.  The workgroup-uniform branch on the last term holds the barrier.
    u32 next = 0;
    for (u32 j = 0; j < terms; ++j) {
      tl = opaque_copy(tau);
      // component 0's prepared row, before the forward's first phase
#pragma unroll
      for (int r = 0; r < Cfg::R; ++r) request1(0u, j, tl, r);
      sched_fence();
      const u32 shift = j * base_log;        // < 64 (tn_poly_gadget_multidot_prepared_dev)
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
      if (j + 1 == terms) {                  // everyone reads the next output row behind the last term's transform, as in the gadget kernel
        __syncthreads();
        next = wave_uniform(*lds_next);
      }
      product0(j);
      if constexpr (BC) basecase<Cfg, Pol>(xa, xb, zeta, ar);      // component 1's product may overwrite the digit row: the gadget kernel's
      else pointwise<E, Cfg, Pol>(xa, xb, ar);
      dot_accumulate<E, Cfg, Pol>(acc1, xa, ar);
      sched_fence();
    }
    // the private twiddles the first inverse starts with (behind the loop: requested inside it they are live across it)
    Tw pre[Cfg::NPRE], pre1[Cfg::NPRE];
    if constexpr (BC) tw_prefetch_stages<E, Cfg, Cfg::stage_begin(Cfg::PHASES - 1), Cfg::LOGN - 1>(pre, tl, tab_inv);
    else tw_prefetch<E, Cfg>(pre, tl, tab_inv);
    sched_fence();
    const TwRefs<E> twi0 = {tab_inv, lds_inv, pre, nullptr, opaque_zero()};
    inverse_all<E, Cfg, Pol, KARG, BC>(acc0, opaque_copy(tau), twi0, ar, lds, [&]() {});
    // the first result leaves its registers here; then the second inverse's private twiddles, through a thread index of their
    // own (with the term's, they ARE the first inverse's records and stay in registers across it instead of being read again)
    tl = opaque_copy(tau);
    st_result<E, Cfg>(c, 2u * row, tl, acc0);
    sched_fence();
    if constexpr (BC) tw_prefetch_stages<E, Cfg, Cfg::stage_begin(Cfg::PHASES - 1), Cfg::LOGN - 1>(pre1, tl, tab_inv);
    else tw_prefetch<E, Cfg>(pre1, tl, tab_inv);
    sched_fence();
    const TwRefs<E> twi1 = {tab_inv, lds_inv, pre1, nullptr, opaque_zero()};
    inverse_all<E, Cfg, Pol, KARG, BC>(acc1, opaque_copy(tau), twi1, ar, lds, [&]() {
      // the next output row's words of a, requested after the inverse's own vector loads have been consumed (inverse_all); this
      // row's last digits have been taken.  Unconditional: after the last row this row's words are read again and dropped.
      const u32 nrow = next < batch ? next : row;
#pragma unroll
      for (int r = 0; r < Cfg::R; ++r) xw[r] = ld_operand<E, Cfg>(a, nrow, tl, r);
    });
    prev = row;
    have_c = true;
    row = next;
  }
  if (have_c) st_result<E, Cfg>(c, 2u * prev + 1u, tau, acc1);
  rearm_row_counters(sched, tau);
}

template <typename Sh>
static hipError_t launch_gadget2_t(const tn_plan* p, const void* a, const void* bhat, bool shared, void* c, size_t batch, size_t terms, u32 base_log,
                                   bool balanced, hipStream_t s) {
  typedef typename Sh::E E;
  typedef typename Sh::Cfg Cfg;
  constexpr int LOGN = Sh::LOGN, LPT = Sh::LPT, XL = gadget2_lds_words<Sh>();
  constexpr bool LAZY = Sh::LAZY;
  const FusedProductLaunch<Sh> L(p);
  const u32 b32 = (u32)batch, t32 = (u32)terms, bal = balanced ? 1u : 0u;
  constexpr size_t lds_bytes = fused_lds_bytes<Sh>(2, (size_t)XL * Cfg::THREADS);
  auto kern = shared ? polydot_gadget2_kernel<E, LOGN, LPT, LAZY, false, true, XL> : polydot_gadget2_kernel<E, LOGN, LPT, LAZY, false, false, XL>;
  if constexpr (L.HAS_BC) {
    if (L.use_bc) kern = shared ? polydot_gadget2_kernel<E, LOGN, LPT, LAZY, true, true, XL> : polydot_gadget2_kernel<E, LOGN, LPT, LAZY, true, false, XL>;
  }
  // Rows are planned as the gadget kernel's (dot_row_bytes, `terms` operand rows): an output row is `terms` forward transforms
  // and two inverses between two atomics, one inverse more than there.
  return launch_persistent(p, s, reinterpret_cast<const void*>(kern), Cfg::THREADS, lds_bytes, dot_row_bytes(Cfg::N * sizeof(E), terms), batch, FUSED_ROWS,
                           [&](u32 grid, u32* sched, u32 chunk) {
    hipLaunchKernelGGL(kern, dim3(grid), dim3(Cfg::THREADS), lds_bytes, s, L.su.ar, L.fwd(), L.inv(),
                       (const E*)a, (const E*)bhat, (E*)c, b32, t32, base_log, bal, sched, chunk);
    return hipGetLastError();
  });
}

hipError_t launch_polydot_gadget2(const tn_plan* p, const void* a, const void* bhat, bool shared, void* c, size_t batch, size_t terms, u32 base_log,
                                  bool balanced, hipStream_t s) {
  if (batch == 0) return hipSuccess;
  return dispatch_fused_shape(p, [&](auto sh) { return launch_gadget2_t<decltype(sh)>(p, a, bhat, shared, c, batch, terms, base_log, balanced, s); });
}

}  // namespace tn
