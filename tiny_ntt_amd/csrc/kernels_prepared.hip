// kernels_prepared.hip — prepared operand: the product with b transformed ahead of time (prepare_fused_kernel,
// polymul_prepared_kernel) and the sum of such products under one inverse transform (polydot_prepared_kernel), with their
// launchers.  The format of a prepared row: ld_prepared, fused_kernels.h.
#include "fused_kernels.h"

namespace tn {

// ============================================================================
// Prepared operand: the product with b transformed ahead of time
// ============================================================================
// bhat[row] = prepared form of b[row].  Persistent workgroups, rows handed out and prefetched as in ntt_fused_kernel.
// BC: the plan's product runs the base case: tab is its psi_bc table and the forward stops one stage early.
template <typename E, int LOGN, int LPT, bool LAZY, bool BC>
__global__ void __launch_bounds__((1 << (LOGN - LPT)), (LPT >= 4 ? 2 : TN_FUSED_MIN_WAVES))
prepare_fused_kernel(const Arith<E> ar, const typename TwOf<E>::type* __restrict__ tab, const E* __restrict__ b, E* __restrict__ bhat, u32 batch,
                     u32* sched, u32 chunk) {
  typedef FusedCfg<E, LOGN, LPT> Cfg;
  typedef Policy<E, LAZY> Pol;
  typedef typename TwOf<E>::type Tw;
  static_assert(Cfg::PHASES >= 2, "the last phase's twiddles are requested during the phase before it");
  extern __shared__ __attribute__((aligned(16))) unsigned char tn_smem[];
  E* lds = reinterpret_cast<E*>(tn_smem);
  const u32 tau = threadIdx.x;
  // LDS: [transpose image][staged twiddles][2 next-row slots]
  Tw* lds_tab = reinterpret_cast<Tw*>(lds + Cfg::lds_elems());
  u32* lds_next = reinterpret_cast<u32*>(lds_tab + Cfg::lds_tw_count());
  for (u32 i = tau; i < (u32)Cfg::lds_tw_count(); i += Cfg::THREADS) lds_tab[i] = tab[Cfg::lds_tw_lo() + i];
  u32 left = chunk - 1, chunk_id = blockIdx.x;            // take_next_row
  if (tau == 0) take_next_row(left, chunk_id, lds_next, 1u, blockIdx.x * chunk, sched, chunk);
  __syncthreads();
  u32 next = wave_uniform(lds_next[1]);
  E xn[Cfg::R];
  u32 row = blockIdx.x * chunk;
  if (row < batch) {
#pragma unroll
    for (int r = 0; r < Cfg::R; ++r) xn[r] = ld_operand<E, Cfg>(b, row, tau, r);
  }
  for (u32 it = 0; row < batch; ++it) {
    if (tau == 0) take_next_row(left, chunk_id, lds_next, it & 1u, next, sched, chunk);      // read back after this row's barriers
    E x[Cfg::R];
#pragma unroll
    for (int r = 0; r < Cfg::R; ++r) x[r] = xn[r];
    sched_fence();
    if (next < batch) {
#pragma unroll
      for (int r = 0; r < Cfg::R; ++r) xn[r] = ld_operand<E, Cfg>(b, next, tau, r);
    }
    sched_fence();
    load_reduce<E, Cfg, Pol>(x, ar);
    {
      Tw pre[Cfg::NPRE];
      const TwRefs<E> tw = {tab, lds_tab, pre, nullptr, 0};
      forward_range<E, Cfg, Pol, 0, Cfg::PHASES, false, Cfg::LOGN, BC>(x, tau, tw, ar, lds, true, tau);
    }
    E* out = bhat + ((size_t)row << Cfg::LOGN);
#pragma unroll
    for (int r = 0; r < Cfg::R; ++r) out[Cfg::prep_idx(tau, r)] = Pol::canon(x[r], ar);
    __syncthreads();                                     // (single-wave workgroups have no barrier inside the transposes)
    row = next;
    next = wave_uniform(lds_next[it & 1u]);
  }
  rearm_row_counters(sched, tau);
}

// c[row] = a[row] * b[SHARED ? 0 : row] with b given in prepared form: polymul_fused_kernel without b's forward transform.
// The row loop is that kernel's: this row's a was requested during the previous row's inverse, the previous row's result is
// stored at the top of the iteration, the twiddles of the middle phases are staged in LDS and the arithmetic constants are read
// per phase (kernarg_arith).  a runs all its forward phases in one go (there is no second transform to share twiddles with).
// SHARED: every row is multiplied by the ONE prepared row, which the workgroup loads into registers once before the row loop
// (R words per thread, ordinary loads: every workgroup reads the same row, so it should stay in L2); otherwise row `row` of
// bhat is streamed like an operand, requested at the top of the iteration and needed only after a's transform.
#ifndef TN_PREPARED_SHARED_WAVES
#define TN_PREPARED_SHARED_WAVES 4   // waves per SIMD of the SHARED kernel where the product kernel is built for more (n = 4096 / 64-bit lazy: 6): the
                                     //    R resident words of the prepared row do not fit 80 registers (52 B / 212 B of scratch per lane without /
                                     //    with the base case); at 4 (128 registers) nothing spills
#endif
template <typename E, int LOGN, int LPT, bool LAZY, bool SHARED>
constexpr int prepared_waves() {
  return SHARED && polymul_waves<E, LOGN, LPT, LAZY>() > TN_PREPARED_SHARED_WAVES ? TN_PREPARED_SHARED_WAVES : polymul_waves<E, LOGN, LPT, LAZY>();
}
template <typename E, int LOGN, int LPT, bool LAZY, bool BC, bool SHARED>
__global__ void __launch_bounds__((1 << (LOGN - LPT)), (prepared_waves<E, LOGN, LPT, LAZY, SHARED>()))
polymul_prepared_kernel(const Arith<E> ar, const typename TwOf<E>::type* __restrict__ tab_fwd,
                        const typename TwOf<E>::type* __restrict__ tab_inv, const E* __restrict__ a, const E* __restrict__ bhat,
                        E* __restrict__ c, u32 batch, u32* sched, u32 chunk) {
  typedef FusedCfg<E, LOGN, LPT> Cfg;
  typedef Policy<E, LAZY> Pol;
  typedef typename TwOf<E>::type Tw;
  static_assert(Cfg::PHASES >= 2, "the last phase's twiddles are requested during the phase before it");
  extern __shared__ __attribute__((aligned(16))) unsigned char tn_smem[];
  const u32 tau = threadIdx.x;
  E* lds = reinterpret_cast<E*>(tn_smem);
  Tw* lds_fwd = reinterpret_cast<Tw*>(lds + Cfg::lds_elems());
  Tw* lds_inv = lds_fwd + Cfg::lds_tw_count();
  u32* lds_next = reinterpret_cast<u32*>(lds_inv + Cfg::lds_tw_count());      // row index this workgroup takes next
  for (u32 i = tau; i < (u32)Cfg::lds_tw_count(); i += Cfg::THREADS) {
    lds_fwd[i] = tab_fwd[Cfg::lds_tw_lo() + i];
    lds_inv[i] = tab_inv[Cfg::lds_tw_lo() + i];
  }
  __syncthreads();
  E xa[Cfg::R], xb[Cfg::R], xn[Cfg::R];      // xa: the row in flight, then its result; xb: the prepared operand; xn: the next row's a
  u32 row = blockIdx.x * chunk;
  u32 taken = 1;                            // rows taken from the current chunk           (both workgroup-uniform: scalar registers)
  u32 chunk_id = blockIdx.x;                // fixed-stride mode: the chunk being processed
  if (row < batch) {
#pragma unroll
    for (int r = 0; r < Cfg::R; ++r) xn[r] = ld_operand<E, Cfg>(a, row, tau, r);
    if constexpr (SHARED) {
#pragma unroll
      for (int r = 0; r < Cfg::R; ++r) xb[r] = ld_prepared<E, Cfg, false>(bhat, 0, tau, r);
    }
  }
  // the thread-private twiddles of the last forward stage stay in registers across rows where the budget allows (polymul_fused_kernel)
  constexpr int PRE_END = (TN_RESIDENT_TW && polymul_waves<E, LOGN, LPT, LAZY>() <= 4 && Cfg::stage_end(Cfg::PHASES - 1) - Cfg::stage_begin(Cfg::PHASES - 1) >= 2) ? Cfg::LOGN - 1 : Cfg::LOGN;
  Tw prf[Cfg::NPRE];
  tw_prefetch_stages<E, Cfg, PRE_END, Cfg::LOGN>(prf, tau, tab_fwd);
  u32 prev = row;
  bool have_c = false;
#pragma unroll
  for (int r = 0; r < Cfg::R; ++r) xa[r] = 0;
  while (row < batch) {
    const u32 zero = opaque_zero();
    const u32 tl = opaque_copy(tau);         // thread index for global addressing within this row (see opaque_copy)
    // one thread determines the next row now; everyone reads the answer after a's transform (barriers in between)
    const bool in_chunk = taken != chunk;
    taken = in_chunk ? taken + 1 : 1;
    chunk_id = in_chunk ? chunk_id : chunk_id + gridDim.x;
    if (tau == 0) *lds_next = in_chunk ? row + 1 : (sched ? gridDim.x + atomicAdd(&sched[0], 1u) : chunk_id) * chunk;
    // consume this row's a first (only its loads are in flight here: the wait is exact), then issue the stores of the previous
    // row (the first iteration writes zeros to this row's own slot, which the same thread overwrites one iteration later) and
    // the loads of the prepared row
    E xt[Cfg::R];
#pragma unroll
    for (int r = 0; r < Cfg::R; ++r) xt[r] = xn[r];
    load_reduce<E, Cfg, Pol>(xt, ar);
    sched_fence();
    st_result<E, Cfg>(c, prev, tl, xa);
    if constexpr (!SHARED) {
#pragma unroll
      for (int r = 0; r < Cfg::R; ++r) xb[r] = ld_prepared<E, Cfg, true>(bhat, row, tl, r);
    }
    sched_fence();
#pragma unroll
    for (int r = 0; r < Cfg::R; ++r) xa[r] = xt[r];
    constexpr bool KARG = TN_KARG_ARITH != 0;
    const TwRefs<E> twf = {tab_fwd, lds_fwd, prf, nullptr, zero};
    forward_range<E, Cfg, Pol, 0, Cfg::PHASES, KARG, PRE_END, BC>(xa, tau, twf, ar, lds, true, tl);
    __syncthreads();
    const u32 next = wave_uniform(*lds_next);
    // the inverse starts with the thread-private phase: request its twiddles before the product
    Tw pre[Cfg::NPRE];
    if constexpr (BC) {
      basecase<Cfg, Pol>(xa, xb, prf + Cfg::pre_off(Cfg::LOGN - 1), ar);       // (the zeta records came with prf)
      sched_fence();
      tw_prefetch_stages<E, Cfg, Cfg::stage_begin(Cfg::PHASES - 1), Cfg::LOGN - 1>(pre, tl, tab_inv);
    } else {
      tw_prefetch<E, Cfg>(pre, tl, tab_inv);
      pointwise<E, Cfg, Pol>(xa, xb, ar);
    }
    const TwRefs<E> twi = {tab_inv, lds_inv, pre, nullptr, zero};
    inverse_all<E, Cfg, Pol, KARG, BC>(xa, tau, twi, ar, lds, [&]() {
      // next row's a, requested after the inverse's own vector loads have been consumed (inverse_all).  Unconditional: after
      // the last row this row's a is read again and dropped.
      const u32 nrow = next < batch ? next : row;
#pragma unroll
      for (int r = 0; r < Cfg::R; ++r) xn[r] = ld_operand<E, Cfg>(a, nrow, tl, r);
    });
    prev = row;
    have_c = true;
    row = next;
  }
  if (have_c) st_result<E, Cfg>(c, prev, tau, xa);
  rearm_row_counters(sched, tau);
}

// bhat: nullptr -> prepare (in = b, out = bhat); otherwise the product (in = a, out = c)
template <typename Sh>
static hipError_t launch_prepared_t(const tn_plan* p, const void* in, const void* bhat, bool shared, void* out, size_t batch, hipStream_t s) {
  typedef typename Sh::E E;
  typedef typename Sh::Cfg Cfg;
  constexpr int LOGN = Sh::LOGN, LPT = Sh::LPT;
  constexpr bool LAZY = Sh::LAZY;
  const FusedProductLaunch<Sh> L(p);
  const u32 b32 = (u32)batch;
  if (!bhat) {
    constexpr size_t lds_bytes = fused_lds_bytes<Sh>(1);
    auto kern = prepare_fused_kernel<E, LOGN, LPT, LAZY, false>;
    if constexpr (L.HAS_BC) { if (L.use_bc) kern = prepare_fused_kernel<E, LOGN, LPT, LAZY, true>; }
    return launch_persistent(p, s, reinterpret_cast<const void*>(kern), Cfg::THREADS, lds_bytes, Cfg::N * sizeof(E), batch, FUSED_ROWS,
                             [&](u32 grid, u32* sched, u32 chunk) {
      hipLaunchKernelGGL(kern, dim3(grid), dim3(Cfg::THREADS), lds_bytes, s, L.su.ar, L.fwd(), (const E*)in, (E*)out, b32, sched, chunk);
      return hipGetLastError();
    });
  }
  constexpr size_t lds_bytes = fused_lds_bytes<Sh>(2);
  auto kern = shared ? polymul_prepared_kernel<E, LOGN, LPT, LAZY, false, true> : polymul_prepared_kernel<E, LOGN, LPT, LAZY, false, false>;
  if constexpr (L.HAS_BC) {
    if (L.use_bc) kern = shared ? polymul_prepared_kernel<E, LOGN, LPT, LAZY, true, true> : polymul_prepared_kernel<E, LOGN, LPT, LAZY, true, false>;
  }
  return launch_persistent(p, s, reinterpret_cast<const void*>(kern), Cfg::THREADS, lds_bytes, Cfg::N * sizeof(E), batch, FUSED_ROWS,
                           [&](u32 grid, u32* sched, u32 chunk) {
    hipLaunchKernelGGL(kern, dim3(grid), dim3(Cfg::THREADS), lds_bytes, s, L.su.ar, L.fwd(), L.inv(),
                       (const E*)in, (const E*)bhat, (E*)out, b32, sched, chunk);
    return hipGetLastError();
  });
}

hipError_t launch_prepare(const tn_plan* p, const void* b, void* bhat, size_t rows, hipStream_t s) {
  if (rows == 0) return hipSuccess;
  return dispatch_fused_shape(p, [&](auto sh) { return launch_prepared_t<decltype(sh)>(p, b, nullptr, false, bhat, rows, s); });
}
hipError_t launch_polymul_prepared(const tn_plan* p, const void* a, const void* bhat, bool shared, void* c, size_t batch, hipStream_t s) {
  if (batch == 0) return hipSuccess;
  return dispatch_fused_shape(p, [&](auto sh) { return launch_prepared_t<decltype(sh)>(p, a, bhat, shared, c, batch, s); });
}

// ============================================================================
// Prepared dot product: c[row] = sum_j a[row][j] * b[SHARED ? 0 : row][j], b given in prepared form
// ============================================================================
// polymul_prepared_kernel's row loop per OUTPUT row, with a run-time loop over the row's terms: every term runs one forward
// transform and the product (pointwise() / basecase()) against its prepared row, the products are summed as canonical
// residues (dot_accumulate, fused_core.h) and ONE inverse transform runs on the sum: terms + 1 transforms per output row.
// The inverse is linear, and with the base case the sum is taken over residues mod y^2 - zeta, where it is linear too.
// Issue points: term j's prepared row is requested first and term j + 1's a behind it (vector-memory operations return in
// order, and the prepared row is needed first), both at the top of the term, before the forward's first phase, as
// polymul_fused_kernel requests b: by the time the forward fetches its last phase's twiddles they have long arrived.  The
// next output row's first a is requested inside the inverse (inverse_all's callback) and the result is stored at the top of
// the next row.  SHARED: the set of `terms` prepared rows is the same for every output row; it does not fit registers for
// terms > 1, so each term reads its row with ordinary cached loads (every workgroup reads the same rows: L2); otherwise
// row `row * terms + j` is streamed like an operand.
// Registers: the sum, the term in flight, its prepared row and the next term's a are 4 R live words, so every shape is built
// for at most TN_DOT_WAVES waves per SIMD (128 registers), like the SHARED prepared kernel.
template <typename E, int LOGN, int LPT, bool LAZY, bool BC, bool SHARED>
__global__ void __launch_bounds__((1 << (LOGN - LPT)), (dot_waves<E, LOGN, LPT, LAZY>()))
polydot_prepared_kernel(const Arith<E> ar, const typename TwOf<E>::type* __restrict__ tab_fwd,
                        const typename TwOf<E>::type* __restrict__ tab_inv, const E* __restrict__ a, const E* __restrict__ bhat,
                        E* __restrict__ c, u32 batch, u32 terms, u32* sched, u32 chunk) {
  typedef FusedCfg<E, LOGN, LPT> Cfg;
  typedef Policy<E, LAZY> Pol;
  typedef typename TwOf<E>::type Tw;
  static_assert(Cfg::PHASES >= 2, "the last phase's twiddles are requested during the phase before it");
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
  E acc[Cfg::R], xn[Cfg::R];                // acc: the sum of this row's products, then its result; xn: the next term's a
  u32 row = blockIdx.x * chunk;
  u32 taken = 1;                            // rows taken from the current chunk           (both workgroup-uniform: scalar registers)
  u32 chunk_id = blockIdx.x;                // fixed-stride mode: the chunk being processed
  if (row < batch) {
#pragma unroll
    for (int r = 0; r < Cfg::R; ++r) xn[r] = ld_operand<E, Cfg>(a, row * terms, tau, r);
  }
  // every term fetches all the thread-private twiddles of its last forward phase: keeping the last stage's in registers across
  // rows (TN_RESIDENT_TW) spilled 36 / 44 B per lane at n = 512 / 2048 with 64-bit lazy lanes, next to the four live rows
  constexpr int PRE_END = Cfg::LOGN;
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
    const u32 arow = row * terms;            // row of a, and of a per-set bhat, of this output row's first term (< 2^31: tn_poly_dot_prepared_dev)
    E xa[Cfg::R], xb[Cfg::R];                // the term in flight and its prepared row
    u32 tl;
    for (u32 j = 0;; ++j) {
      tl = opaque_copy(tau);                 // thread index for global addressing within this term (see opaque_copy)
      // consume this term's a first (only its loads are in flight here: the wait is exact); before the first term, issue the
      // stores of the previous row (the first iteration writes zeros to this row's own slot, which the same thread overwrites
      // one iteration later); then request the prepared row and, behind it, the next term's a
      E xt[Cfg::R];
#pragma unroll
      for (int r = 0; r < Cfg::R; ++r) xt[r] = xn[r];
      load_reduce<E, Cfg, Pol>(xt, ar);
      sched_fence();
      if (j == 0) {
        st_result<E, Cfg>(c, prev, tl, acc);
#pragma unroll
        for (int r = 0; r < Cfg::R; ++r) acc[r] = 0;
      }
#pragma unroll
      for (int r = 0; r < Cfg::R; ++r) xb[r] = SHARED ? ld_prepared<E, Cfg, false>(bhat, j, tl, r) : ld_prepared<E, Cfg, true>(bhat, arow + j, tl, r);
      if (j + 1 < terms) {
#pragma unroll
        for (int r = 0; r < Cfg::R; ++r) xn[r] = ld_operand<E, Cfg>(a, arow + j + 1, tl, r);
      }
      sched_fence();
#pragma unroll
      for (int r = 0; r < Cfg::R; ++r) xa[r] = xt[r];
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
    // (the thread index through opaque_copy: the inverse's LDS addresses are recomputed per row, not kept in registers across
    //  the row loop, where one of them was spilled at n = 4096 / 64-bit lazy with the base case and reloaded behind a vmcnt(0))
    inverse_all<E, Cfg, Pol, KARG, BC>(acc, opaque_copy(tau), twi, ar, lds, [&]() {
      // the next output row's first a, requested after the inverse's own vector loads have been consumed (inverse_all).
      // Unconditional: after the last row this row's first a is read again and dropped.
      const u32 nrow = (next < batch ? next : row) * terms;
#pragma unroll
      for (int r = 0; r < Cfg::R; ++r) xn[r] = ld_operand<E, Cfg>(a, nrow, tl, r);
    });
    prev = row;
    have_c = true;
    row = next;
  }
  if (have_c) st_result<E, Cfg>(c, prev, tau, acc);
  rearm_row_counters(sched, tau);
}

template <typename Sh>
static hipError_t launch_dot_t(const tn_plan* p, const void* a, const void* bhat, bool shared, void* c, size_t batch, size_t terms, hipStream_t s) {
  typedef typename Sh::E E;
  typedef typename Sh::Cfg Cfg;
  constexpr int LOGN = Sh::LOGN, LPT = Sh::LPT;
  constexpr bool LAZY = Sh::LAZY;
  const FusedProductLaunch<Sh> L(p);
  const u32 b32 = (u32)batch, t32 = (u32)terms;
  constexpr size_t lds_bytes = fused_lds_bytes<Sh>(2);
  auto kern = shared ? polydot_prepared_kernel<E, LOGN, LPT, LAZY, false, true> : polydot_prepared_kernel<E, LOGN, LPT, LAZY, false, false>;
  if constexpr (L.HAS_BC) {
    if (L.use_bc) kern = shared ? polydot_prepared_kernel<E, LOGN, LPT, LAZY, true, true> : polydot_prepared_kernel<E, LOGN, LPT, LAZY, true, false>;
  }
  // one output row is `terms` operand rows of work: rows are handed out in chunks of at least FUSED_ROWS.chunk_bytes of a
  return launch_persistent(p, s, reinterpret_cast<const void*>(kern), Cfg::THREADS, lds_bytes, dot_row_bytes(Cfg::N * sizeof(E), terms), batch, FUSED_ROWS,
                           [&](u32 grid, u32* sched, u32 chunk) {
    hipLaunchKernelGGL(kern, dim3(grid), dim3(Cfg::THREADS), lds_bytes, s, L.su.ar, L.fwd(), L.inv(),
                       (const E*)a, (const E*)bhat, (E*)c, b32, t32, sched, chunk);
    return hipGetLastError();
  });
}

hipError_t launch_polydot_prepared(const tn_plan* p, const void* a, const void* bhat, bool shared, void* c, size_t batch, size_t terms, hipStream_t s) {
  if (batch == 0) return hipSuccess;
  if (terms == 1) return launch_polymul_prepared(p, a, bhat, shared, c, batch, s);       // the same kernel, bits and speed as a single product
  return dispatch_fused_shape(p, [&](auto sh) { return launch_dot_t<decltype(sh)>(p, a, bhat, shared, c, batch, terms, s); });
}

}  // namespace tn
