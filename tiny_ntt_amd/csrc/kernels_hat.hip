// kernels_hat.hip — transform domain: the dot product of prepared rows (polydot_hat_kernel) and the way back from a prepared
// row to coefficients (unprepare_fused_kernel), with their launchers.
#include "fused_kernels.h"

namespace tn {

// ============================================================================
// Transform domain: prepared rows in, prepared rows or coefficients out
// ============================================================================
// Both operands of polydot_hat_kernel are prepared rows and unprepare_fused_kernel turns a prepared row back into
// coefficients: no forward transform runs in this file.  Canonical words (what the library writes into a prepared row) are
// below every bound the product and the inverse schedules start from (fused_core.h: dot_accumulate), so the
// schedules of polymul_fused_kernel run unchanged.  No address depends on a loaded word.
template <typename E, typename Cfg>
__device__ __forceinline__ void st_prepared(E* __restrict__ c, u32 row, u32 tau, const E (&x)[Cfg::R]) {
  const size_t off = (size_t)row << Cfg::LOGN;
#pragma unroll
  for (int r = 0; r < Cfg::R; ++r) {
#if TN_NT_STREAM
    __builtin_nontemporal_store(x[r], uniform_ptr(c + off + Cfg::prep_idx(0, r)) + Cfg::prep_idx(tau, 0));
#else
    c[off + Cfg::prep_idx(tau, r)] = x[r];
#endif
  }
}

// x[row] = the polynomial whose prepared form is xhat[row]: prepare_fused_kernel's mirror.  Persistent workgroups, rows handed
// out and prefetched as there.  The R words at prep_idx ARE the last phase's register layout (no natural-order image and no
// extra transpose, unlike the cg_intt mode of ntt_fused_kernel); the inverse then runs on the plan's inverse table, one stage
// short and with (n/2)^-1 where the plan's product runs the base case (BC), and the result is stored in natural order.
template <typename E, int LOGN, int LPT, bool LAZY, bool BC>
__global__ void __launch_bounds__((1 << (LOGN - LPT)), (LPT >= 4 ? 2 : TN_FUSED_MIN_WAVES))
unprepare_fused_kernel(const Arith<E> ar, const typename TwOf<E>::type* __restrict__ tab, const E* __restrict__ xhat, E* __restrict__ out, u32 batch,
                       u32* sched, u32 chunk) {
  typedef FusedCfg<E, LOGN, LPT> Cfg;
  typedef Policy<E, LAZY> Pol;
  typedef typename TwOf<E>::type Tw;
  extern __shared__ __attribute__((aligned(16))) unsigned char tn_smem[];
  E* lds = reinterpret_cast<E*>(tn_smem);
  const u32 tau = threadIdx.x;
  // LDS: [transpose image][staged twiddles of the inverse table][2 next-row slots]
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
    for (int r = 0; r < Cfg::R; ++r) xn[r] = ld_prepared<E, Cfg, true>(xhat, row, tau, r);
  }
  for (u32 it = 0; row < batch; ++it) {
    if (tau == 0) take_next_row(left, chunk_id, lds_next, it & 1u, next, sched, chunk);      // read back after this row's barriers
    // (as in the product kernel: an opaque zero / thread index per row keep the uniform twiddle loads, the arithmetic constants
    //  and the row addresses inside the row loop instead of in registers across it: without them the n = 8192 / 64-bit lazy
    //  kernel spilled 116 B per lane)
    const u32 zero = opaque_zero();
    const u32 tl = opaque_copy(tau);
    constexpr bool KARG = TN_KARG_ARITH != 0;
    E x[Cfg::R];
#pragma unroll
    for (int r = 0; r < Cfg::R; ++r) x[r] = xn[r];
    sched_fence();
    // the inverse starts with the thread-private phase: its twiddles first, the next row behind them (vector-memory
    // operations return in order: inverse_all)
    Tw pre[Cfg::NPRE];
    tw_prefetch_stages<E, Cfg, Cfg::stage_begin(Cfg::PHASES - 1), BC ? Cfg::LOGN - 1 : Cfg::LOGN>(pre, tl, tab);
    const TwRefs<E> tw = {tab, lds_tab, pre, nullptr, zero};
    inverse_all<E, Cfg, Pol, KARG, BC>(x, tau, tw, ar, lds, [&]() {
      if (next < batch) {
#pragma unroll
        for (int r = 0; r < Cfg::R; ++r) xn[r] = ld_prepared<E, Cfg, true>(xhat, next, tl, r);
      }
    });
    st_result<E, Cfg>(out, row, tl, x);
    __syncthreads();                                     // (single-wave workgroups have no barrier inside the transposes)
    row = next;
    next = wave_uniform(lds_next[it & 1u]);
  }
  rearm_row_counters(sched, tau);
}

// out[row] = sum_j a[row][j] * b[SHARED ? 0 : row][j] with BOTH operands prepared: polydot_prepared_kernel's row loop without
// load_reduce and forward_range.  Per term: the two prepared rows (ahat row * terms + j streamed; bhat row j through cached
// loads when SHARED, as there, otherwise row * terms + j streamed), pointwise() / basecase_each(), dot_accumulate.
// INV: one inverse transform on the sum, stored in natural order (the coefficients).  !INV: the canonical sum is stored at
// prep_idx, which by linearity is the prepared row of that result: no transform, no LDS table and no LDS image.
// Issue points: the next term's two rows are requested before this term's product (ahat first: loads return in order and
// the product's first use is of a); the next output row's first pair inside the inverse (inverse_all's callback) or, without
// an inverse, with the last product; the result is stored at the top of the next row.  Base case: the requests go pair by
// pair BEHIND the product of each register pair, into the registers it has just finished with, and the sum is taken pair by
// pair too: requested up front, five rows were live during the product (60-68 B per lane of scratch, reloaded behind a
// vmcnt(0): profiles/hat_domain_ab.txt).
// The base case's zeta records (stage LOGN - 1 of psi_bc) used to arrive with the forward's last-phase prefetch; they do not
// depend on the row.  Each thread fetches its R / 2 records once per workgroup and keeps them in LDS (n / 2 records, read
// back one at a time just before their pair): resident in registers they cost 16 of the 128 and 36-52 B per lane spilled.
// The next-row slot is double-buffered: without an inverse there is one workgroup barrier per row, and two slots keep thread
// 0's write of row k + 2's index behind every wave's read of row k's (ntt_fused_kernel).
template <typename E, int LOGN, int LPT, bool LAZY, bool BC, bool SHARED, bool INV>
__global__ void __launch_bounds__((1 << (LOGN - LPT)), (dot_waves<E, LOGN, LPT, LAZY>()))
polydot_hat_kernel(const Arith<E> ar, const typename TwOf<E>::type* __restrict__ tab_fwd, const typename TwOf<E>::type* __restrict__ tab_inv,
                   const E* __restrict__ ahat, const E* __restrict__ bhat, E* __restrict__ out, u32 batch, u32 terms, u32* sched, u32 chunk) {
  typedef FusedCfg<E, LOGN, LPT> Cfg;
  typedef Policy<E, LAZY> Pol;
  typedef typename TwOf<E>::type Tw;
  extern __shared__ __attribute__((aligned(16))) unsigned char tn_smem[];
  E* lds = reinterpret_cast<E*>(tn_smem);
  const u32 tau = threadIdx.x;
  // LDS: [INV: transpose image][INV: staged twiddles of the inverse table][BC: n / 2 zeta records][2 next-row slots]
  Tw* lds_inv = reinterpret_cast<Tw*>(lds + (INV ? Cfg::lds_elems() : 0));
  Tw* lds_zeta = lds_inv + (INV ? Cfg::lds_tw_count() : 0);
  u32* lds_next = reinterpret_cast<u32*>(lds_zeta + (BC ? Cfg::N / 2 : 0));
  if constexpr (INV) {
    for (u32 i = tau; i < (u32)Cfg::lds_tw_count(); i += Cfg::THREADS) lds_inv[i] = tab_inv[Cfg::lds_tw_lo() + i];
  }
  if constexpr (BC) {                       // record i of thread tau at [i * THREADS + tau]; only that thread reads it back
    Tw zt[Cfg::NPRE];
    tw_prefetch_stages<E, Cfg, Cfg::LOGN - 1, Cfg::LOGN>(zt, tau, tab_fwd);
#pragma unroll
    for (int i = 0; i < Cfg::R / 2; ++i) lds_zeta[i * Cfg::THREADS + tau] = zt[Cfg::pre_off(Cfg::LOGN - 1) + i];
  }
  __syncthreads();
  const Tw* zeta = lds_zeta + tau;
  E acc[Cfg::R], xna[Cfg::R], xnb[Cfg::R];  // acc: the sum of this row's products, then its result; xna, xnb: the next term's rows
  u32 row = blockIdx.x * chunk;
  u32 taken = 1;                            // rows taken from the current chunk           (both workgroup-uniform: scalar registers)
  u32 chunk_id = blockIdx.x;                // fixed-stride mode: the chunk being processed
  // term j of the output row whose first row of ahat is arow: register r of both rows / both rows
  auto request1 = [&](u32 arow, u32 j, u32 t, int r) {
    xna[r] = ld_prepared<E, Cfg, true>(ahat, arow + j, t, r);
    xnb[r] = SHARED ? ld_prepared<E, Cfg, false>(bhat, j, t, r) : ld_prepared<E, Cfg, true>(bhat, arow + j, t, r);
  };
  auto request = [&](u32 arow, u32 j, u32 t) {
#pragma unroll
    for (int r = 0; r < Cfg::R; ++r) xna[r] = ld_prepared<E, Cfg, true>(ahat, arow + j, t, r);
#pragma unroll
    for (int r = 0; r < Cfg::R; ++r) xnb[r] = SHARED ? ld_prepared<E, Cfg, false>(bhat, j, t, r) : ld_prepared<E, Cfg, true>(bhat, arow + j, t, r);
  };
  // acc += the product of the term in flight; REQ: term j of row arow is requested meanwhile (see above)
  auto term = [&](E (&xa)[Cfg::R], const E (&xb)[Cfg::R], auto req_, u32 arow, u32 j, u32 t) {
    constexpr bool REQ = decltype(req_)::value;
    if constexpr (BC) {
      basecase_each<Cfg, Pol, Cfg::THREADS>(xa, xb, zeta, ar, [&](auto i_) {
        constexpr int r = 2 * decltype(i_)::value;
        acc[r] = dot_accumulate_one<E, Pol>(acc[r], xa[r], ar);
        acc[r + 1] = dot_accumulate_one<E, Pol>(acc[r + 1], xa[r + 1], ar);
        if constexpr (REQ) {
          sched_fence();
          request1(arow, j, t, r);
          request1(arow, j, t, r + 1);
        }
        sched_fence();
      });
    } else {
      if constexpr (REQ) {
        request(arow, j, t);
        sched_fence();
      }
      pointwise<E, Cfg, Pol>(xa, xb, ar);
      dot_accumulate<E, Cfg, Pol>(acc, xa, ar);
    }
  };
  if (row < batch) request(row * terms, 0, tau);
  constexpr bool KARG = TN_KARG_ARITH != 0;
  u32 prev = row, slot = 0;
  bool have_c = false;
#pragma unroll
  for (int r = 0; r < Cfg::R; ++r) acc[r] = 0;
  while (row < batch) {
    // one thread determines the next output row now; everyone reads the answer before the last term's product
    const bool in_chunk = taken != chunk;
    taken = in_chunk ? taken + 1 : 1;
    chunk_id = in_chunk ? chunk_id : chunk_id + gridDim.x;
    if (tau == 0) lds_next[slot] = in_chunk ? row + 1 : (sched ? gridDim.x + atomicAdd(&sched[0], 1u) : chunk_id) * chunk;
    const u32 arow = row * terms;            // row of ahat, and of a per-set bhat, of this output row's first term (< 2^31: tn_poly_dot_hat_dev)
    E xa[Cfg::R], xb[Cfg::R];                // the term in flight
    u32 tl;
    for (u32 j = 0;; ++j) {
      tl = opaque_copy(tau);                 // thread index for global addressing within this term (see opaque_copy)
      // consume this term's rows first (only their loads are in flight here: the wait is exact); before the first term, issue
      // the stores of the previous row (the first iteration writes zeros to this row's own slot, which the same thread
      // overwrites one iteration later); then the product, with the next term's rows requested
#pragma unroll
      for (int r = 0; r < Cfg::R; ++r) { xa[r] = xna[r]; xb[r] = xnb[r]; }
      sched_fence();
      if (j == 0) {
        if constexpr (INV) st_result<E, Cfg>(out, prev, tl, acc);
        else st_prepared<E, Cfg>(out, prev, tl, acc);
#pragma unroll
        for (int r = 0; r < Cfg::R; ++r) acc[r] = 0;
      }
      if (j + 1 == terms) break;             // the last term's product follows the read of the next output row, below
      term(xa, xb, std::true_type(), arow, j + 1, tl);
      sched_fence();
    }
    __syncthreads();
    const u32 next = wave_uniform(lds_next[slot]);
    slot ^= 1u;
    // Unconditional: after the last row this row's first pair is read again and dropped.
    const u32 nrow = (next < batch ? next : row) * terms;
    if constexpr (INV) {
      const u32 zero = opaque_zero();
      // the inverse starts with the thread-private phase: request its twiddles around the last product, as polydot_prepared_kernel does
      Tw pre[Cfg::NPRE];
      if constexpr (BC) {
        term(xa, xb, std::false_type(), 0u, 0u, tl);
        sched_fence();
        tw_prefetch_stages<E, Cfg, Cfg::stage_begin(Cfg::PHASES - 1), Cfg::LOGN - 1>(pre, tl, tab_inv);
      } else {
        tw_prefetch<E, Cfg>(pre, tl, tab_inv);
        term(xa, xb, std::false_type(), 0u, 0u, tl);
      }
      const TwRefs<E> twi = {tab_inv, lds_inv, pre, nullptr, zero};
      // (the thread index through opaque_copy: polydot_prepared_kernel)
      inverse_all<E, Cfg, Pol, KARG, BC>(acc, opaque_copy(tau), twi, ar, lds, [&]() { request(nrow, 0, tl); });
    } else {
      sched_fence();
      term(xa, xb, std::true_type(), nrow, 0u, tl);
    }
    prev = row;
    have_c = true;
    row = next;
  }
  if (have_c) {
    if constexpr (INV) st_result<E, Cfg>(out, prev, tau, acc);
    else st_prepared<E, Cfg>(out, prev, tau, acc);
  }
  rearm_row_counters(sched, tau);
}

// bhat == nullptr: unprepare (in = xhat, out = x); otherwise the dot product of prepared rows (in = ahat)
template <typename Sh>
static hipError_t launch_hat_t(const tn_plan* p, const void* in, const void* bhat, bool shared, void* out, size_t batch, size_t terms, bool inv,
                               hipStream_t s) {
  typedef typename Sh::E E;
  typedef typename Sh::Cfg Cfg;
  typedef typename TwOf<E>::type Tw;
  constexpr int LOGN = Sh::LOGN, LPT = Sh::LPT;
  constexpr bool LAZY = Sh::LAZY;
  const FusedProductLaunch<Sh> L(p);
  const u32 b32 = (u32)batch, t32 = (u32)terms;
  constexpr size_t lds_inverse = fused_lds_bytes<Sh>(1);
  if (!bhat) {
    auto kern = unprepare_fused_kernel<E, LOGN, LPT, LAZY, false>;
    if constexpr (L.HAS_BC) { if (L.use_bc) kern = unprepare_fused_kernel<E, LOGN, LPT, LAZY, true>; }
    return launch_persistent(p, s, reinterpret_cast<const void*>(kern), Cfg::THREADS, lds_inverse, Cfg::N * sizeof(E), batch, FUSED_ROWS,
                             [&](u32 grid, u32* sched, u32 chunk) {
      hipLaunchKernelGGL(kern, dim3(grid), dim3(Cfg::THREADS), lds_inverse, s, L.su.ar, L.inv(), (const E*)in, (E*)out, b32, sched, chunk);
      return hipGetLastError();
    });
  }
  const size_t lds_bytes = (inv ? lds_inverse : 16) + (L.use_bc ? (size_t)(Cfg::N / 2) * sizeof(Tw) : 0);        // + the base case's zeta records
  auto pick = [&](auto bc_) {
    constexpr bool BC = decltype(bc_)::value;
    if (inv) return shared ? polydot_hat_kernel<E, LOGN, LPT, LAZY, BC, true, true> : polydot_hat_kernel<E, LOGN, LPT, LAZY, BC, false, true>;
    return shared ? polydot_hat_kernel<E, LOGN, LPT, LAZY, BC, true, false> : polydot_hat_kernel<E, LOGN, LPT, LAZY, BC, false, false>;
  };
  auto kern = pick(std::false_type());
  if constexpr (L.HAS_BC) { if (L.use_bc) kern = pick(std::true_type()); }
  // one output row is `terms` rows of each operand: planned like the prepared dot product's rows
  return launch_persistent(p, s, reinterpret_cast<const void*>(kern), Cfg::THREADS, lds_bytes, dot_row_bytes(Cfg::N * sizeof(E), terms), batch, FUSED_ROWS,
                           [&](u32 grid, u32* sched, u32 chunk) {
    hipLaunchKernelGGL(kern, dim3(grid), dim3(Cfg::THREADS), lds_bytes, s, L.su.ar, L.fwd(), L.inv(),
                       (const E*)in, (const E*)bhat, (E*)out, b32, t32, sched, chunk);
    return hipGetLastError();
  });
}

hipError_t launch_unprepare(const tn_plan* p, const void* xhat, void* x, size_t rows, hipStream_t s) {
  if (rows == 0) return hipSuccess;
  return dispatch_fused_shape(p, [&](auto sh) { return launch_hat_t<decltype(sh)>(p, xhat, nullptr, false, x, rows, 1, true, s); });
}
hipError_t launch_polydot_hat(const tn_plan* p, const void* ahat, const void* bhat, bool shared, void* out, size_t batch, size_t terms, bool out_prepared,
                              hipStream_t s) {
  if (batch == 0) return hipSuccess;
  return dispatch_fused_shape(p, [&](auto sh) { return launch_hat_t<decltype(sh)>(p, ahat, bhat, shared, out, batch, terms, !out_prepared, s); });
}

}  // namespace tn
