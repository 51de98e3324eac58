// fused_kernels.h — what more than one family of fused kernels uses: the build switches, the transforms on the register-tiled
// machinery of fused_core.h, the row accessors, the row hand-out of the persistent workgroups, and the host side every
// launcher shares (shape dispatch, launch preamble, dynamic-LDS size).  One translation unit per family includes it:
//   kernels.hip           the product kernel, the standalone transforms, the dispatcher of the constant-geometry kernels and
//                         the element-wise / checker / benchmark kernels
//   kernels_prepared.hip  prepared operand: prepare, the product and the dot product with b prepared
//   kernels_hat.hip       transform domain: both operands prepared; unprepare
//   kernels_gadget.hip    gadget decomposition and the dot product that decomposes a itself
//   kernels_extprod.hip   external product: the digits of all input polynomials of a row into both output components
//   kernels_cmux.hip      CMux rotation step: the external product of (X^e - 1) * a, added to a
//   kernels_blindrot.hip  blind rotation: CMux rotation steps with the accumulator kept in LDS
//   kernels_galoisks.hip  automorphism key switch: sigma_g on the load, the two-component gadget product, the add-in at the store
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>
#include "plan.h"
#include "dev_addr.h"

#ifndef TN_ABL_NO_BARRIER
#define TN_ABL_NO_BARRIER 0      // timing ablation: cross-wave transposes without workgroup barriers (wrong results)
#endif
#ifndef TN_ABL_ROWMASK
#define TN_ABL_ROWMASK 0         // timing ablation: rows & mask -> operands and results stay in L2 (no HBM traffic; wrong results)
#endif
#ifndef TN_ABL_NO_GLOBAL
#define TN_ABL_NO_GLOBAL 0       // timing ablation: operands synthesised in registers instead of loaded from HBM
#endif
#ifndef TN_STORE_AT_TOP
#define TN_STORE_AT_TOP 1        // 1: row k's result is stored at the top of iteration k+1 (see the kernel's comment)
#endif
#ifndef TN_NT_STREAM
#define TN_NT_STREAM 1           // 1: non-temporal loads/stores for the streamed operands a, b, c
#endif
#ifndef TN_FUSED_MIN_WAVES
#define TN_FUSED_MIN_WAVES 4     // waves per SIMD the register allocator must leave room for (4 -> <= 128 VGPRs)
#endif
#ifndef TN_POLYMUL60_WAVES
#define TN_POLYMUL60_WAVES 6     // the same for the benchmark-shape product kernel (n = 4096, 64-bit lanes, lazy): 6 -> <= 80 VGPRs, three
                                 //    512-thread workgroups per CU (3 x 51,204 B of LDS).  Measured +3 % over 4 (profiles/r2_h_*): the extra
                                 //    waves fill the issue slots the barriers and LDS round trips leave (10 % fewer cycles per launch) and the
                                 //    power cap gives two thirds of that back as clock (2.06 -> 1.92 GHz at 1.39 kW)
#endif

#ifndef TN_NTTF_PIN_LOGN
#define TN_NTTF_PIN_LOGN 99      // standalone transforms: from this log2 n on, loop invariants are pinned inside the row loop (ntt_fused_kernel).  Off:
                                 // pinning removes the 60-68 B/lane of scratch of the n = 8192 kernels and is SLOWER (0.408 vs 0.428, profiles/r3_n8192_ab.txt)
#endif
#ifndef TN_VEC_PREFETCH
#define TN_VEC_PREFETCH 1         // 1: twiddles of a vector-loaded phase (n = 8192) are requested one transpose ahead (28 more registers across it)
#endif
#ifndef TN_FUSED_CIN
#define TN_FUSED_CIN 0           // 1: also build the n = 4096 / 64-bit product kernel whose bound schedule assumes canonical inputs (see launch_fused_t)
#endif
#ifndef TN_SADDR
#define TN_SADDR 1               // 1: operand rows are addressed as scalar base (+ register offset, scalar unit) + 32-bit thread offset
#endif
#ifndef TN_KARG_ARITH
#define TN_KARG_ARITH 1          // 1: the product kernel reads its arithmetic constants and scalar twiddles per phase (kernarg_arith)
#endif
#ifndef TN_RESIDENT_TW
#define TN_RESIDENT_TW 1         // 1: the thread-private twiddles of the LAST forward stage (4 of the 7 records of the last phase; they do
                                 //    not depend on the row) stay in registers across rows of the persistent loop: 64 fewer bytes per
                                 //    thread and row from L2.  Only where the register budget is 128 (polymul_waves() <= 4): worth 0.8 %,
                                 //    against the 3 % of the third workgroup per CU that those 16 registers would cost
#endif
#ifndef TN_SHARE_MID_TW
#define TN_SHARE_MID_TW 1        // 1: ... and the phase before it (twiddles staged in LDS) likewise: a: ph 0-1, b: ph 0-1, a: ph 2, b: ph 2, b: ph 3, a: ph 3
#endif
#ifndef TN_SHARE_LAST_TW
#define TN_SHARE_LAST_TW 1       // 1: a and b run their last forward phase back to back on ONE fetch of its thread-private twiddles
#endif
#ifdef TN_MARKS
#define TN_MARK(n) asm volatile("; TNMARK " n)
#else
#define TN_MARK(n)
#endif
namespace tn {

// ============================================================================
// Transforms
// ============================================================================
// One LDS transpose between register layouts.  Data that crosses waves needs workgroup
// barriers on all three sides (the buffer is shared with the wave-private transposes before
// and after); a wave-local transpose only needs the compiler not to reorder it (the LDS
// operations of one wave execute in issue order and touch that wave's private region).
#ifndef TN_SHUFFLE_LAST
#define TN_SHUFFLE_LAST 0        // developer A/B (profiles/r3_shuffle_ab.txt): 1 = the LAST transpose of a transform (an 8 x 8 transpose between the
                                 // register index and the low three lane bits) through DPP lane permutes instead of LDS
#endif
// 8 x 8 transpose between registers and groups of 8 neighbouring lanes, without LDS: three butterfly stages; in stage b a lane
// and its partner (lane ^ 2^b) exchange, for every register pair (r, r | 2^b), the register the other one needs.  Per pair and
// 32-bit half: one select of what to send, the permute (quad_perm for distances 1 and 2; row_shl:4 / row_shr:4 under
// complementary bank masks for distance 4), two selects of what to keep.
template <int DIST> __device__ __forceinline__ u32 lane_xor(u32 v) {
  if constexpr (DIST == 1) return (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xf, 0xf, false);         // quad_perm [1,0,3,2]
  else if constexpr (DIST == 2) return (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xf, 0xf, false);    // quad_perm [2,3,0,1]
  else {
    int r = __builtin_amdgcn_update_dpp(0, (int)v, 0x104, 0xf, 0x5, false);                                     // row_shl:4 -> banks 0, 2 (lane i <- lane i + 4)
    return (u32)__builtin_amdgcn_update_dpp(r, (int)v, 0x114, 0xf, 0xA, false);                                 // row_shr:4 -> banks 1, 3 (lane i <- lane i - 4)
  }
}
template <typename E>
__device__ __forceinline__ void transpose8_lanes(E (&x)[8], u32 lane) {
  static_for<0, 3>([&](auto b_) {
    constexpr int b = decltype(b_)::value, m = 1 << b;
    const bool hi = (lane >> b) & 1u;
    static_for<0, 8>([&](auto r_) {
      constexpr int r0 = decltype(r_)::value;
      if constexpr (!(r0 & m)) {
        constexpr int r1 = r0 | m;
        const E send = hi ? x[r0] : x[r1];
        E recv;
        if constexpr (sizeof(E) == 8) recv = ((u64)lane_xor<m>((u32)(send >> 32)) << 32) | lane_xor<m>((u32)send);
        else recv = lane_xor<m>((u32)send);
        x[r0] = hi ? recv : x[r0];
        x[r1] = hi ? x[r1] : recv;
      }
    });
  });
}

template <typename E, typename Cfg, int EX, int FROM, int TO>
__device__ __forceinline__ void exchange(E (&x)[Cfg::R], u32 tau, E* lds) {
  if constexpr (TN_SHUFFLE_LAST && Cfg::LPT == 3 && EX == Cfg::PHASES - 2 && Cfg::pos(EX + 1) == 0 && Cfg::pos(EX) == Cfg::LPT) {
    // register index <-> lane bits [0, 3): jidx(EX) = (tau >> 3) << 6 | r << 3 | (tau & 7),  jidx(EX + 1) = tau << 3 | r
    transpose8_lanes<E>(x, tau);
  } else if constexpr (Cfg::ex_wave_local(EX)) {
    __builtin_amdgcn_wave_barrier();
    ex_store<E, Cfg, EX, FROM>(x, tau, lds);
    __builtin_amdgcn_wave_barrier();     // lanes read what OTHER lanes of the wave wrote: loads may not move above the stores
    ex_load<E, Cfg, EX, TO>(x, tau, lds);
    __builtin_amdgcn_wave_barrier();
  } else {
#if TN_ABL_NO_BARRIER
    __builtin_amdgcn_wave_barrier();
    ex_store<E, Cfg, EX, FROM>(x, tau, lds);
    __builtin_amdgcn_wave_barrier();
    ex_load<E, Cfg, EX, TO>(x, tau, lds);
    __builtin_amdgcn_wave_barrier();
#else
    __syncthreads();
    ex_store<E, Cfg, EX, FROM>(x, tau, lds);
    __syncthreads();
    ex_load<E, Cfg, EX, TO>(x, tau, lds);
    __syncthreads();
#endif
  }
}

// The kernel's Arith argument as it lies in the kernel-argument segment (first argument of every fused kernel), addressed
// through an opaque zero: fields are then read by scalar loads AFTER the point where `zero` was defined, i.e. per phase,
// instead of living in SGPRs (or, spilled, in VGPR lanes) across the whole persistent row loop.
template <typename E>
__device__ __forceinline__ const Arith<E>& kernarg_arith(u32 zero) {
  typedef const __attribute__((address_space(4))) char* KP;
  return *(const Arith<E>*)((KP)__builtin_amdgcn_kernarg_segment_ptr() + zero);
}

// Forward transform, phases [P0, P1).  The thread-private twiddles of the last phase live in tw.pre[]; with `fetch_pre` they
// are requested from L2 just before the transpose that precedes that phase, so their latency hides behind it.
// KARG: take the arithmetic constants and the scalar twiddles of each phase through a fresh opaque zero (see kernarg_arith).
// BC: the base-case product's incomplete transform (fwd_phase).
template <typename E, typename Cfg, typename Pol, int P0, int P1, bool KARG = false, int PRE_END = Cfg::LOGN, bool BC = false>
__device__ __forceinline__ void forward_range(E (&x)[Cfg::R], u32 tau, const TwRefs<E>& tw_in, const Arith<E>& ar_in, E* lds, bool fetch_pre,
                                              u32 tau_g) {      // tau_g: the thread index again, for global addressing (opaque_copy)
  typename TwOf<E>::type vec[Cfg::R];        // twiddles of a vector-loaded phase (n = 8192), requested one transpose ahead
  static_for<P0, P1>([&](auto p_) {
    constexpr int p = decltype(p_)::value;
    constexpr bool FULL = Cfg::stage_end(p) - Cfg::stage_begin(p) == Cfg::LPT;
    TN_MARK("fwd_phase");
    TwRefs<E> tw = tw_in;
    if constexpr (KARG) tw.zero = opaque_zero();
    if constexpr (TN_VEC_PREFETCH && Cfg::tw_src(p) == Cfg::TW_VEC && FULL && p > P0) tw.mid = vec;
    const Arith<E>& ar = KARG ? kernarg_arith<E>(tw.zero) : ar_in;
    fwd_phase<E, Cfg, Pol, p, BC>(x, tau, tw, ar);
    TN_MARK("fwd_other");
    if constexpr (p == Cfg::PHASES - 2) {
      if (fetch_pre) {
        sched_fence();                 // request the last phase's private twiddles; they fly during the transpose
        tw_prefetch_stages<E, Cfg, Cfg::stage_begin(Cfg::PHASES - 1), PRE_END>(tw.pre, tau_g, tw.glob);   // (stages >= PRE_END: resident)
        sched_fence();
      }
    }
    if constexpr (p + 1 < P1) {
      constexpr int pn = p + 1 < Cfg::PHASES ? p + 1 : p;
      if constexpr (TN_VEC_PREFETCH && Cfg::tw_src(pn) == Cfg::TW_VEC && Cfg::stage_end(pn) - Cfg::stage_begin(pn) == Cfg::LPT) {
        sched_fence();
        tw_fetch_vec<E, Cfg, pn>(vec, tau_g, tw.glob);
        sched_fence();
      }
    }
    if constexpr (p + 1 < Cfg::PHASES) exchange<E, Cfg, p, p, p + 1>(x, tau, lds);
  });
}
template <typename E, typename Cfg, typename Pol>
__device__ __forceinline__ void forward_all(E (&x)[Cfg::R], u32 tau, const typename TwOf<E>::type* __restrict__ glob,
                                            const typename TwOf<E>::type* lds_tw, const Arith<E>& ar, E* lds, u32 zero = 0) {
  typename TwOf<E>::type pre[Cfg::NPRE];
  const TwRefs<E> tw = {glob, lds_tw, pre, nullptr, zero};
  forward_range<E, Cfg, Pol, 0, Cfg::PHASES>(x, tau, tw, ar, lds, true, tau);
}

// Inverse transform.  `after_first` runs once the first phase (the one whose thread-private
// twiddles come from L2 through vector loads) has been computed: vector-memory operations
// complete in order, so the long-latency HBM prefetch of the next row must be issued AFTER
// those twiddle loads have been consumed, or every wave would wait for HBM at the top of the inverse.
template <typename E, typename Cfg, typename Pol, bool KARG = false, bool BC = false, typename F>
__device__ __forceinline__ void inverse_all(E (&x)[Cfg::R], u32 tau, const TwRefs<E>& tw_in, const Arith<E>& ar_in, E* lds,
                                            F&& after_first) {
  typename TwOf<E>::type vec[Cfg::R];        // twiddles of a vector-loaded phase (n = 8192), requested one transpose ahead
  static_for<0, Cfg::PHASES>([&](auto i_) {
    constexpr int p = Cfg::PHASES - 1 - decltype(i_)::value;
    constexpr bool FULL = Cfg::stage_end(p) - Cfg::stage_begin(p) == Cfg::LPT;
    TN_MARK("inv_phase");
    TwRefs<E> tw = tw_in;
    if constexpr (KARG) tw.zero = opaque_zero();
    if constexpr (TN_VEC_PREFETCH && Cfg::tw_src(p) == Cfg::TW_VEC && FULL && p < Cfg::PHASES - 1) tw.mid = vec;
    const Arith<E>& ar = KARG ? kernarg_arith<E>(tw.zero) : ar_in;
    inv_phase<E, Cfg, Pol, p, BC>(x, tau, tw, ar);
    TN_MARK("inv_other");
    // (the next phase's vector-loaded twiddles are requested BEFORE the next row's HBM prefetch: vector-memory operations return
    //  in order, and behind the prefetch the phase would wait for HBM: n = 8192 cg_intt, profiles/r3_n8192_ab.txt)
    if constexpr (p > 0) {
      constexpr int pn = p > 0 ? p - 1 : 0;
      if constexpr (TN_VEC_PREFETCH && Cfg::tw_src(pn) == Cfg::TW_VEC && Cfg::stage_end(pn) - Cfg::stage_begin(pn) == Cfg::LPT) {
        sched_fence();
        tw_fetch_vec<E, Cfg, pn>(vec, tau, tw.glob);
        sched_fence();
      }
    }
    if constexpr (p == Cfg::PHASES - 1) { sched_fence(); after_first(); sched_fence(); }
    if constexpr (p > 0) exchange<E, Cfg, p - 1, p, p - 1>(x, tau, lds);
  });
}

template <typename E> struct alignas(2 * sizeof(E)) PairOf { E lo, hi; };

// ============================================================================
// Rows in HBM
// ============================================================================
template <typename E, typename Cfg>
__device__ __forceinline__ E ld_operand(const E* __restrict__ p, u32 row, u32 tau, int r) {
#if TN_ABL_NO_GLOBAL
  return (E)(tau * 2654435761u + 7 * r + row);
#else
#if TN_ABL_ROWMASK
  row &= TN_ABL_ROWMASK;
#endif
#if TN_NT_STREAM
  // address = (row base + the register's offset: wave-uniform, scalar unit) + the thread's offset (ONE vector register for all
  // R accesses); written out so the compiler does not keep one vector offset per 8 KiB of row (loop invariants it then spills)
  const TN_GLOBAL_AS E* rp = uniform_ptr(p + ((size_t)row << Cfg::LOGN) + Cfg::jidx(0, 0, r));
  return __builtin_nontemporal_load(rp + (Cfg::jidx(0, tau, 0) & (u32)(Cfg::N - 1)));   // streamed once: keep L2 for the twiddle tables
#else
  return p[((size_t)row << Cfg::LOGN) + Cfg::jidx(0, tau, r)];
#endif
#endif
}

// Word (v mod n) of row `row` of p: the load of a row rotated by a monomial (kernels_cmux.hip, kernels_pack.hip; cmux_core.h's
// monomial_index).  The index is MASKED to the row: no v addresses a word outside it.  A plain load: the row is read again by
// the unit-stride load and may hit in L2.
template <typename E, typename Cfg>
__device__ __forceinline__ E ld_rotated(const E* __restrict__ p, u32 row, u32 v) {
  const TN_GLOBAL_AS E* rp = uniform_ptr(p + ((size_t)row << Cfg::LOGN));
  return rp[v & (u32)(Cfg::N - 1)];
}

template <typename E, typename Cfg>
__device__ __forceinline__ void st_result(E* __restrict__ c, u32 row, u32 tau, const E (&x)[Cfg::R]) {
#if TN_ABL_ROWMASK
  row &= TN_ABL_ROWMASK;
#endif
  const size_t off = (size_t)row << Cfg::LOGN;
#pragma unroll
  for (int r = 0; r < Cfg::R; ++r) {
#if TN_NT_STREAM
    __builtin_nontemporal_store(x[r], uniform_ptr(c + off + Cfg::jidx(0, 0, r)) + (Cfg::jidx(0, tau, 0) & (u32)(Cfg::N - 1)));
#else
    c[off + Cfg::jidx(0, tau, r)] = x[r];
#endif
  }
}

// A prepared row holds what polymul_fused_kernel of the same plan has in xb just before pointwise() / basecase(): b's
// negacyclic transform (stopped one stage early where the plan runs the base case), as canonical residues, word
// FusedCfg::prep_idx(tau, r) = register r of thread tau of the last phase.  Canonical words are within every bound the
// product's schedules assume for xb (pointwise(): any value below 14 q; basecase(): any word; 32-bit lanes fold), so the
// products on prepared rows run on the schedules of polymul_fused_kernel unchanged.
template <typename E, typename Cfg, bool NT>
__device__ __forceinline__ E ld_prepared(const E* __restrict__ p, u32 row, u32 tau, int r) {
  if constexpr (NT && TN_NT_STREAM) {      // a row streamed once: addressed like an operand row (ld_operand)
    const TN_GLOBAL_AS E* rp = uniform_ptr(p + ((size_t)row << Cfg::LOGN) + Cfg::prep_idx(0, r));
    return __builtin_nontemporal_load(rp + Cfg::prep_idx(tau, 0));
  } else {
    return p[((size_t)row << Cfg::LOGN) + Cfg::prep_idx(tau, r)];
  }
}

// waves per SIMD the product kernel's register allocation leaves room for (16 coeff/thread shapes need > 128 VGPRs)
template <typename E, int LOGN, int LPT, bool LAZY>
constexpr int polymul_waves() {
  return LPT >= 4 ? 2 : (sizeof(E) == 8 && LOGN == 12 && LAZY) ? TN_POLYMUL60_WAVES : TN_FUSED_MIN_WAVES;
}
// ... and the dot-product kernels': the sum, the term in flight, its prepared row and the next term's a (or the words of a, or
// the next pair of prepared rows) are 4 R live words, so every shape is built for at most TN_DOT_WAVES waves per SIMD (128
// registers), like the SHARED prepared kernel.
#ifndef TN_DOT_WAVES
#define TN_DOT_WAVES 4
#endif
template <typename E, int LOGN, int LPT, bool LAZY>
constexpr int dot_waves() {
  return polymul_waves<E, LOGN, LPT, LAZY>() > TN_DOT_WAVES ? TN_DOT_WAVES : polymul_waves<E, LOGN, LPT, LAZY>();
}

// ============================================================================
// Row hand-out of the persistent workgroups (device side of launch_persistent, plan.h, and plan_rows, launch_plan.h)
// ============================================================================
// Rows come in chunks of `chunk` consecutive rows: chunk blockIdx.x first, then whatever the device-wide counter sched[0]
// hands out (atomicAdd): a workgroup on a slower CU / XCD simply takes fewer chunks, so the launch ends when the work does,
// not when the slowest fixed share does.  (chunk > 1 for short rows keeps the rate of atomics on that one address low.)
// sched == nullptr: fixed stride over chunks.  Two forms.  The product-family kernels publish the next row at the top of a
// row and read it behind the row's barriers: that form is written out in each of them (polymul_fused_kernel has the comments;
// as a function it changed the code of polydot_hat_kernel).  The other form:
//
// take_next_row: for kernels that prefetch the next row's input at the TOP of a row and so need its index one row ahead
// (the standalone transforms, prepare, unprepare).  Thread 0 alone keeps the bookkeeping and asks one iteration ahead: before
// the loop for the second row (slot 1), at the top of iteration `it` for the row after the next (slot it & 1); everyone reads
// slot it & 1 at the bottom of the iteration, behind its barrier(s).  Two slots, so that this is the only barrier needed.
// State, in the kernel: left = chunk - 1, chunk_id = blockIdx.x (thread 0's copies are the ones used).
__device__ __forceinline__ void take_next_row(u32& left, u32& chunk_id, u32* lds_next, u32 slot, u32 cur, u32* sched, u32 chunk) {      // thread 0 only
  if (left) { --left; lds_next[slot] = cur + 1; }
  else {
    chunk_id = sched ? gridDim.x + atomicAdd(&sched[0], 1u) : chunk_id + gridDim.x;
    left = chunk - 1;
    lds_next[slot] = chunk_id * chunk;
  }
}

// the last workgroup to run out of rows re-arms the counters for the next launch that uses this slot
__device__ __forceinline__ void rearm_row_counters(u32* sched, u32 tau) {
  if (sched && tau == 0 && atomicAdd(&sched[1], 1u) == gridDim.x - 1) { sched[0] = 0; sched[1] = 0; }
}

// ============================================================================
// What the dot-product kernels with a forward transform per term share (polydot_prepared_kernel, polydot_gadget_kernel)
// ============================================================================
// The last term of an output row: its product, the request of the private twiddles the inverse starts with (before the
// product; with the base case behind it: the inverse's private phase has one stage less, and the zeta records came with prf),
// and the sum.  zeta: the base case's records within prf; pre: what the inverse's TwRefs then points to.
template <typename E, typename Cfg, typename Pol, bool BC>
__device__ __forceinline__ void dot_last_term(E (&acc)[Cfg::R], E (&xa)[Cfg::R], const E (&xb)[Cfg::R], const typename TwOf<E>::type* zeta,
                                              typename TwOf<E>::type (&pre)[Cfg::NPRE], u32 tl, const typename TwOf<E>::type* tab_inv,
                                              const Arith<E>& ar) {
  if constexpr (BC) {
    basecase<Cfg, Pol>(xa, xb, zeta, ar);
    sched_fence();
    tw_prefetch_stages<E, Cfg, Cfg::stage_begin(Cfg::PHASES - 1), Cfg::LOGN - 1>(pre, tl, tab_inv);
  } else {
    tw_prefetch<E, Cfg>(pre, tl, tab_inv);
    pointwise<E, Cfg, Pol>(xa, xb, ar);
  }
  dot_accumulate<E, Cfg, Pol>(acc, xa, ar);
}

// ============================================================================
// Host side of every fused launcher
// ============================================================================
// f(FusedShape of the plan), or hipErrorInvalidValue for a plan without fused kernels.  The shapes are named in launch_plan.h
// (with_fused_shape).  PRODUCT: the caller is the product launcher.  Developer builds with -DTN_ONLY_MAIN (tools/asm_main.sh)
// instantiate only its n = 4096 / 64-bit lazy shape; every other launcher returns hipErrorInvalidValue there and instantiates
// nothing.
template <bool PRODUCT = false, typename F>
inline hipError_t dispatch_fused_shape(const tn_plan* p, F&& f) {
#ifdef TN_ONLY_MAIN
  if constexpr (PRODUCT) { if (p->elem_bytes == 8 && p->lazy && p->logn == 12) return f(FusedShape<u64, 12, true>()); }
  return hipErrorInvalidValue;
#else
  return with_fused_shape(p->elem_bytes, p->lazy, p->logn, hipErrorInvalidValue, f);
#endif
}

// What a launch of the product family (product, prepared operand, transform domain, gadget) takes from the plan; use_bc by
// the family's one rule (launch_plan.h: fused_use_bc).
template <typename Sh> struct FusedProductLaunch {
  typedef typename Sh::E E;
  typedef typename TwOf<E>::type Tw;
  static constexpr bool HAS_BC = Sh::HAS_BC;
  const PlanView<E> pv;
  const bool use_bc;
  const FusedProductSetup<E> su;
  explicit FusedProductLaunch(const tn_plan* p, bool cyclic = false, bool no_bc = false)
      : pv(make_view<E>(p)), use_bc(fused_use_bc<Sh>(p->bc_ok, no_bc)), su(fused_product_setup(pv.ar, use_bc, cyclic)) {}
  const Tw* fwd() const { return fused_table(pv, su.fwd); }
  const Tw* inv() const { return fused_table(pv, su.inv); }
};

// Dynamic LDS of a fused kernel: the transpose image (+ extra_elems more words), `tables` staged twiddle tables, the next-row slots
template <typename Sh>
constexpr size_t fused_lds_bytes(int tables, size_t extra_elems = 0) {
  typedef typename Sh::Cfg Cfg;
  return ((size_t)Cfg::lds_elems() + extra_elems) * sizeof(typename Sh::E) + (size_t)tables * Cfg::lds_tw_count() * sizeof(typename TwOf<typename Sh::E>::type) + 16;
}

// Words of a per thread that the kernels with two sums (polydot_gadget2_kernel, polydot_extprod_kernel) keep in LDS instead of
// registers: as many as the CU's LDS holds without a resident workgroup fewer than the gadget kernel's.
constexpr size_t GADGET2_CU_LDS = 160 * 1024;
template <typename Sh> constexpr int gadget2_lds_words() {
  typedef typename Sh::Cfg Cfg;
  const size_t base = fused_lds_bytes<Sh>(2), word_row = (size_t)Cfg::THREADS * sizeof(typename Sh::E);
  const size_t waves = (size_t)(Cfg::THREADS + 63) / 64, by_waves = 4 * (size_t)dot_waves<typename Sh::E, Sh::LOGN, Sh::LPT, Sh::LAZY>() / waves;
  size_t wgs = GADGET2_CU_LDS / base;        // resident workgroups of the gadget kernel: what LDS holds, what the waves allow, one at least
  if (wgs > by_waves) wgs = by_waves;
  if (wgs < 1) wgs = 1;
  int x = Cfg::R;
  while (x > 0 && GADGET2_CU_LDS / (base + (size_t)x * word_row) < wgs) --x;
  return x;
}

}  // namespace tn
