// kernels.hip — gfx950 kernels of libtinyntt and their launchers.
//
//  polymul_fused_kernel : K6, the throughput path.  Persistent workgroups, one
//      polynomial pair at a time; coefficients live in VGPRs (2^LPT per thread), the
//      log2(n) radix-2 stages run as ceil(log2 n / LPT) register phases with LDS
//      transposes between them (padded, bank-conflict-free images addressed as
//      base + immediate offset); psi-twist and n^-1 folded into the twiddles
//      (fused_core.h); the same kernel on the x^n - 1 twiddle tables is the cyclic product.
//      HBM traffic per product = read a, read b, write c.
//  ntt_fused_kernel     : the standalone transforms (twist+forward, cg_ntt, cg_intt)
//      on the same machinery, natural order in and out.
//  cg_kernel            : K1-K5/K7, the reference's own constant-geometry dataflow (cg_ntt.py:49-64): cg_kernel_impl.h,
//      instantiated in slices by cg_part.hip; only the dispatcher launch_cg() lives here.
//  fill_lcg_kernel / checksum_kernel : the reference benchmark's input
//      generator and digest (benchmark_ntt_60bit.cpp:79-87,182-188), on device.
#include <hip/hip_runtime.h>
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
// This file is compiled in four slices that build in parallel (Makefile: kernels.o, kernels_prepared.o, kernels_hat.o,
// kernels_gadget.o), the way cg_part.hip is:
//   TN_KERNELS_PART 0  everything but the prepared-operand kernels
//   TN_KERNELS_PART 1  the prepared-operand kernels and their launchers
//   TN_KERNELS_PART 2  the transform-domain kernels (both operands prepared; unprepare) and their launchers
//   TN_KERNELS_PART 3  the gadget kernels (decomposition into digits; the dot product that decomposes a itself) and their launchers
// Undefined (`make resources`, tools/build_variant.sh): the whole file as one translation unit.
#ifndef TN_KERNELS_PART
#define TN_KERNELS_MAIN 1
#define TN_KERNELS_PREPARED 1
#define TN_KERNELS_HAT 1
#define TN_KERNELS_GADGET 1
#else
#define TN_KERNELS_MAIN (TN_KERNELS_PART == 0)
#define TN_KERNELS_PREPARED (TN_KERNELS_PART == 1)
#define TN_KERNELS_HAT (TN_KERNELS_PART == 2)
#define TN_KERNELS_GADGET (TN_KERNELS_PART == 3)
#endif
namespace tn {

// ============================================================================
// Fused kernel
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

// The kernel's Arith argument as it lies in the kernel-argument segment (first argument of both fused kernels), addressed
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

#if defined(TN_FUSED_STAMPS) && TN_KERNELS_MAIN
// DIAGNOSTIC BUILD ONLY (tools/gpu_fused_clock.py; MI355X_MICROARCH.md, DVFS give-back item 6): every workgroup of the product
// kernel stamps s_memtime (shader cycles) and s_memrealtime (100 MHz) once before and once after its row loop into an array
// of its own in the code object; nothing in the kernel reads it and no output depends on it.  The shipped library has no stamp.
__device__ unsigned long long tn_fused_stamps[4 * 4096];
#endif

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

// waves per SIMD the product kernel's register allocation leaves room for (16 coeff/thread shapes need > 128 VGPRs)
template <typename E, int LOGN, int LPT, bool LAZY>
constexpr int polymul_waves() {
  return LPT >= 4 ? 2 : (sizeof(E) == 8 && LOGN == 12 && LAZY) ? TN_POLYMUL60_WAVES : TN_FUSED_MIN_WAVES;
}

#if TN_KERNELS_MAIN
// BC (n = 4096 / 64-bit lazy only): both forward transforms stop one stage early, basecase() replaces the last stage, the
// pointwise product and the first inverse stage (fused_core.h); tab_fwd is then the plan's psi_bc / cyc_bc table, whose last
// level holds the base case's zeta records, and ar.fninv / fninv_w1 carry (n/2)^-1 (launch_plan.h: fused_product_setup).
template <typename E, int LOGN, int LPT, bool LAZY, bool CIN = false, bool BC = false>
__global__ void __launch_bounds__((1 << (LOGN - LPT)), (polymul_waves<E, LOGN, LPT, LAZY>()))
polymul_fused_kernel(const Arith<E> ar, const typename TwOf<E>::type* __restrict__ tab_fwd,
                     const typename TwOf<E>::type* __restrict__ tab_inv, const E* __restrict__ a, const E* __restrict__ b,
                     E* __restrict__ c, u32 batch, u32* sched, u32 chunk) {
  // The twiddle tables are separate __restrict__ kernel arguments (not fields of a struct) so the
  // compiler can prove the stores to c never alias them: wave-uniform twiddle loads then become
  // scalar loads (s_load_dwordx4) instead of vector loads that every wave would wait on.
  typedef FusedCfg<E, LOGN, LPT> Cfg;
  typedef Policy<E, LAZY, CIN> Pol;
  extern __shared__ __attribute__((aligned(16))) unsigned char tn_smem[];
  E* lds = reinterpret_cast<E*>(tn_smem);
  typedef typename TwOf<E>::type Tw;
  const u32 tau = threadIdx.x;
  // twiddles of the lane-dependent middle phases: staged once per (persistent) workgroup in LDS
  Tw* lds_fwd = reinterpret_cast<Tw*>(lds + Cfg::lds_elems());
  Tw* lds_inv = lds_fwd + Cfg::lds_tw_count();
  u32* lds_next = reinterpret_cast<u32*>(lds_inv + Cfg::lds_tw_count());      // row index this workgroup takes next
  for (u32 i = tau; i < (u32)Cfg::lds_tw_count(); i += Cfg::THREADS) {
    lds_fwd[i] = tab_fwd[Cfg::lds_tw_lo() + i];
    lds_inv[i] = tab_inv[Cfg::lds_tw_lo() + i];
  }
  __syncthreads();
  // Persistent workgroup.  Rows come in chunks of `chunk` consecutive rows: chunk blockIdx.x first, then whatever the
  // device-wide counter sched[0] hands out (atomicAdd): a workgroup on a slower CU / XCD simply takes fewer chunks, so
  // the launch ends when the work does, not when the slowest fixed share does.  (chunk > 1 for short rows keeps the
  // rate of atomics on that one address low.)  sched == nullptr: fixed stride.  The next row's first
  // operand is fetched from HBM into the registers that held b (dead after the pointwise
  // product) while the inverse transform of the current row runs; b itself is requested at the
  // top of the row and not needed until a's forward transform is done.
  E xa[Cfg::R], xb[Cfg::R];
#ifdef TN_FUSED_STAMPS
  const unsigned long long st_t0 = __builtin_amdgcn_s_memtime(), st_r0 = __builtin_amdgcn_s_memrealtime();
#endif
  u32 row = blockIdx.x * chunk;
  u32 taken = 1;                            // rows taken from the current chunk           (both workgroup-uniform: scalar registers)
  u32 chunk_id = blockIdx.x;                // fixed-stride mode: the chunk being processed
  if (row < batch) {
#pragma unroll
    for (int r = 0; r < Cfg::R; ++r) xb[r] = ld_operand<E, Cfg>(a, row, tau, r);
  }
  // The stores of row k are issued at the TOP of iteration k+1 (software-pipelined): vector-memory
  // operations retire in order and the compiler drains them all at the loop back-edge, so stores
  // issued at the bottom would expose their full latency there on every row.  Issued at the top,
  // the only operations in flight at the back-edge are the prefetch loads, which are needed anyway.
  // (first iteration: nothing to store yet -> the zero-initialised registers are written to this
  //  row's own slot, which the same thread overwrites with the real result one iteration later;
  //  keeping the store unconditional keeps the loop top branch-free so the ordering below holds)
  // last forward phase's thread-private twiddles, shared by a and b; those of the last stage are loaded once per workgroup
  constexpr int PRE_END = (TN_RESIDENT_TW && polymul_waves<E, LOGN, LPT, LAZY>() <= 4 && Cfg::stage_end(Cfg::PHASES - 1) - Cfg::stage_begin(Cfg::PHASES - 1) >= 2) ? Cfg::LOGN - 1 : Cfg::LOGN;
  Tw prf[Cfg::NPRE];
  tw_prefetch_stages<E, Cfg, PRE_END, Cfg::LOGN>(prf, tau, tab_fwd);
  u32 prev = row;
  bool have_c = false;
#pragma unroll
  for (int r = 0; r < Cfg::R; ++r) xa[r] = 0;
  while (row < batch) {
    // The workgroup-uniform twiddles of the first phase (13 records = 52 SGPRs) are reloaded by the scalar unit in every
    // row instead of being hoisted out of the loop: hoisted they do not fit the SGPR file and come back through
    // v_readlane (a vector-ALU slot each), while a scalar load that hits the scalar cache is free.
    const u32 zero = opaque_zero();
    const u32 tl = opaque_copy(tau);         // thread index for global addressing within this row (see opaque_copy)
    // one thread determines the next row now; everyone reads the answer after a's transform (barriers in between)
    const bool in_chunk = taken != chunk;                  // workgroup-uniform bookkeeping, kept on the scalar unit (counting up:
    taken = in_chunk ? taken + 1 : 1;                      // a down-counter's "subtract and test the borrow" is selected as a vector op)
    chunk_id = in_chunk ? chunk_id : chunk_id + gridDim.x;
    if (tau == 0) *lds_next = in_chunk ? row + 1 : (sched ? gridDim.x + atomicAdd(&sched[0], 1u) : chunk_id) * chunk;
    // consume this row's a (prefetched during the previous inverse) FIRST: at this point only those
    // loads are in flight, so the wait is exact; only then issue the stores of the previous row and b's loads
    TN_MARK("loop_top");
    E xn[Cfg::R];
#pragma unroll
    for (int r = 0; r < Cfg::R; ++r) xn[r] = xb[r];
    load_reduce<E, Cfg, Pol>(xn, ar);
    sched_fence();
#if TN_STORE_AT_TOP
    st_result<E, Cfg>(c, prev, tl, xa);
#endif
#pragma unroll
    for (int r = 0; r < Cfg::R; ++r) xb[r] = ld_operand<E, Cfg>(b, row, tl, r);
    sched_fence();
#pragma unroll
    for (int r = 0; r < Cfg::R; ++r) xa[r] = xn[r];
    constexpr bool KARG = TN_KARG_ARITH != 0;
    constexpr bool SHARE = TN_SHARE_LAST_TW && Cfg::PHASES >= 2;
    // SHARE2: the phase before the last is a full LDS-sourced phase: its 2^LPT - 1 twiddles are read into registers once
    constexpr int PM = Cfg::PHASES >= 3 ? Cfg::PHASES - 2 : 0;
    constexpr bool SHARE2 = SHARE && TN_SHARE_MID_TW && Cfg::PHASES >= 3 && Cfg::tw_src(PM) == Cfg::TW_LDS &&
                            Cfg::stage_end(PM) - Cfg::stage_begin(PM) == Cfg::LPT;
    const TwRefs<E> twf = {tab_fwd, lds_fwd, prf, nullptr, zero};
    // A^ stays in registers while b is transformed
    static_assert(!BC || SHARE2, "base case: built for the shared-twiddle schedule only");
    if constexpr (SHARE2) forward_range<E, Cfg, Pol, 0, PM, KARG, Cfg::LOGN, BC>(xa, tau, twf, ar, lds, false, tl);
    else if constexpr (SHARE) forward_range<E, Cfg, Pol, 0, Cfg::PHASES - 1, KARG>(xa, tau, twf, ar, lds, false, tl);
    else forward_all<E, Cfg, Pol>(xa, tau, tab_fwd, lds_fwd, ar, lds, zero);
    __syncthreads();
    const u32 next = wave_uniform(*lds_next);
    load_reduce<E, Cfg, Pol>(xb, ar);
    if constexpr (SHARE2) {
      forward_range<E, Cfg, Pol, 0, PM, KARG, Cfg::LOGN, BC>(xb, tau, twf, ar, lds, false, tl);
      Tw mid[Cfg::R];
      tw_fetch_mid<E, Cfg, PM>(mid, tau, lds_fwd);
      const TwRefs<E> twm = {tab_fwd, lds_fwd, prf, mid, zero};
      forward_range<E, Cfg, Pol, PM, PM + 1, KARG, Cfg::LOGN, BC>(xa, tau, twm, ar, lds, false, tl);
      forward_range<E, Cfg, Pol, PM, PM + 1, KARG, PRE_END, BC>(xb, tau, twm, ar, lds, true, tl);
      forward_range<E, Cfg, Pol, PM + 1, Cfg::PHASES, KARG, Cfg::LOGN, BC>(xb, tau, twf, ar, lds, false, tl);
      forward_range<E, Cfg, Pol, PM + 1, Cfg::PHASES, KARG, Cfg::LOGN, BC>(xa, tau, twf, ar, lds, false, tl);
    } else if constexpr (SHARE) {
      forward_range<E, Cfg, Pol, 0, Cfg::PHASES - 1, KARG, PRE_END>(xb, tau, twf, ar, lds, true, tl);
      forward_range<E, Cfg, Pol, Cfg::PHASES - 1, Cfg::PHASES, KARG>(xb, tau, twf, ar, lds, false, tl);
      forward_range<E, Cfg, Pol, Cfg::PHASES - 1, Cfg::PHASES, KARG>(xa, tau, twf, ar, lds, false, tl);
    } else {
      forward_all<E, Cfg, Pol>(xb, tau, tab_fwd, lds_fwd, ar, lds, zero);
    }
    // the inverse starts with the thread-private phase: request its twiddles before the product
    // (base case: the inverse's private phase has one stage less, so 3 of the 7 records; the zeta records came with prf)
    Tw pre[Cfg::NPRE];
    if constexpr (BC) {
      TN_MARK("basecase");
      basecase<Cfg, Pol>(xa, xb, prf + Cfg::pre_off(Cfg::LOGN - 1), ar);
      sched_fence();
      tw_prefetch_stages<E, Cfg, Cfg::stage_begin(Cfg::PHASES - 1), Cfg::LOGN - 1>(pre, tl, tab_inv);
    } else {
      tw_prefetch<E, Cfg>(pre, tl, tab_inv);
      TN_MARK("pointwise");
      pointwise<E, Cfg, Pol>(xa, xb, ar);
    }
    TN_MARK("after_pointwise");
    const TwRefs<E> twi = {tab_inv, lds_inv, pre, nullptr, zero};
    inverse_all<E, Cfg, Pol, KARG, BC>(xa, tau, twi, ar, lds, [&]() {
      // next row's first operand -> the registers that held b.  Unconditional (after the last row this row's a is read
      // again and dropped): a branch here costs a register copy of all R values on the path that skips it.
      const u32 nrow = next < batch ? next : row;
#pragma unroll
      for (int r = 0; r < Cfg::R; ++r) xb[r] = ld_operand<E, Cfg>(a, nrow, tl, r);
    });
#if TN_STORE_AT_TOP
    prev = row;
    have_c = true;
#else
    st_result<E, Cfg>(c, row, tau, xa);
#endif
    row = next;
  }
  if (have_c) st_result<E, Cfg>(c, prev, tau, xa);
#ifdef TN_FUSED_STAMPS
  if (tau == 0 && blockIdx.x < 4096) {
    tn_fused_stamps[4 * blockIdx.x + 0] = st_t0; tn_fused_stamps[4 * blockIdx.x + 1] = st_r0;
    tn_fused_stamps[4 * blockIdx.x + 2] = __builtin_amdgcn_s_memtime(); tn_fused_stamps[4 * blockIdx.x + 3] = __builtin_amdgcn_s_memrealtime();
  }
#endif
  // the last workgroup to run out of rows re-arms the counters for the next launch that uses this slot
  if (sched && tau == 0 && atomicAdd(&sched[1], 1u) == gridDim.x - 1) { sched[0] = 0; sched[1] = 0; }
}

// Standalone transforms on the register-tiled machinery, natural order in and out:
//   FNTT_TWIST_FWD   X[k] = sum_i x[i] psi^(i(2k+1))   = twist + cg_ntt = forward_ntt_bench (benchmark_ntt_60bit.cpp:161-165)
//   FNTT_CYCLIC_FWD  cg_ntt(x, omega=psi^2)            (cg_ntt.py:29-65)
//   FNTT_CYCLIC_INV  cg_intt(X, omega=psi^2)           (cg_ntt.py:68-75)
// All three are the same merged Cooley-Tukey / Gentleman-Sande butterflies; only the twiddle table differs: the
// negacyclic one (psi_brv: factorisation tree of x^n + 1) or the cyclic one (cyc_brv / cyc_inv_brv: tree of x^n - 1,
// see HostTables).  The merged transform produces / consumes bit-reversed order in the last phase's register layout;
// one extra LDS transpose through a natural-order image turns that into unit-stride HBM accesses.
template <typename E, int LOGN, int LPT, bool LAZY, int MODE>
__global__ void __launch_bounds__((1 << (LOGN - LPT)), (LPT >= 4 ? 2 : TN_FUSED_MIN_WAVES))
ntt_fused_kernel(const Arith<E> ar, const typename TwOf<E>::type* __restrict__ tab, const E* __restrict__ in, E* __restrict__ out, u32 batch,
                 u32* sched, u32 chunk) {
  typedef FusedCfg<E, LOGN, LPT> Cfg;
  typedef Policy<E, LAZY> Pol;
  typedef typename TwOf<E>::type Tw;
  extern __shared__ __attribute__((aligned(16))) unsigned char tn_smem[];
  E* lds = reinterpret_cast<E*>(tn_smem);
  const u32 tau = threadIdx.x;
  // LDS: [transpose image][natural-order image][staged twiddles][2 next-row slots].  The natural-order image has its own
  // region so that the only workgroup barrier a row adds to those of the cross-wave transpose is the one between writing
  // and reading that image; the next-row slot is double-buffered for the same reason.
  E* nat = lds + Cfg::lds_elems();
  Tw* lds_tab = reinterpret_cast<Tw*>(nat + Cfg::N);
  u32* lds_next = reinterpret_cast<u32*>(lds_tab + Cfg::lds_tw_count());
  for (u32 i = tau; i < (u32)Cfg::lds_tw_count(); i += Cfg::THREADS) lds_tab[i] = tab[Cfg::lds_tw_lo() + i];
  // rows: chunk blockIdx.x, then whatever the device-wide counter hands out (see polymul_fused_kernel); the prefetch needs
  // the next row at the top of an iteration, so the counter is asked one iteration ahead
  u32 left = chunk - 1, chunk_id = blockIdx.x;            // thread 0's copies are the ones used
  auto take_next = [&](u32 cur, u32 slot) {               // thread 0 only
    if (left) { --left; lds_next[slot] = cur + 1; }
    else {
      chunk_id = sched ? gridDim.x + atomicAdd(&sched[0], 1u) : chunk_id + gridDim.x;
      left = chunk - 1;
      lds_next[slot] = chunk_id * chunk;
    }
  };
  if (tau == 0) take_next(blockIdx.x * chunk, 1u);
  __syncthreads();
  u32 next = wave_uniform(lds_next[1]);
  constexpr int LAST = Cfg::PHASES - 1;
  // The next row's input is requested as soon as the current one has been consumed, so the HBM latency of row k+1
  // hides behind the arithmetic of row k (persistent workgroup, like the product kernel).
  E xn[Cfg::R];
  u32 row = blockIdx.x * chunk;
  if (row < batch) {
#pragma unroll
    for (int r = 0; r < Cfg::R; ++r) xn[r] = ld_operand<E, Cfg>(in, row, tau, r);
  }
  for (u32 it = 0; row < batch; ++it) {
    if (tau == 0) take_next(next, it & 1u);              // read back after this row's barrier(s)
    // (as in the product kernel: an opaque zero / thread index per row keep the uniform twiddle loads, the arithmetic constants
    //  and the operand addresses inside the row loop instead of in registers across it — at n = 8192 they spilled: 60-68 B/lane)
    constexpr bool PIN = LOGN >= TN_NTTF_PIN_LOGN;
    const u32 zero = PIN ? opaque_zero() : 0u;
    const u32 tl = PIN ? opaque_copy(tau) : tau;
    constexpr bool KARG = PIN && TN_KARG_ARITH != 0;
    E x[Cfg::R];
#pragma unroll
    for (int r = 0; r < Cfg::R; ++r) x[r] = xn[r];
    sched_fence();
    if (MODE != FNTT_CYCLIC_INV && next < batch) {
#pragma unroll
      for (int r = 0; r < Cfg::R; ++r) xn[r] = ld_operand<E, Cfg>(in, next, tl, r);
    }
    sched_fence();
    if (MODE == FNTT_CYCLIC_INV) {
#pragma unroll
      for (int r = 0; r < Cfg::R; ++r) x[r] = Pol::load(x[r], ar);
#pragma unroll
      for (int r = 0; r < Cfg::R; ++r) nat[Cfg::nat_addr(Cfg::jidx(0, tau, r))] = x[r];
      __syncthreads();
#pragma unroll
      for (int r = 0; r < Cfg::R; ++r) x[r] = nat[Cfg::nat_addr(bitrev(Cfg::jidx(LAST, tau, r), LOGN))];
      Tw pre[Cfg::NPRE];
      tw_prefetch<E, Cfg>(pre, tl, tab);
      const TwRefs<E> tw = {tab, lds_tab, pre, nullptr, zero};
      // the inverse starts with the thread-private phase (28 registers of twiddles): the prefetch goes after it,
      // as in the product kernel
      inverse_all<E, Cfg, Pol, KARG>(x, tau, tw, ar, lds, [&]() {
        if (next < batch) {
#pragma unroll
          for (int r = 0; r < Cfg::R; ++r) xn[r] = ld_operand<E, Cfg>(in, next, tl, r);
        }
      });
      st_result<E, Cfg>(out, row, tl, x);
    } else {
#pragma unroll
      for (int r = 0; r < Cfg::R / 2; ++r) x[r] = Pol::load(x[r], ar);                 // the other half is multiplied first
      if (!LAZY) {
#pragma unroll
        for (int r = Cfg::R / 2; r < Cfg::R; ++r) x[r] = Pol::load(x[r], ar);
      }
      {
        Tw pre[Cfg::NPRE];
        const TwRefs<E> tw = {tab, lds_tab, pre, nullptr, zero};
        forward_range<E, Cfg, Pol, 0, Cfg::PHASES, KARG>(x, tau, tw, ar, lds, true, tl);
      }
#pragma unroll
      for (int r = 0; r < Cfg::R; ++r)
        nat[Cfg::nat_addr(bitrev(Cfg::jidx(LAST, tau, r), LOGN))] = LAZY ? Pol::canon(x[r], ar) : x[r];
      __syncthreads();
#pragma unroll
      for (int r = 0; r < Cfg::R; ++r) x[r] = nat[Cfg::nat_addr(Cfg::jidx(0, tau, r))];
      st_result<E, Cfg>(out, row, tl, x);
    }
    if (Cfg::THREADS <= 64) __syncthreads();             // single-wave workgroups have no barrier inside the transposes
    row = next;
    next = wave_uniform(lds_next[it & 1u]);
  }
  if (sched && tau == 0 && atomicAdd(&sched[1], 1u) == gridDim.x - 1) { sched[0] = 0; sched[1] = 0; }
}

template <typename E, int LOGN, int LPT, bool LAZY>
static hipError_t launch_nttf_t(const tn_plan* p, int mode, const void* in, void* out, size_t batch, hipStream_t s) {
  typedef FusedCfg<E, LOGN, LPT> Cfg;
  typedef typename TwOf<E>::type Tw;
  const size_t lds_bytes = (size_t)(Cfg::lds_elems() + Cfg::N) * sizeof(E) + (size_t)Cfg::lds_tw_count() * sizeof(Tw) + 16;   // + natural image, next-row slots
  const PlanView<E> pv = make_view<E>(p);
  auto kern = ntt_fused_kernel<E, LOGN, LPT, LAZY, FNTT_TWIST_FWD>;
  if (mode == FNTT_CYCLIC_FWD) kern = ntt_fused_kernel<E, LOGN, LPT, LAZY, FNTT_CYCLIC_FWD>;
  else if (mode != FNTT_TWIST_FWD) kern = ntt_fused_kernel<E, LOGN, LPT, LAZY, FNTT_CYCLIC_INV>;
  const FusedNttSetup<E> su = fused_ntt_setup(pv.ar, mode);
  return launch_persistent(p, s, (const void*)kern, Cfg::THREADS, lds_bytes, Cfg::N * sizeof(E), batch, FUSED_ROWS, [&](u32 grid, u32* sched, u32 chunk) {
    const Tw* tab = fused_table(pv, su.tab);
    const E* in_ = (const E*)in; E* out_ = (E*)out; u32 b32 = (u32)batch;
    Arith<E> ar = su.ar;
    void* args[] = {&ar, &tab, &in_, &out_, &b32, &sched, &chunk};
    return hipLaunchKernel((const void*)kern, dim3(grid), dim3(Cfg::THREADS), args, lds_bytes, s);
  });
}

template <typename E, bool LAZY>
static hipError_t launch_nttf_e(const tn_plan* p, int mode, const void* in, void* out, size_t batch, hipStream_t s) {
#ifdef TN_ONLY_MAIN
  return hipErrorInvalidValue;
#else
  switch (p->logn) {
    case 8: return launch_nttf_t<E, 8, fused_lpt(8), LAZY>(p, mode, in, out, batch, s);
    case 9: return launch_nttf_t<E, 9, fused_lpt(9), LAZY>(p, mode, in, out, batch, s);
    case 10: return launch_nttf_t<E, 10, fused_lpt(10), LAZY>(p, mode, in, out, batch, s);
    case 11: return launch_nttf_t<E, 11, fused_lpt(11), LAZY>(p, mode, in, out, batch, s);
    case 12: return launch_nttf_t<E, 12, fused_lpt(12), LAZY>(p, mode, in, out, batch, s);
    case 13: return launch_nttf_t<E, 13, fused_lpt(13), LAZY>(p, mode, in, out, batch, s);
    default: return hipErrorInvalidValue;
  }
#endif
}

hipError_t launch_ntt_fused(const tn_plan* p, int mode, const void* in, void* out, size_t batch, hipStream_t s) {
  if (batch == 0) return hipSuccess;
  if (p->elem_bytes == 8)
    return p->lazy ? launch_nttf_e<u64, true>(p, mode, in, out, batch, s) : launch_nttf_e<u64, false>(p, mode, in, out, batch, s);
  return p->lazy ? launch_nttf_e<u32, true>(p, mode, in, out, batch, s) : launch_nttf_e<u32, false>(p, mode, in, out, batch, s);
}

bool fused_supported(u32 logn, int) { return fused_lpt((int)logn) != 0; }

template <typename E, int LOGN, int LPT, bool LAZY>
static hipError_t launch_fused_t(const tn_plan* p, const void* a, const void* b, void* c, size_t batch, hipStream_t s, bool cyclic) {
  typedef FusedCfg<E, LOGN, LPT> Cfg;
  const size_t lds_bytes = (size_t)Cfg::lds_elems() * sizeof(E) +
                           (size_t)2 * Cfg::lds_tw_count() * sizeof(typename TwOf<E>::type) + 16;      // + the next-row slot
  // promised-canonical inputs (TN_PLAN_CANONICAL_INPUTS): the n = 4096 / 64-bit lazy kernel has a second instantiation whose bound
  // schedule starts from q (no load folds); every other shape ignores the promise
  // Built only with -DTN_FUSED_CIN=1 (developer A/B, tools/gpu_ledger.py): measured 2.7 % SLOWER than the any-word kernel on the same
  // box (same 1,963 vector instructions per wave and row, 36 instead of 8 bytes of scratch: profiles/r3_headline_ledger.txt), so the
  // shipped library accepts the promise and runs the any-word kernel.
  constexpr bool HAS_CIN = TN_FUSED_CIN && sizeof(E) == 8 && LOGN == 12 && LAZY;
  // base case: for plans whose (k, c) passes h_bc_sched_ok(), unless the promised-canonical-inputs kernel is built and applies
  constexpr bool HAS_BC = fused_has_bc<E, LOGN, LPT, LAZY>();
  const bool use_cin = HAS_CIN && p->canonical_inputs && !cyclic;
  const bool use_bc = HAS_BC && p->bc_ok && !use_cin;
  auto kern = polymul_fused_kernel<E, LOGN, LPT, LAZY>;
  if constexpr (HAS_CIN) { if (use_cin) kern = polymul_fused_kernel<E, LOGN, LPT, LAZY, true>; }
  if constexpr (HAS_BC) { if (use_bc) kern = polymul_fused_kernel<E, LOGN, LPT, LAZY, false, true>; }
  const PlanView<E> pv = make_view<E>(p);
  const FusedProductSetup<E> su = fused_product_setup(pv.ar, use_bc, cyclic);
  return launch_persistent(p, s, reinterpret_cast<const void*>(kern), Cfg::THREADS, lds_bytes, Cfg::N * sizeof(E), batch, FUSED_ROWS,
                           [&](u32 grid, u32* sched, u32 chunk) {
    hipLaunchKernelGGL(kern, dim3(grid), dim3(Cfg::THREADS), lds_bytes, s, su.ar, fused_table(pv, su.fwd), fused_table(pv, su.inv),
                       (const E*)a, (const E*)b, (E*)c, (u32)batch, sched, chunk);
    return hipGetLastError();
  });
}

template <typename E, bool LAZY>
static hipError_t launch_fused_e(const tn_plan* p, const void* a, const void* b, void* c, size_t batch, hipStream_t s, bool cyclic) {
#ifdef TN_ONLY_MAIN      // developer builds (tools/build_variant.sh -DTN_ONLY_MAIN): only the n = 4096 / 64-bit lazy product kernel
  if constexpr (!(sizeof(E) == 8 && LAZY)) return hipErrorInvalidValue;
  else return p->logn == 12 ? launch_fused_t<E, 12, fused_lpt(12), LAZY>(p, a, b, c, batch, s, cyclic) : hipErrorInvalidValue;
#else
  switch (p->logn) {
    case 8: return launch_fused_t<E, 8, fused_lpt(8), LAZY>(p, a, b, c, batch, s, cyclic);
    case 9: return launch_fused_t<E, 9, fused_lpt(9), LAZY>(p, a, b, c, batch, s, cyclic);
    case 10: return launch_fused_t<E, 10, fused_lpt(10), LAZY>(p, a, b, c, batch, s, cyclic);
    case 11: return launch_fused_t<E, 11, fused_lpt(11), LAZY>(p, a, b, c, batch, s, cyclic);
    case 12: return launch_fused_t<E, 12, fused_lpt(12), LAZY>(p, a, b, c, batch, s, cyclic);
    case 13: return launch_fused_t<E, 13, fused_lpt(13), LAZY>(p, a, b, c, batch, s, cyclic);
    default: return hipErrorInvalidValue;
  }
#endif
}

hipError_t launch_polymul_fused(const tn_plan* p, const void* a, const void* b, void* c, size_t batch, hipStream_t s, bool cyclic) {
  if (batch == 0) return hipSuccess;
  if (p->elem_bytes == 8)
    return p->lazy ? launch_fused_e<u64, true>(p, a, b, c, batch, s, cyclic) : launch_fused_e<u64, false>(p, a, b, c, batch, s, cyclic);
  return p->lazy ? launch_fused_e<u32, true>(p, a, b, c, batch, s, cyclic) : launch_fused_e<u32, false>(p, a, b, c, batch, s, cyclic);
}

const char* fused_kernel_name(const tn_plan* p) {
  (void)p;
  return "polymul_fused_kernel";
}

// ============================================================================
// Constant-geometry kernels: dispatch to the slices of cg_part.hip (cg_kernel_impl.h)
// ============================================================================
#define TN_CG_PART_DECL(k) hipError_t launch_cg_part##k(const tn_plan*, int, int, int, bool, const void*, const void*, void*, void*, size_t, hipStream_t)
TN_CG_PART_DECL(0); TN_CG_PART_DECL(1); TN_CG_PART_DECL(2); TN_CG_PART_DECL(3); TN_CG_PART_DECL(4); TN_CG_PART_DECL(5); TN_CG_PART_DECL(6);
#undef TN_CG_PART_DECL

// group: butterflies per lane-step (1, 2, 4, 8); layout: CgLayout.  The LDS layouts differ only where the sweep of BASELINE
// config 5 is defined (lazy 64-bit plans at n = 4096); every other plan runs the linear image whatever the variant says.
hipError_t launch_cg(const tn_plan* p, int mode, int group, int layout, const void* a, const void* b, void* out, void* trace,
                     size_t batch, hipStream_t s) {
  if (batch == 0) return hipSuccess;
#ifdef TN_ONLY_MAIN
  return hipErrorInvalidValue;
#else
  if (group != 1 && group != 2 && group != 4 && group != 8) return hipErrorInvalidValue;
  while ((2u * (u32)group) > p->n) group /= 2;                      // tiny n: a lane-step cannot hold more than the polynomial
  const bool big = p->n / (2u * (u32)group) > (group == 1 ? 2048u : 1024u);   // n = 8192 at GROUP 1, 2 (CgShape)
  if (p->elem_bytes == 4) return launch_cg_part0(p, mode, group, layout, big, a, b, out, trace, batch, s);
  if (!(p->lazy)) return launch_cg_part1(p, mode, group, layout, big, a, b, out, trace, batch, s);
  // lazy 64-bit plan: every table holds split constants.  Per-stage traces need canonical values at every stage.
  if (trace || !p->cg_lazy) return launch_cg_part2(p, mode, group, layout, big, a, b, out, trace, batch, s);
  if (p->logn != 12 || !p->cg_sched) return launch_cg_part3(p, mode, group, layout, big, a, b, out, trace, batch, s);
  if (group <= 2) return launch_cg_part4(p, mode, group, layout, big, a, b, out, trace, batch, s);
  if (group == 4) return launch_cg_part5(p, mode, group, layout, big, a, b, out, trace, batch, s);
  return launch_cg_part6(p, mode, group, layout, big, a, b, out, trace, batch, s);
#endif
}

const char* cg_kernel_name(const tn_plan*, int, int) { return "cg_kernel"; }

// ============================================================================
// Elementwise product and the O(n^2) direct product (on-device checker)
// ============================================================================
// pointwise_mul (benchmark_ntt_60bit.cpp:142-146; cg_ntt.py:88): c[i] = a[i] * b[i] mod q
template <typename E>
__global__ void pointwise_kernel(PlanView<E> pv, const E* __restrict__ a, const E* __restrict__ b, E* __restrict__ c, size_t total) {
  const Arith<E> ar = pv.ar;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x)
    c[i] = mulmod_barrett(mul_tw(a[i], ar.one, ar.q), mul_tw(b[i], ar.one, ar.q), ar.q, ar.mu, ar.k);
}

// negacyclic_mul_reference (benchmark_ntt_60bit.cpp:167-180; test_cg_ntt.py:11-21; the
// benchmark_simple family): c[k] = sum_{i<=k} a[i] b[k-i] - sum_{i>k} a[i] b[n+k-i]  (mod q).
// One workgroup per (row, 256 output coefficients); operands staged in LDS.
template <typename E>
__global__ void __launch_bounds__(256)
schoolbook_kernel(PlanView<E> pv, const E* __restrict__ a, const E* __restrict__ b, E* __restrict__ c, u32 batch) {
  extern __shared__ __attribute__((aligned(16))) unsigned char tn_smem[];
  const u32 n = pv.n;
  const Arith<E> ar = pv.ar;
  E* sa = reinterpret_cast<E*>(tn_smem);
  E* sb = sa + n;
  const u32 chunks = (n + 255) / 256;
  for (u32 w = blockIdx.x; w < batch * chunks; w += gridDim.x) {
    const u32 row = w / chunks, k = (w % chunks) * 256 + threadIdx.x;
    const size_t off = (size_t)row * n;
    __syncthreads();
    for (u32 i = threadIdx.x; i < n; i += 256) {
      sa[i] = mul_tw(a[off + i], ar.one, ar.q);
      sb[i] = mul_tw(b[off + i], ar.one, ar.q);
    }
    __syncthreads();
    if (k < n) {
      E acc = 0;
      for (u32 i = 0; i < n; ++i) {
        const E t = mulmod_barrett(sa[i], sb[(k - i) & (n - 1)], ar.q, ar.mu, ar.k);
        if (i <= k) acc = csub((E)(acc + t), ar.q);
        else acc = acc >= t ? (E)(acc - t) : (E)(acc + (ar.q - t));
      }
      c[off + k] = acc;
    }
  }
}

template <typename E>
static hipError_t launch_aux_e(const tn_plan* p, int what, const void* a, const void* b, void* c, size_t batch, hipStream_t s) {
  if (what == 0) {
    const size_t total = batch * p->n;
    const u32 blocks = (u32)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
    hipLaunchKernelGGL(pointwise_kernel<E>, dim3(blocks), dim3(256), 0, s, make_view<E>(p), (const E*)a, (const E*)b, (E*)c, total);
  } else {
    const size_t lds_bytes = (size_t)2 * p->n * sizeof(E);
    auto kern = schoolbook_kernel<E>;
    if (lds_bytes > 48 * 1024) {
      hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
      if (e != hipSuccess) return e;
    }
    const size_t work = batch * ((p->n + 255) / 256);
    const u32 blocks = (u32)(work < 65536 ? work : 65536);
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), lds_bytes, s, make_view<E>(p), (const E*)a, (const E*)b, (E*)c, (u32)batch);
  }
  return hipGetLastError();
}

hipError_t launch_pointwise(const tn_plan* p, const void* a, const void* b, void* c, size_t batch, hipStream_t s) {
  if (batch == 0) return hipSuccess;
  return p->elem_bytes == 8 ? launch_aux_e<u64>(p, 0, a, b, c, batch, s) : launch_aux_e<u32>(p, 0, a, b, c, batch, s);
}
hipError_t launch_schoolbook(const tn_plan* p, const void* a, const void* b, void* c, size_t batch, hipStream_t s) {
  if (batch == 0) return hipSuccess;
  return p->elem_bytes == 8 ? launch_aux_e<u64>(p, 1, a, b, c, batch, s) : launch_aux_e<u32>(p, 1, a, b, c, batch, s);
}

// ============================================================================
// Synthetic inputs + digest (reference benchmark conventions)
// ============================================================================
static constexpr u64 LCG_A = 6364136223846793005ULL, LCG_C = 1442695040888963407ULL;

template <typename E>
__global__ void fill_lcg_kernel(E* __restrict__ dst, u32 n, u64 q, int narrow, u64 seed0, u64 stride, u32 batch) {
  const u32 CH = n < 16 ? n : 16;
  const u32 chunks = n / CH;
  const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= (size_t)batch * chunks) return;
  const u32 row = (u32)(gid / chunks), i0 = (u32)(gid % chunks) * CH;
  // x_i0 = f^i0(seed), f(x) = A x + C mod 2^64: square-and-multiply on affine maps
  u64 ra = 1, rc = 0, ba = LCG_A, bc = LCG_C;
  for (u32 e = i0; e; e >>= 1) {
    if (e & 1) { rc = ba * rc + bc; ra = ba * ra; }
    bc = ba * bc + bc; ba = ba * ba;
  }
  u64 x = ra * (seed0 + (u64)row * stride) + rc;
  for (u32 i = 0; i < CH; ++i) {
    x = LCG_A * x + LCG_C;                                         // benchmark_ntt_60bit.cpp:83
    dst[(size_t)row * n + i0 + i] = (E)(narrow ? (x >> 17) % q : x % q);   // :84 / benchmark_ntt.cpp:87
  }
}

template <typename E>
__global__ void checksum_kernel(const E* __restrict__ src, u64* __restrict__ out, u32 n, int narrow, u32 batch) {
  const u32 row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= batch) return;
  const u64 M = 0xffffffffffffffc5ULL;
  u64 acc = 0;
  for (u32 i = 0; i < n; ++i) {
    const u64 v = src[(size_t)row * n + i];
    if (narrow) {
      acc = (acc * 1315423911ULL + v) % M;                          // benchmark_ntt.cpp:228-233 (wraps mod 2^64 first)
    } else {
      // (acc*K + v) mod M with a 128-bit intermediate (benchmark_ntt_60bit.cpp:182-188); M = 2^64 - 59
      u64 lo = acc * 1315423911ULL, hi = mulhi64(acc, 1315423911ULL);
      const u64 lo2 = lo + v;
      hi += (lo2 < lo);
      u64 r = lo2 + hi * 59;                                        // 2^64 == 59 (mod M); hi < 2^31
      if (r < lo2) r += 59;
      acc = r >= M ? r - M : r;
    }
  }
  out[row] = acc;
}

hipError_t launch_fill_lcg(const tn_plan* p, void* dst, size_t batch, u64 seed0, u64 stride, hipStream_t s) {
  if (batch == 0) return hipSuccess;
  const u32 CH = p->n < 16 ? p->n : 16;
  const size_t total = batch * (p->n / CH);
  const u32 blocks = (u32)((total + 255) / 256);
  const int narrow = p->q < ((u64)1 << 32);
  if (p->elem_bytes == 8)
    hipLaunchKernelGGL(fill_lcg_kernel<u64>, dim3(blocks), dim3(256), 0, s, (u64*)dst, p->n, p->q, narrow, seed0, stride, (u32)batch);
  else
    hipLaunchKernelGGL(fill_lcg_kernel<u32>, dim3(blocks), dim3(256), 0, s, (u32*)dst, p->n, p->q, narrow, seed0, stride, (u32)batch);
  return hipGetLastError();
}

hipError_t launch_checksum(const tn_plan* p, const void* src, u64* out, size_t batch, hipStream_t s) {
  if (batch == 0) return hipSuccess;
  const u32 blocks = (u32)((batch + 63) / 64);
  const int narrow = p->q < ((u64)1 << 32);
  if (p->elem_bytes == 8)
    hipLaunchKernelGGL(checksum_kernel<u64>, dim3(blocks), dim3(64), 0, s, (const u64*)src, out, p->n, narrow, (u32)batch);
  else
    hipLaunchKernelGGL(checksum_kernel<u32>, dim3(blocks), dim3(64), 0, s, (const u32*)src, out, p->n, narrow, (u32)batch);
  return hipGetLastError();
}

#endif  // TN_KERNELS_MAIN

#if TN_KERNELS_PREPARED || TN_KERNELS_HAT || TN_KERNELS_GADGET
// ============================================================================
// Prepared operand: the product with b transformed ahead of time
// ============================================================================
// A prepared row holds what polymul_fused_kernel of the same plan has in xb just before pointwise() / basecase(): b's
// negacyclic transform (stopped one stage early where the plan runs the base case), as canonical residues, word
// FusedCfg::prep_idx(tau, r) = register r of thread tau of the last phase.  Canonical words are within every bound the
// product's schedules assume for xb (pointwise(): any value below 14 q; basecase(): any word; 32-bit lanes fold), so the
// product below runs on the schedules of polymul_fused_kernel unchanged.
template <typename E, typename Cfg, bool NT>
__device__ __forceinline__ E ld_prepared(const E* __restrict__ p, u32 row, u32 tau, int r) {
  if constexpr (NT && TN_NT_STREAM) {      // a row streamed once: addressed like an operand row (ld_operand)
    const TN_GLOBAL_AS E* rp = uniform_ptr(p + ((size_t)row << Cfg::LOGN) + Cfg::prep_idx(0, r));
    return __builtin_nontemporal_load(rp + Cfg::prep_idx(tau, 0));
  } else {
    return p[((size_t)row << Cfg::LOGN) + Cfg::prep_idx(tau, r)];
  }
}
#endif  // TN_KERNELS_PREPARED || TN_KERNELS_HAT || TN_KERNELS_GADGET

#if TN_KERNELS_PREPARED
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
  u32 left = chunk - 1, chunk_id = blockIdx.x;            // thread 0's copies are the ones used
  auto take_next = [&](u32 cur, u32 slot) {               // thread 0 only
    if (left) { --left; lds_next[slot] = cur + 1; }
    else {
      chunk_id = sched ? gridDim.x + atomicAdd(&sched[0], 1u) : chunk_id + gridDim.x;
      left = chunk - 1;
      lds_next[slot] = chunk_id * chunk;
    }
  };
  if (tau == 0) take_next(blockIdx.x * chunk, 1u);
  __syncthreads();
  u32 next = wave_uniform(lds_next[1]);
  E xn[Cfg::R];
  u32 row = blockIdx.x * chunk;
  if (row < batch) {
#pragma unroll
    for (int r = 0; r < Cfg::R; ++r) xn[r] = ld_operand<E, Cfg>(b, row, tau, r);
  }
  for (u32 it = 0; row < batch; ++it) {
    if (tau == 0) take_next(next, it & 1u);              // read back after this row's barriers
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
  if (sched && tau == 0 && atomicAdd(&sched[1], 1u) == gridDim.x - 1) { sched[0] = 0; sched[1] = 0; }
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
  E* lds = reinterpret_cast<E*>(tn_smem);
  const u32 tau = threadIdx.x;
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
  // the last workgroup to run out of rows re-arms the counters for the next launch that uses this slot
  if (sched && tau == 0 && atomicAdd(&sched[1], 1u) == gridDim.x - 1) { sched[0] = 0; sched[1] = 0; }
}

// what: nullptr -> prepare (in = b, out = bhat); otherwise the product (in = a, what = bhat, out = c)
template <typename E, int LOGN, int LPT, bool LAZY>
static hipError_t launch_prepared_t(const tn_plan* p, const void* in, const void* bhat, bool shared, void* out, size_t batch, hipStream_t s) {
  typedef FusedCfg<E, LOGN, LPT> Cfg;
  typedef typename TwOf<E>::type Tw;
  // the base case exactly where the plan's product kernel runs it (launch_fused_t)
  constexpr bool HAS_BC = fused_has_bc<E, LOGN, LPT, LAZY>();
  const bool use_bc = HAS_BC && p->bc_ok;
  const PlanView<E> pv = make_view<E>(p);
  const FusedProductSetup<E> su = fused_product_setup(pv.ar, use_bc, false);
  const u32 b32 = (u32)batch;
  if (!bhat) {
    const size_t lds_bytes = (size_t)Cfg::lds_elems() * sizeof(E) + (size_t)Cfg::lds_tw_count() * sizeof(Tw) + 16;       // + next-row slots
    auto kern = prepare_fused_kernel<E, LOGN, LPT, LAZY, false>;
    if constexpr (HAS_BC) { if (use_bc) kern = prepare_fused_kernel<E, LOGN, LPT, LAZY, true>; }
    return launch_persistent(p, s, reinterpret_cast<const void*>(kern), Cfg::THREADS, lds_bytes, Cfg::N * sizeof(E), batch, FUSED_ROWS,
                             [&](u32 grid, u32* sched, u32 chunk) {
      hipLaunchKernelGGL(kern, dim3(grid), dim3(Cfg::THREADS), lds_bytes, s, su.ar, fused_table(pv, su.fwd), (const E*)in, (E*)out, b32, sched, chunk);
      return hipGetLastError();
    });
  }
  const size_t lds_bytes = (size_t)Cfg::lds_elems() * sizeof(E) + (size_t)2 * Cfg::lds_tw_count() * sizeof(Tw) + 16;     // + the next-row slot
  auto kern = shared ? polymul_prepared_kernel<E, LOGN, LPT, LAZY, false, true> : polymul_prepared_kernel<E, LOGN, LPT, LAZY, false, false>;
  if constexpr (HAS_BC) {
    if (use_bc) kern = shared ? polymul_prepared_kernel<E, LOGN, LPT, LAZY, true, true> : polymul_prepared_kernel<E, LOGN, LPT, LAZY, true, false>;
  }
  return launch_persistent(p, s, reinterpret_cast<const void*>(kern), Cfg::THREADS, lds_bytes, Cfg::N * sizeof(E), batch, FUSED_ROWS,
                           [&](u32 grid, u32* sched, u32 chunk) {
    hipLaunchKernelGGL(kern, dim3(grid), dim3(Cfg::THREADS), lds_bytes, s, su.ar, fused_table(pv, su.fwd), fused_table(pv, su.inv),
                       (const E*)in, (const E*)bhat, (E*)out, b32, sched, chunk);
    return hipGetLastError();
  });
}

template <typename E, bool LAZY>
static hipError_t launch_prepared_e(const tn_plan* p, const void* in, const void* bhat, bool shared, void* out, size_t batch, hipStream_t s) {
#ifdef TN_ONLY_MAIN
  return hipErrorInvalidValue;
#else
  switch (p->logn) {
    case 8: return launch_prepared_t<E, 8, fused_lpt(8), LAZY>(p, in, bhat, shared, out, batch, s);
    case 9: return launch_prepared_t<E, 9, fused_lpt(9), LAZY>(p, in, bhat, shared, out, batch, s);
    case 10: return launch_prepared_t<E, 10, fused_lpt(10), LAZY>(p, in, bhat, shared, out, batch, s);
    case 11: return launch_prepared_t<E, 11, fused_lpt(11), LAZY>(p, in, bhat, shared, out, batch, s);
    case 12: return launch_prepared_t<E, 12, fused_lpt(12), LAZY>(p, in, bhat, shared, out, batch, s);
    case 13: return launch_prepared_t<E, 13, fused_lpt(13), LAZY>(p, in, bhat, shared, out, batch, s);
    default: return hipErrorInvalidValue;
  }
#endif
}

static hipError_t launch_prepared_any(const tn_plan* p, const void* in, const void* bhat, bool shared, void* out, size_t batch, hipStream_t s) {
  if (batch == 0) return hipSuccess;
  if (p->elem_bytes == 8)
    return p->lazy ? launch_prepared_e<u64, true>(p, in, bhat, shared, out, batch, s) : launch_prepared_e<u64, false>(p, in, bhat, shared, out, batch, s);
  return p->lazy ? launch_prepared_e<u32, true>(p, in, bhat, shared, out, batch, s) : launch_prepared_e<u32, false>(p, in, bhat, shared, out, batch, s);
}

hipError_t launch_prepare(const tn_plan* p, const void* b, void* bhat, size_t rows, hipStream_t s) {
  return launch_prepared_any(p, b, nullptr, false, bhat, rows, s);
}
hipError_t launch_polymul_prepared(const tn_plan* p, const void* a, const void* bhat, bool shared, void* c, size_t batch, hipStream_t s) {
  return launch_prepared_any(p, a, bhat, shared, c, batch, s);
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
#endif  // TN_KERNELS_PREPARED
#if TN_KERNELS_PREPARED || TN_KERNELS_HAT || TN_KERNELS_GADGET
#ifndef TN_DOT_WAVES
#define TN_DOT_WAVES 4
#endif
template <typename E, int LOGN, int LPT, bool LAZY>
constexpr int dot_waves() {
  return polymul_waves<E, LOGN, LPT, LAZY>() > TN_DOT_WAVES ? TN_DOT_WAVES : polymul_waves<E, LOGN, LPT, LAZY>();
}
#endif  // TN_KERNELS_PREPARED || TN_KERNELS_HAT || TN_KERNELS_GADGET
#if TN_KERNELS_PREPARED
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
  E* lds = reinterpret_cast<E*>(tn_smem);
  const u32 tau = threadIdx.x;
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
    // the inverse starts with the thread-private phase: request its twiddles before the last product
    Tw pre[Cfg::NPRE];
    if constexpr (BC) {
      basecase<Cfg, Pol>(xa, xb, prf + Cfg::pre_off(Cfg::LOGN - 1), ar);
      sched_fence();
      tw_prefetch_stages<E, Cfg, Cfg::stage_begin(Cfg::PHASES - 1), Cfg::LOGN - 1>(pre, tl, tab_inv);
    } else {
      tw_prefetch<E, Cfg>(pre, tl, tab_inv);
      pointwise<E, Cfg, Pol>(xa, xb, ar);
    }
    dot_accumulate<E, Cfg, Pol>(acc, xa, ar);
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
  // the last workgroup to run out of rows re-arms the counters for the next launch that uses this slot
  if (sched && tau == 0 && atomicAdd(&sched[1], 1u) == gridDim.x - 1) { sched[0] = 0; sched[1] = 0; }
}

template <typename E, int LOGN, int LPT, bool LAZY>
static hipError_t launch_dot_t(const tn_plan* p, const void* a, const void* bhat, bool shared, void* c, size_t batch, size_t terms, hipStream_t s) {
  typedef FusedCfg<E, LOGN, LPT> Cfg;
  typedef typename TwOf<E>::type Tw;
  // the base case exactly where launch_prepared_t picks it
  constexpr bool HAS_BC = fused_has_bc<E, LOGN, LPT, LAZY>();
  const bool use_bc = HAS_BC && p->bc_ok;
  const PlanView<E> pv = make_view<E>(p);
  const FusedProductSetup<E> su = fused_product_setup(pv.ar, use_bc, false);
  const u32 b32 = (u32)batch, t32 = (u32)terms;
  const size_t lds_bytes = (size_t)Cfg::lds_elems() * sizeof(E) + (size_t)2 * Cfg::lds_tw_count() * sizeof(Tw) + 16;     // + the next-row slot
  auto kern = shared ? polydot_prepared_kernel<E, LOGN, LPT, LAZY, false, true> : polydot_prepared_kernel<E, LOGN, LPT, LAZY, false, false>;
  if constexpr (HAS_BC) {
    if (use_bc) kern = shared ? polydot_prepared_kernel<E, LOGN, LPT, LAZY, true, true> : polydot_prepared_kernel<E, LOGN, LPT, LAZY, true, false>;
  }
  // one output row is `terms` operand rows of work: rows are handed out in chunks of at least FUSED_ROWS.chunk_bytes of a
  return launch_persistent(p, s, reinterpret_cast<const void*>(kern), Cfg::THREADS, lds_bytes, dot_row_bytes(Cfg::N * sizeof(E), terms), batch, FUSED_ROWS,
                           [&](u32 grid, u32* sched, u32 chunk) {
    hipLaunchKernelGGL(kern, dim3(grid), dim3(Cfg::THREADS), lds_bytes, s, su.ar, fused_table(pv, su.fwd), fused_table(pv, su.inv),
                       (const E*)a, (const E*)bhat, (E*)c, b32, t32, sched, chunk);
    return hipGetLastError();
  });
}

template <typename E, bool LAZY>
static hipError_t launch_dot_e(const tn_plan* p, const void* a, const void* bhat, bool shared, void* c, size_t batch, size_t terms, hipStream_t s) {
#ifdef TN_ONLY_MAIN
  return hipErrorInvalidValue;
#else
  switch (p->logn) {
    case 8: return launch_dot_t<E, 8, fused_lpt(8), LAZY>(p, a, bhat, shared, c, batch, terms, s);
    case 9: return launch_dot_t<E, 9, fused_lpt(9), LAZY>(p, a, bhat, shared, c, batch, terms, s);
    case 10: return launch_dot_t<E, 10, fused_lpt(10), LAZY>(p, a, bhat, shared, c, batch, terms, s);
    case 11: return launch_dot_t<E, 11, fused_lpt(11), LAZY>(p, a, bhat, shared, c, batch, terms, s);
    case 12: return launch_dot_t<E, 12, fused_lpt(12), LAZY>(p, a, bhat, shared, c, batch, terms, s);
    case 13: return launch_dot_t<E, 13, fused_lpt(13), LAZY>(p, a, bhat, shared, c, batch, terms, s);
    default: return hipErrorInvalidValue;
  }
#endif
}

hipError_t launch_polydot_prepared(const tn_plan* p, const void* a, const void* bhat, bool shared, void* c, size_t batch, size_t terms, hipStream_t s) {
  if (batch == 0) return hipSuccess;
  if (terms == 1) return launch_polymul_prepared(p, a, bhat, shared, c, batch, s);       // the same kernel, bits and speed as a single product
  if (p->elem_bytes == 8)
    return p->lazy ? launch_dot_e<u64, true>(p, a, bhat, shared, c, batch, terms, s) : launch_dot_e<u64, false>(p, a, bhat, shared, c, batch, terms, s);
  return p->lazy ? launch_dot_e<u32, true>(p, a, bhat, shared, c, batch, terms, s) : launch_dot_e<u32, false>(p, a, bhat, shared, c, batch, terms, s);
}
#endif  // TN_KERNELS_PREPARED

#if TN_KERNELS_HAT
// ============================================================================
// Transform domain: prepared rows in, prepared rows or coefficients out
// ============================================================================
// Both operands of polydot_hat_kernel are prepared rows and unprepare_fused_kernel turns a prepared row back into
// coefficients: no forward transform runs in this slice.  Canonical words (what the library writes into a prepared row) are
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
  u32 left = chunk - 1, chunk_id = blockIdx.x;            // thread 0's copies are the ones used
  auto take_next = [&](u32 cur, u32 slot) {               // thread 0 only
    if (left) { --left; lds_next[slot] = cur + 1; }
    else {
      chunk_id = sched ? gridDim.x + atomicAdd(&sched[0], 1u) : chunk_id + gridDim.x;
      left = chunk - 1;
      lds_next[slot] = chunk_id * chunk;
    }
  };
  if (tau == 0) take_next(blockIdx.x * chunk, 1u);
  __syncthreads();
  u32 next = wave_uniform(lds_next[1]);
  E xn[Cfg::R];
  u32 row = blockIdx.x * chunk;
  if (row < batch) {
#pragma unroll
    for (int r = 0; r < Cfg::R; ++r) xn[r] = ld_prepared<E, Cfg, true>(xhat, row, tau, r);
  }
  for (u32 it = 0; row < batch; ++it) {
    if (tau == 0) take_next(next, it & 1u);              // read back after this row's barriers
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
  if (sched && tau == 0 && atomicAdd(&sched[1], 1u) == gridDim.x - 1) { sched[0] = 0; sched[1] = 0; }
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
  // the last workgroup to run out of rows re-arms the counters for the next launch that uses this slot
  if (sched && tau == 0 && atomicAdd(&sched[1], 1u) == gridDim.x - 1) { sched[0] = 0; sched[1] = 0; }
}

// bhat == nullptr: unprepare (in = xhat, out = x); otherwise the dot product of prepared rows (in = ahat)
template <typename E, int LOGN, int LPT, bool LAZY>
static hipError_t launch_hat_t(const tn_plan* p, const void* in, const void* bhat, bool shared, void* out, size_t batch, size_t terms, bool inv,
                               hipStream_t s) {
  typedef FusedCfg<E, LOGN, LPT> Cfg;
  typedef typename TwOf<E>::type Tw;
  // the base case exactly where launch_prepared_t picks it: the formats agree
  constexpr bool HAS_BC = fused_has_bc<E, LOGN, LPT, LAZY>();
  const bool use_bc = HAS_BC && p->bc_ok;
  const PlanView<E> pv = make_view<E>(p);
  const FusedProductSetup<E> su = fused_product_setup(pv.ar, use_bc, false);
  const u32 b32 = (u32)batch, t32 = (u32)terms;
  const size_t lds_inverse = (size_t)Cfg::lds_elems() * sizeof(E) + (size_t)Cfg::lds_tw_count() * sizeof(Tw) + 16;       // + next-row slots
  if (!bhat) {
    auto kern = unprepare_fused_kernel<E, LOGN, LPT, LAZY, false>;
    if constexpr (HAS_BC) { if (use_bc) kern = unprepare_fused_kernel<E, LOGN, LPT, LAZY, true>; }
    return launch_persistent(p, s, reinterpret_cast<const void*>(kern), Cfg::THREADS, lds_inverse, Cfg::N * sizeof(E), batch, FUSED_ROWS,
                             [&](u32 grid, u32* sched, u32 chunk) {
      hipLaunchKernelGGL(kern, dim3(grid), dim3(Cfg::THREADS), lds_inverse, s, su.ar, fused_table(pv, su.inv), (const E*)in, (E*)out, b32, sched, chunk);
      return hipGetLastError();
    });
  }
  const size_t lds_bytes = (inv ? lds_inverse : 16) + (use_bc ? (size_t)(Cfg::N / 2) * sizeof(Tw) : 0);        // + the base case's zeta records
  auto pick = [&](auto bc_) {
    constexpr bool BC = decltype(bc_)::value;
    if (inv) return shared ? polydot_hat_kernel<E, LOGN, LPT, LAZY, BC, true, true> : polydot_hat_kernel<E, LOGN, LPT, LAZY, BC, false, true>;
    return shared ? polydot_hat_kernel<E, LOGN, LPT, LAZY, BC, true, false> : polydot_hat_kernel<E, LOGN, LPT, LAZY, BC, false, false>;
  };
  auto kern = pick(std::false_type());
  if constexpr (HAS_BC) { if (use_bc) kern = pick(std::true_type()); }
  // one output row is `terms` rows of each operand: planned like the prepared dot product's rows
  return launch_persistent(p, s, reinterpret_cast<const void*>(kern), Cfg::THREADS, lds_bytes, dot_row_bytes(Cfg::N * sizeof(E), terms), batch, FUSED_ROWS,
                           [&](u32 grid, u32* sched, u32 chunk) {
    hipLaunchKernelGGL(kern, dim3(grid), dim3(Cfg::THREADS), lds_bytes, s, su.ar, fused_table(pv, su.fwd), fused_table(pv, su.inv),
                       (const E*)in, (const E*)bhat, (E*)out, b32, t32, sched, chunk);
    return hipGetLastError();
  });
}

template <typename E, bool LAZY>
static hipError_t launch_hat_e(const tn_plan* p, const void* in, const void* bhat, bool shared, void* out, size_t batch, size_t terms, bool inv,
                               hipStream_t s) {
#ifdef TN_ONLY_MAIN
  return hipErrorInvalidValue;
#else
  switch (p->logn) {
    case 8: return launch_hat_t<E, 8, fused_lpt(8), LAZY>(p, in, bhat, shared, out, batch, terms, inv, s);
    case 9: return launch_hat_t<E, 9, fused_lpt(9), LAZY>(p, in, bhat, shared, out, batch, terms, inv, s);
    case 10: return launch_hat_t<E, 10, fused_lpt(10), LAZY>(p, in, bhat, shared, out, batch, terms, inv, s);
    case 11: return launch_hat_t<E, 11, fused_lpt(11), LAZY>(p, in, bhat, shared, out, batch, terms, inv, s);
    case 12: return launch_hat_t<E, 12, fused_lpt(12), LAZY>(p, in, bhat, shared, out, batch, terms, inv, s);
    case 13: return launch_hat_t<E, 13, fused_lpt(13), LAZY>(p, in, bhat, shared, out, batch, terms, inv, s);
    default: return hipErrorInvalidValue;
  }
#endif
}

static hipError_t launch_hat_any(const tn_plan* p, const void* in, const void* bhat, bool shared, void* out, size_t batch, size_t terms, bool inv,
                                 hipStream_t s) {
  if (batch == 0) return hipSuccess;
  if (p->elem_bytes == 8)
    return p->lazy ? launch_hat_e<u64, true>(p, in, bhat, shared, out, batch, terms, inv, s) : launch_hat_e<u64, false>(p, in, bhat, shared, out, batch, terms, inv, s);
  return p->lazy ? launch_hat_e<u32, true>(p, in, bhat, shared, out, batch, terms, inv, s) : launch_hat_e<u32, false>(p, in, bhat, shared, out, batch, terms, inv, s);
}

hipError_t launch_unprepare(const tn_plan* p, const void* xhat, void* x, size_t rows, hipStream_t s) {
  return launch_hat_any(p, xhat, nullptr, false, x, rows, 1, true, s);
}
hipError_t launch_polydot_hat(const tn_plan* p, const void* ahat, const void* bhat, bool shared, void* out, size_t batch, size_t terms, bool out_prepared,
                              hipStream_t s) {
  return launch_hat_any(p, ahat, bhat, shared, out, batch, terms, !out_prepared, s);
}
#endif  // TN_KERNELS_HAT

#if TN_KERNELS_GADGET
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
  E* lds = reinterpret_cast<E*>(tn_smem);
  const u32 tau = threadIdx.x;
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
    // the inverse starts with the thread-private phase: request its twiddles before the last product
    Tw pre[Cfg::NPRE];
    if constexpr (BC) {
      basecase<Cfg, Pol>(xa, xb, prf + Cfg::pre_off(Cfg::LOGN - 1), ar);
      sched_fence();
      tw_prefetch_stages<E, Cfg, Cfg::stage_begin(Cfg::PHASES - 1), Cfg::LOGN - 1>(pre, tl, tab_inv);
    } else {
      tw_prefetch<E, Cfg>(pre, tl, tab_inv);
      pointwise<E, Cfg, Pol>(xa, xb, ar);
    }
    dot_accumulate<E, Cfg, Pol>(acc, xa, ar);
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
  // the last workgroup to run out of rows re-arms the counters for the next launch that uses this slot
  if (sched && tau == 0 && atomicAdd(&sched[1], 1u) == gridDim.x - 1) { sched[0] = 0; sched[1] = 0; }
}

template <typename E, int LOGN, int LPT, bool LAZY>
static hipError_t launch_gadget_t(const tn_plan* p, const void* a, const void* bhat, bool shared, void* c, size_t batch, size_t terms, u32 base_log,
                                  bool balanced, hipStream_t s) {
  typedef FusedCfg<E, LOGN, LPT> Cfg;
  typedef typename TwOf<E>::type Tw;
  // the base case exactly where launch_prepared_t picks it
  constexpr bool HAS_BC = fused_has_bc<E, LOGN, LPT, LAZY>();
  const bool use_bc = HAS_BC && p->bc_ok;
  const PlanView<E> pv = make_view<E>(p);
  const FusedProductSetup<E> su = fused_product_setup(pv.ar, use_bc, false);
  const u32 b32 = (u32)batch, t32 = (u32)terms, bal = balanced ? 1u : 0u;
  const size_t lds_bytes = (size_t)Cfg::lds_elems() * sizeof(E) + (size_t)2 * Cfg::lds_tw_count() * sizeof(Tw) + 16;     // + the next-row slot
  auto kern = shared ? polydot_gadget_kernel<E, LOGN, LPT, LAZY, false, true> : polydot_gadget_kernel<E, LOGN, LPT, LAZY, false, false>;
  if constexpr (HAS_BC) {
    if (use_bc) kern = shared ? polydot_gadget_kernel<E, LOGN, LPT, LAZY, true, true> : polydot_gadget_kernel<E, LOGN, LPT, LAZY, true, false>;
  }
  // Bytes per row: one output row is `terms` forward transforms and one inverse, the work of a row of the prepared dot product,
  // although only one row of a is read for it.  Rows are handed out to keep the rate of atomics on the one counter low against
  // the WORK between them, so the row is planned as the dot kernel's: dot_row_bytes, `terms` operand rows.
  return launch_persistent(p, s, reinterpret_cast<const void*>(kern), Cfg::THREADS, lds_bytes, dot_row_bytes(Cfg::N * sizeof(E), terms), batch, FUSED_ROWS,
                           [&](u32 grid, u32* sched, u32 chunk) {
    hipLaunchKernelGGL(kern, dim3(grid), dim3(Cfg::THREADS), lds_bytes, s, su.ar, fused_table(pv, su.fwd), fused_table(pv, su.inv),
                       (const E*)a, (const E*)bhat, (E*)c, b32, t32, base_log, bal, sched, chunk);
    return hipGetLastError();
  });
}

template <typename E, bool LAZY>
static hipError_t launch_gadget_e(const tn_plan* p, const void* a, const void* bhat, bool shared, void* c, size_t batch, size_t terms, u32 base_log,
                                  bool balanced, hipStream_t s) {
#ifdef TN_ONLY_MAIN
  return hipErrorInvalidValue;
#else
  switch (p->logn) {
    case 8: return launch_gadget_t<E, 8, fused_lpt(8), LAZY>(p, a, bhat, shared, c, batch, terms, base_log, balanced, s);
    case 9: return launch_gadget_t<E, 9, fused_lpt(9), LAZY>(p, a, bhat, shared, c, batch, terms, base_log, balanced, s);
    case 10: return launch_gadget_t<E, 10, fused_lpt(10), LAZY>(p, a, bhat, shared, c, batch, terms, base_log, balanced, s);
    case 11: return launch_gadget_t<E, 11, fused_lpt(11), LAZY>(p, a, bhat, shared, c, batch, terms, base_log, balanced, s);
    case 12: return launch_gadget_t<E, 12, fused_lpt(12), LAZY>(p, a, bhat, shared, c, batch, terms, base_log, balanced, s);
    case 13: return launch_gadget_t<E, 13, fused_lpt(13), LAZY>(p, a, bhat, shared, c, batch, terms, base_log, balanced, s);
    default: return hipErrorInvalidValue;
  }
#endif
}

// terms == 1 runs the same kernel: one digit, then the prepared product
hipError_t launch_polydot_gadget(const tn_plan* p, const void* a, const void* bhat, bool shared, void* c, size_t batch, size_t terms, u32 base_log,
                                 bool balanced, hipStream_t s) {
  if (batch == 0) return hipSuccess;
  if (p->elem_bytes == 8)
    return p->lazy ? launch_gadget_e<u64, true>(p, a, bhat, shared, c, batch, terms, base_log, balanced, s)
                   : launch_gadget_e<u64, false>(p, a, bhat, shared, c, batch, terms, base_log, balanced, s);
  return p->lazy ? launch_gadget_e<u32, true>(p, a, bhat, shared, c, batch, terms, base_log, balanced, s)
                 : launch_gadget_e<u32, false>(p, a, bhat, shared, c, batch, terms, base_log, balanced, s);
}
#endif  // TN_KERNELS_GADGET
}  // namespace tn

#if defined(TN_FUSED_STAMPS) && TN_KERNELS_MAIN
extern "C" size_t tn_debug_fused_stamps(void* host, size_t max_bytes) {
  (void)hipDeviceSynchronize();
  const size_t nb = sizeof(tn::tn_fused_stamps) < max_bytes ? sizeof(tn::tn_fused_stamps) : max_bytes;
  if (hipMemcpyFromSymbol(host, HIP_SYMBOL(tn::tn_fused_stamps), nb, 0, hipMemcpyDeviceToHost) != hipSuccess) return 0;
  return nb;
}
#endif
