// launch_plan.h — what a launch of the persistent kernels decides on the host, as plain functions without the HIP runtime:
// which fused shape (with_fused_shape) and whether its base case runs (fused_use_bc), which tables and constants
// (fused_product_setup, fused_ntt_setup) and how rows are handed out (plan_rows).  The launchers (kernels*.hip, cg_kernel_impl.h through plan.h: launch_persistent) and the CPU stepping of
// tests/emu both take their decisions from here, so the CPU tests check what the launchers do.
#pragma once
#include <stddef.h>
#include "fused_core.h"

#ifndef TN_DYNAMIC_ROWS
#define TN_DYNAMIC_ROWS 1        // 1: persistent workgroups take their next row from a device counter (atomicAdd) instead of a fixed
                                 //    stride: workgroups do not all run at the same speed, and with a fixed share the slowest sets the time
#endif
#ifndef TN_SCHED_CHUNK_BYTES
#define TN_SCHED_CHUNK_BYTES 32768   // dynamic scheduler: bytes of one operand handed out per atomicAdd (>= one row).  The launch's tail is up
                                     // to one chunk long: 32 / 64 / 128 KiB measured 2.138 / 2.147 / 2.160 ms at n = 4096 / 64-bit
#endif
#ifndef TN_CG_DYNAMIC_ROWS
#define TN_CG_DYNAMIC_ROWS 1     // the same switch for the constant-geometry kernels (fixed stride below TN_CG_DYNAMIC_MIN chunks each)
#endif
#ifndef TN_CG_DYNAMIC_MIN
#define TN_CG_DYNAMIC_MIN 8
#endif
#ifndef TN_CG_CHUNK_BYTES
#define TN_CG_CHUNK_BYTES 32768  // bytes of one operand handed out per atomicAdd (as TN_SCHED_CHUNK_BYTES of the fused kernels)
#endif

namespace tn {

enum FusedNttMode { FNTT_TWIST_FWD = 0, FNTT_CYCLIC_FWD = 1, FNTT_CYCLIC_INV = 2 };

// The twiddle tables of the fused kernels (HostTables / PlanView fields of the same names).
enum FusedTable { FT_PSI_BRV, FT_PSI_INV_BRV, FT_CYC_BRV, FT_CYC_INV_BRV, FT_PSI_BC, FT_CYC_BC };

// The one shape with a base-case product kernel (fused_core.h basecase(); measured in profiles/r4_basecase_ab.txt): n = 4096,
// 64-bit lanes, lazy.  Every other shape keeps the last stage and the pointwise product.
constexpr int FUSED_BC_LOGN = 12;
template <typename E, int LOGN, int LPT, bool LAZY> constexpr bool fused_has_bc() {
  return sizeof(E) == 8 && LOGN == FUSED_BC_LOGN && LPT == 3 && LAZY;
}

// A fused shape as a type: what with_fused_shape hands to a launcher or to the CPU stepping.
template <typename E_, int LOGN_, bool LAZY_> struct FusedShape {
  typedef E_ E;
  static constexpr int LOGN = LOGN_, LPT = fused_lpt(LOGN_);
  static constexpr bool LAZY = LAZY_, HAS_BC = fused_has_bc<E_, LOGN_, LPT, LAZY_>();
  typedef FusedCfg<E_, LOGN_, LPT> Cfg;
};

// f(lane type, std::true_type / std::false_type for the lazy policy) of a plan's (elem_bytes, lazy): for what depends on the
// arithmetic only.
template <typename F>
inline auto with_lane_policy(int elem_bytes, bool lazy, F&& f) {
  if (elem_bytes == 8) return lazy ? f(u64(), std::true_type()) : f(u64(), std::false_type());
  return lazy ? f(u32(), std::true_type()) : f(u32(), std::false_type());
}

// f(FusedShape of (elem_bytes, lazy, logn)), or `none` where no fused kernel is built for that n.  The one place that names
// the shapes: the launchers come here through dispatch_fused_shape (fused_kernels.h), the CPU stepping through emu_with_shape
// (tests/emu/emu_stepper.h).
template <typename R, typename F>
inline R with_fused_shape(int elem_bytes, bool lazy, u32 logn, R none, F&& f) {
  return with_lane_policy(elem_bytes, lazy, [&](auto e_, auto lazy_) -> R {
    typedef decltype(e_) E;
    constexpr bool LAZY = decltype(lazy_)::value;
    switch (logn) {
      case 8: return f(FusedShape<E, 8, LAZY>());
      case 9: return f(FusedShape<E, 9, LAZY>());
      case 10: return f(FusedShape<E, 10, LAZY>());
      case 11: return f(FusedShape<E, 11, LAZY>());
      case 12: return f(FusedShape<E, 12, LAZY>());
      case 13: return f(FusedShape<E, 13, LAZY>());
      default: return none;
    }
  });
}

// The base case runs for plans whose (k, c) passes h_bc_sched_ok() (bc_ok) at the one shape that has it, in EVERY kernel of the
// product family (product, prepared operand, transform domain, gadget): a prepared row is the product kernel's xb, so the
// formats agree only if they all choose alike.  no_bc: the product launcher's promised-canonical-inputs kernel takes
// precedence (launch_fused_t).
template <typename Sh> constexpr bool fused_use_bc(bool bc_ok, bool no_bc = false) { return Sh::HAS_BC && bc_ok && !no_bc; }

// Product launch.  bc: this launch runs the base-case kernel (fused_use_bc).  Then the forward table is psi_bc / cyc_bc, whose
// last level holds the base case's zeta records, and the inverse runs log2(n) - 1 stages: (n/2)^-1 in place of n^-1.
// cyclic = product in Z_q[x]/(x^n - 1) (python_poly_mult, test_ntt_poly_mult.py:38-43): same kernel, twiddle tables of the
// x^n - 1 factorisation tree (HostTables::cyc_brv), whose inverse table has entry 1 equal to 1.
template <typename E> struct FusedProductSetup { bool bc; Arith<E> ar; FusedTable fwd, inv; };
template <typename E> inline FusedProductSetup<E> fused_product_setup(const Arith<E>& ar, bool bc, bool cyclic) {
  FusedProductSetup<E> s = {bc, ar, cyclic ? FT_CYC_BRV : FT_PSI_BRV, cyclic ? FT_CYC_INV_BRV : FT_PSI_INV_BRV};
  if (bc) { s.ar.fninv = ar.bninv; s.ar.fninv_w1 = ar.bninv_w1; s.fwd = cyclic ? FT_CYC_BC : FT_PSI_BC; }
  if (cyclic) s.ar.fninv_w1 = s.ar.fninv;
  return s;
}

// Standalone transform launch (ntt_fused_kernel): the table of the mode; cg_intt's has entry 1 equal to 1.
template <typename E> struct FusedNttSetup { Arith<E> ar; FusedTable tab; };
template <typename E> inline FusedNttSetup<E> fused_ntt_setup(const Arith<E>& ar, int mode) {
  FusedNttSetup<E> s = {ar, mode == FNTT_TWIST_FWD ? FT_PSI_BRV : mode == FNTT_CYCLIC_FWD ? FT_CYC_BRV : FT_CYC_INV_BRV};
  if (mode == FNTT_CYCLIC_INV) s.ar.fninv_w1 = s.ar.fninv;
  return s;
}

// Row hand-out of the persistent kernels.  Dynamic (one atomicAdd on a device counter per chunk of rows) when the launch is
// long enough for every resident workgroup to take at least min_chunks chunks of chunk_bytes worth of rows (1 row at
// n = 4096 / 64-bit, 8 at n = 1024 / 32-bit, 2 at n = 2048 / 60-bit): a chunk that large keeps the one counter address from
// becoming the bottleneck (one row per atomic at n = 256 ran 13x slower than a fixed stride; at n = 1024 / 24-bit, batch
// 16,384, 10x).  Otherwise a fixed stride of single rows.
// single_rows_without_slot: what a launch does that planned dynamic rows but got no counter pair (none free, or the stream is
// being captured: plan.h sched_acquire).  It runs at a fixed stride either way.  The fused kernels keep their chunk (a
// workgroup then strides over chunks); the constant-geometry kernel hands out single rows.  The grid stays in both cases.
struct RowPolicy { size_t chunk_bytes, min_chunks; bool enabled, single_rows_without_slot; };
constexpr RowPolicy FUSED_ROWS = {TN_SCHED_CHUNK_BYTES, 4, TN_DYNAMIC_ROWS != 0, false};
constexpr RowPolicy CG_ROWS = {TN_CG_CHUNK_BYTES, TN_CG_DYNAMIC_MIN, TN_CG_DYNAMIC_ROWS != 0, true};

struct RowPlan { u32 chunk; bool dynamic; };
inline RowPlan plan_rows(size_t row_bytes, size_t batch, size_t resident, const RowPolicy& pol) {
  // rounded up: a chunk never holds less than chunk_bytes (the same as rounding down for every power-of-two row; a row of the
  // prepared dot product, dot_row_bytes, need not divide chunk_bytes)
  size_t want = (pol.chunk_bytes + row_bytes - 1) / row_bytes;
  if (want < 1) want = 1;
  if (pol.enabled && batch >= pol.min_chunks * resident * want) return {(u32)want, true};
  return {1u, false};
}
// Prepared dot product (polydot_prepared_kernel): one output row is `terms` operand rows of work, so that is the row size its
// rows are planned with: a chunk stays at or above chunk_bytes of operand per atomic however short a single row is.
inline size_t dot_row_bytes(size_t operand_row_bytes, size_t terms) { return operand_row_bytes * terms; }

// Blind rotation in one launch (polydot_blindrot_kernel, kernels_blindrot.hip): the LDS request of a workgroup is the CMux
// step's layout (the transpose image, xl * THREADS words of an input put away, two staged twiddle tables, the next-row slot:
// fused_lds_bytes of fused_kernels.h) plus the accumulator, two rows of n words.  A shape is supported when that request fits
// the 160 KiB a workgroup can have.  One rule for the launcher, the argument check (api_checks.h) and the CPU stepping.
constexpr size_t BLINDROT_WG_LDS = 160 * 1024;
constexpr size_t BLINDROT_WAVES = 4;                 // waves per SIMD the kernel is built for (dot_waves, fused_kernels.h)
template <typename Sh> constexpr size_t blindrot_lds_bytes(int xl) {
  typedef typename Sh::Cfg Cfg;
  return ((size_t)Cfg::lds_elems() + (size_t)xl * Cfg::THREADS + 2 * (size_t)Cfg::N) * sizeof(typename Sh::E) +
         2 * (size_t)Cfg::lds_tw_count() * sizeof(typename TwOf<typename Sh::E>::type) + 16;
}
// Words of an input polynomial per thread put away in LDS instead of registers: as many as leave the CU the resident
// workgroups it has with none put away (what LDS holds, what the waves allow, one at least), chosen from the resource report
// (DESIGN.md 3.2i).
template <typename Sh> constexpr int blindrot_lds_words() {
  typedef typename Sh::Cfg Cfg;
  const size_t base = blindrot_lds_bytes<Sh>(0), word_row = (size_t)Cfg::THREADS * sizeof(typename Sh::E);
  const size_t waves = (size_t)(Cfg::THREADS + 63) / 64, by_waves = 4 * BLINDROT_WAVES / waves;
  size_t wgs = BLINDROT_WG_LDS / base;
  if (wgs > by_waves) wgs = by_waves;
  if (wgs < 1) wgs = 1;
  int x = Cfg::R;
  while (x > 0 && BLINDROT_WG_LDS / (base + (size_t)x * word_row) < wgs) --x;
  // 64-bit words: half of them at least.  With fewer put away the n = 512 kernels use scratch (12 - 80 bytes per lane with 0
  // and 2 of 8; none with 4), and no instantiation may; the rule by itself gives 0 only there.
  if (sizeof(typename Sh::E) == 8 && x < Cfg::R / 2) x = Cfg::R / 2;
  return x;
}
template <typename Sh> constexpr bool blindrot_lds_fits() { return blindrot_lds_bytes<Sh>(blindrot_lds_words<Sh>()) <= BLINDROT_WG_LDS; }
// ... of a plan's (elem_bytes, lazy, logn); false where no fused kernel is built for that n.  Over the limit: n = 8192 with
// 64-bit words alone (tests/test_blindrot_emu.py walks the list).
inline bool blindrot_supported(int elem_bytes, bool lazy, u32 logn) {
  return with_fused_shape(elem_bytes, lazy, logn, false, [](auto sh) { return blindrot_lds_fits<decltype(sh)>(); });
}

}  // namespace tn
