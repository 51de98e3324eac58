// emu_stepper.h — TEST INFRASTRUCTURE: what every family of the CPU stepping uses.  The Stepper runs one workgroup of the fused
// kernels' per-thread code (tiny_ntt_amd/csrc/fused_core.h, modarith.h, plan_tables.h: the very headers the gfx950 kernels
// are compiled from), one emulated thread at a time with the LDS image between phases.  emu_with_shape picks the instantiation
// for a plan through the launchers' own dispatcher and base-case rule (launch_plan.h: with_fused_shape, fused_use_bc), so
// tests/emu names no shape.  gadget_ok and api_answer put the library's own argument checks (csrc/api_checks.h) behind the
// stepping entry points, which restate no bound of the library.  Included by every emu_*.cpp of this directory (kernels,
// prepared, dot, hat, gadget, gadget2, galois, extprod, cmux, blindrot), which tests/emu/Makefile links into one libemu.so.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <cstdio>
#include <vector>
#include "../../tiny_ntt_amd/csrc/plan_tables.h"
#include "../../tiny_ntt_amd/csrc/api_checks.h"

using namespace tn;

namespace {        // internal linkage: each object keeps (and inlines) its own instantiations, the library exports only its entry points

inline const std::vector<u64>& host_table(const HostTables& t, FusedTable w) {
  switch (w) {
    case FT_PSI_BRV: return t.psi_brv;
    case FT_PSI_INV_BRV: return t.psi_inv_brv;
    case FT_CYC_BRV: return t.cyc_brv;
    case FT_CYC_INV_BRV: return t.cyc_inv_brv;
    case FT_PSI_BC: return t.psi_bc;
    case FT_CYC_BC: return t.cyc_bc;
  }
  return t.psi_brv;
}

// One workgroup of the fused kernels: every thread runs phase p, then all of them exchange through the LDS image.
// BC: the base-case product's incomplete transform (fwd_phase / inv_phase).
template <typename E, int LOGN, int LPT, typename Pol, bool BC = false> struct Stepper {
  typedef FusedCfg<E, LOGN, LPT> Cfg;
  typedef typename TwOf<E>::type Tw;
  static constexpr u32 T = Cfg::THREADS;
  struct Regs { E x[Cfg::R]; };
  struct Pre { Tw t[Cfg::NPRE]; };
  // a table in the plan's record format and the slice of it the kernel stages in LDS
  struct Table {
    std::vector<Tw> glob, lds;
    Table(const HostTables& t, FusedTable w) : glob(h_fused_table<E>(host_table(t, w), t)), lds(glob.begin() + Cfg::lds_tw_lo(), glob.begin() + Cfg::lds_tw_hi()) {}
  };
  const Arith<E> ar;
  std::vector<E> lds = std::vector<E>(Cfg::lds_elems());
  std::vector<Pre> pre = std::vector<Pre>(T);        // the last phase's thread-private records of the transform stepped last

  template <int EX, int FROM, int TO> void exchange(std::vector<Regs>& x) {
    for (auto& v : lds) v = (E)0xDEADBEEFu;
    for (u32 tau = 0; tau < T; ++tau) ex_store<E, Cfg, EX, FROM>(x[tau].x, tau, lds.data());
    for (u32 tau = 0; tau < T; ++tau) ex_load<E, Cfg, EX, TO>(x[tau].x, tau, lds.data());
  }
  void forward(std::vector<Regs>& x, const Table& tab) {
    for (u32 tau = 0; tau < T; ++tau) tw_prefetch<E, Cfg>(pre[tau].t, tau, tab.glob.data());
    static_for<0, Cfg::PHASES>([&](auto p_) {
      constexpr int p = decltype(p_)::value;
      for (u32 tau = 0; tau < T; ++tau) {
        const TwRefs<E> tw = {tab.glob.data(), tab.lds.data(), pre[tau].t};
        fwd_phase<E, Cfg, Pol, p, BC>(x[tau].x, tau, tw, ar);
      }
      if constexpr (p + 1 < Cfg::PHASES) exchange<p, p, p + 1>(x);
    });
  }
  void inverse(std::vector<Regs>& x, const Table& tab) {
    for (u32 tau = 0; tau < T; ++tau) {
      if constexpr (BC) for (auto& r : pre[tau].t) r = Tw{~(u64)0, ~(u64)0};      // records the base case's inverse must not read
      tw_prefetch_stages<E, Cfg, Cfg::stage_begin(Cfg::PHASES - 1), BC ? LOGN - 1 : LOGN>(pre[tau].t, tau, tab.glob.data());
    }
    static_for<0, Cfg::PHASES>([&](auto i_) {
      constexpr int p = Cfg::PHASES - 1 - decltype(i_)::value;
      for (u32 tau = 0; tau < T; ++tau) {
        const TwRefs<E> tw = {tab.glob.data(), tab.lds.data(), pre[tau].t};
        inv_phase<E, Cfg, Pol, p, BC>(x[tau].x, tau, tw, ar);
      }
      if constexpr (p > 0) exchange<p - 1, p, p - 1>(x);
    });
  }
};

// One term of the gadget kernels (polydot_gadget_kernel, ..._gadget2_, ..._extprod_, ..._cmux_, ..._blindrot_kernel) for every
// thread of the workgroup: digit j is cut out of the thread's put-away words xw (gadget_digit, the carries of the thread's
// words in one mask that is handed on to the next term), ONE forward transform runs WITHOUT load_reduce, then one product per
// component against its prepared row bhat[boff[o] << LOGN ...]: every component but the last through dot_product_into, which
// leaves the digit row as it is for the next one; the last in place (the gadget kernel's product) and through dot_accumulate.
// Component o is summed into *acc[o].  How xw is put away and what happens to the sums is the family's own.
template <typename E, int LOGN, int LPT, typename Pol, bool BC>
void gadget_term_step(Stepper<E, LOGN, LPT, Pol, BC>& wg, const typename Stepper<E, LOGN, LPT, Pol, BC>::Table& fwd,
                      const std::vector<typename Stepper<E, LOGN, LPT, Pol, BC>::Regs>& xw, std::vector<u32>& carries, size_t j, u32 base_log,
                      bool balanced, const u64* bhat, size_t comps, const size_t* boff,
                      std::vector<typename Stepper<E, LOGN, LPT, Pol, BC>::Regs>* const* acc) {
  typedef Stepper<E, LOGN, LPT, Pol, BC> S;
  typedef typename S::Cfg Cfg;
  static_assert(Cfg::R <= 32, "one carry bit per word of the thread in a 32-bit mask");
  std::vector<typename S::Regs> xa(S::T), xb(S::T);
  const u32 shift = (u32)j * base_log;
  for (u32 tau = 0; tau < S::T; ++tau) {
    u32 next_carries = 0;
    for (int r = 0; r < Cfg::R; ++r) {
      u32 cy = (carries[tau] >> r) & 1u;
      xa[tau].x[r] = gadget_digit<E>(xw[tau].x[r], shift, base_log, balanced, cy, wg.ar.q);
      next_carries |= cy << r;
    }
    carries[tau] = next_carries;
  }
  wg.forward(xa, fwd);                                       // once per term, for every component
  for (size_t o = 0; o < comps; ++o)
    for (u32 tau = 0; tau < S::T; ++tau) {
      for (int r = 0; r < Cfg::R; ++r) xb[tau].x[r] = (E)bhat[(boff[o] << LOGN) + Cfg::prep_idx(tau, (u32)r)];
      const typename S::Tw* zeta = wg.pre[tau].t + Cfg::pre_off(LOGN - 1);      // the zeta records came with the forward's
      if (o + 1 < comps) {                                   // the digit row is needed again
        dot_product_into<E, Cfg, Pol, BC>((*acc[o])[tau].x, xa[tau].x, xb[tau].x, zeta, wg.ar, [](auto) {});
      } else {                                               // the last component may overwrite it
        if constexpr (BC) basecase<Cfg, Pol>(xa[tau].x, xb[tau].x, zeta, wg.ar);
        else pointwise<E, Cfg, Pol>(xa[tau].x, xb[tau].x, wg.ar);
        dot_accumulate<E, Cfg, Pol>((*acc[o])[tau].x, xa[tau].x, wg.ar);
      }
    }
}

inline bool params_ok(u32 n, u64 q, u64 psi) {
  if (n < 4 || (n & (n - 1)) || q < 3 || !(q & 1) || q >= ((u64)1 << 62)) return false;
  return h_powmod(psi % q, n, q) == q - 1;
}

// f(FusedShape of the plan, std::true_type / std::false_type: a product-family launch of the plan runs the base case), or 7
// for an n without fused kernels.
template <typename F>
int emu_with_shape(const HostTables& t, F&& f) {
  return with_fused_shape(t.elem_bytes, t.lazy, t.logn, 7, [&](auto sh) -> int {
    typedef decltype(sh) Sh;
    if constexpr (Sh::HAS_BC) { if (fused_use_bc<Sh>(t.bc_ok)) return f(sh, std::true_type()); }
    return f(sh, std::false_type());
  });
}

// What the gadget calls refuse of (terms, base_log, flags) for a plan: ApiCheck::gadget itself, one row, so that its row limit
// never speaks.  The stepping entry points answer 4 where it refuses.
inline bool gadget_ok(const HostTables& t, size_t terms, u32 base_log, u32 flags) {
  ApiCheck k{ApiPlan{t.n, t.elem_bytes, true, false, t.q}, "emu"};
  return k.gadget(1, terms, base_log, flags);
}

// The end of every *_api_check entry point: the status; *launch = 1 when the call would go on to its launch; msg receives the
// text tn_last_error would give.
inline int api_answer(const ApiCheck& k, bool go, int* launch, char* msg, size_t msg_len) {
  if (launch) *launch = go ? 1 : 0;
  if (msg && msg_len) std::snprintf(msg, msg_len, "%s", k.msg.c_str());
  return (int)k.st;
}

}  // namespace
