// bc_emu.cpp — TEST INFRASTRUCTURE: steps the product kernel's base-case path (forward stages 0 .. log2(n)-2, basecase(),
// inverse from the second stage on: fused_core.h) on the CPU, one emulated thread at a time, with the very headers the
// gfx950 kernel is compiled from.  Built with g++ by tests/test_basecase.py; nothing in tiny_ntt_amd/ loads it.
#include <stdint.h>
#include <stddef.h>
#include <vector>
#include "../../tiny_ntt_amd/csrc/plan_tables.h"

using namespace tn;

namespace {

template <int LOGN, int LPT>
int bc_polymul_emu(const HostTables& t, const u64* a, const u64* b, u64* c, size_t batch, bool cyclic) {
  typedef u64 E;
  typedef FusedCfg<E, LOGN, LPT> Cfg;
  typedef Policy<E, true> Pol;
  typedef Tw64 Tw;
  constexpr int LAST = Cfg::PHASES - 1;
  // as launch_fused_t does for the base-case kernel
  Arith<E> ar = h_make_arith<E>(t);
  ar.fninv = ar.bninv;
  ar.fninv_w1 = cyclic ? ar.bninv : ar.bninv_w1;
  const std::vector<Tw> fwd = h_fused_table<E>(cyclic ? t.cyc_bc : t.psi_bc, t),
                        inv = h_fused_table<E>(cyclic ? t.cyc_inv_brv : t.psi_inv_brv, t);
  std::vector<E> lds(Cfg::lds_elems());
  struct Regs { E x[Cfg::R]; };
  std::vector<Regs> xa(Cfg::THREADS), xb(Cfg::THREADS);
  std::vector<Tw> lds_fwd(fwd.begin() + Cfg::lds_tw_lo(), fwd.begin() + Cfg::lds_tw_hi());
  std::vector<Tw> lds_inv(inv.begin() + Cfg::lds_tw_lo(), inv.begin() + Cfg::lds_tw_hi());
  struct Pre { Tw t[Cfg::NPRE]; };
  std::vector<Pre> pre(Cfg::THREADS), prei(Cfg::THREADS);
  for (auto& p : prei) for (auto& r : p.t) r = Tw{~(u64)0, ~(u64)0};      // records the inverse must not read

  auto forward = [&](std::vector<Regs>& x) {
    for (u32 tau = 0; tau < (u32)Cfg::THREADS; ++tau) tw_prefetch<E, Cfg>(pre[tau].t, tau, fwd.data());
    static_for<0, Cfg::PHASES>([&](auto p_) {
      constexpr int p = decltype(p_)::value;
      for (u32 tau = 0; tau < (u32)Cfg::THREADS; ++tau) {
        const TwRefs<E> tw = {fwd.data(), lds_fwd.data(), pre[tau].t};
        fwd_phase<E, Cfg, Pol, p, true>(x[tau].x, tau, tw, ar);
      }
      if constexpr (p + 1 < Cfg::PHASES) {
        for (auto& v : lds) v = (E)0xDEADBEEFu;
        for (u32 tau = 0; tau < (u32)Cfg::THREADS; ++tau) ex_store<E, Cfg, p, p>(x[tau].x, tau, lds.data());
        for (u32 tau = 0; tau < (u32)Cfg::THREADS; ++tau) ex_load<E, Cfg, p, p + 1>(x[tau].x, tau, lds.data());
      }
    });
  };
  auto inverse = [&](std::vector<Regs>& x) {
    for (u32 tau = 0; tau < (u32)Cfg::THREADS; ++tau)
      tw_prefetch_stages<E, Cfg, Cfg::stage_begin(LAST), LOGN - 1>(prei[tau].t, tau, inv.data());
    static_for<0, Cfg::PHASES>([&](auto i_) {
      constexpr int p = Cfg::PHASES - 1 - decltype(i_)::value;
      for (u32 tau = 0; tau < (u32)Cfg::THREADS; ++tau) {
        const TwRefs<E> tw = {inv.data(), lds_inv.data(), prei[tau].t};
        inv_phase<E, Cfg, Pol, p, true>(x[tau].x, tau, tw, ar);
      }
      if constexpr (p > 0) {
        for (u32 tau = 0; tau < (u32)Cfg::THREADS; ++tau) ex_store<E, Cfg, p - 1, p>(x[tau].x, tau, lds.data());
        for (u32 tau = 0; tau < (u32)Cfg::THREADS; ++tau) ex_load<E, Cfg, p - 1, p - 1>(x[tau].x, tau, lds.data());
      }
    });
  };
  for (size_t row = 0; row < batch; ++row) {
    const size_t off = row << LOGN;
    for (u32 tau = 0; tau < (u32)Cfg::THREADS; ++tau) {
      for (int r = 0; r < Cfg::R; ++r) {
        xa[tau].x[r] = a[off + Cfg::jidx(0, tau, r)];
        xb[tau].x[r] = b[off + Cfg::jidx(0, tau, r)];
      }
      load_reduce<E, Cfg, Pol>(xa[tau].x, ar);
      load_reduce<E, Cfg, Pol>(xb[tau].x, ar);
    }
    forward(xa);
    forward(xb);
    for (u32 tau = 0; tau < (u32)Cfg::THREADS; ++tau)
      basecase<Cfg, Pol>(xa[tau].x, xb[tau].x, pre[tau].t + Cfg::pre_off(LOGN - 1), ar);
    inverse(xa);
    for (u32 tau = 0; tau < (u32)Cfg::THREADS; ++tau)
      for (int r = 0; r < Cfg::R; ++r) c[off + Cfg::jidx(0, tau, r)] = xa[tau].x[r];
  }
  return 0;
}

}  // namespace

extern "C" {

// 1 if a plan for (n, q, psi) runs the base-case product kernel
int bc_enabled(uint32_t n, uint64_t q, uint64_t psi) { return h_build_tables(n, q, psi, true).bc_ok ? 1 : 0; }

// exact replay of the base-case bound schedule for n = 2^logn, q = 2^k - c
int bc_sched_ok(uint32_t logn, int k, uint64_t c) { return h_bc_sched_ok(logn, k, c) ? 1 : 0; }
int split_sched_ok(uint32_t logn, int k, uint64_t c) { return h_split_sched_ok(logn, k, c) ? 1 : 0; }

// c = a * b in Z_q[x]/(x^n + 1) (or x^n - 1: cyclic) through the base-case path; -1 if the plan does not take it
int bc_polymul(uint32_t n, uint64_t q, uint64_t psi, const uint64_t* a, const uint64_t* b, uint64_t* c, size_t batch, int cyclic) {
  const HostTables t = h_build_tables(n, q, psi, true);
  if (!t.bc_ok || n != 4096) return -1;
  return bc_polymul_emu<12, fused_lpt(12)>(t, a, b, c, batch, cyclic != 0);
}

// one base-case pair on raw words (the caller keeps a0, a1 within the schedule's bound): out = {c0, c1}, not reduced
void bc_pair(int k, uint64_t c, uint64_t a0, uint64_t a1, uint64_t b0, uint64_t b1, uint64_t zeta, uint64_t* out) {
  const u64 q = (((u64)1) << k) - c;
  Arith<u64> ar;
  ar.q = q; ar.k = k; ar.fold_c = (u32)c; ar.mu = 0;
  ar.sk.mulp = (u32)1 << (k - 31);
  ar.sk.cf = (u32)((((unsigned __int128)1) << (k + 1)) % q);
  basecase_pair(a0, a1, b0, b1, h_make_tw64_split(zeta, q, k), ar);
  out[0] = a0; out[1] = a1;
}

// the record split_rec() makes of b, decoded: {w, x} with w = wlo + whi 2^p, x = xlo + xhi 2^p
void bc_split_rec(int k, uint64_t c, uint64_t b, uint64_t* out) {
  const u64 q = (((u64)1) << k) - c;
  const Tw64 t = split_rec(b, k, (u32)c, q);
  out[0] = (u64)(u32)t.w + ((t.w >> 32) << (k - 31));
  out[1] = (u64)(u32)t.wp + ((t.wp >> 32) << (k - 31));
}

}
