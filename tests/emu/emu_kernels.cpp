// emu_kernels.cpp — TEST INFRASTRUCTURE: steps the per-thread code of the product kernel, the standalone transforms and the
// constant-geometry kernels (tiny_ntt_amd/csrc/fused_core.h, cg_core.h, modarith.h, plan_tables.h — the very headers the
// gfx950 kernels are compiled from) on the CPU, one emulated thread at a time with barriers between phases, so index maps,
// LDS layouts, table semantics and lazy-reduction bounds can be checked without a GPU; also the layout, schedule and
// arithmetic probes, and the entry points' argument checks (csrc/api_checks.h: emu_api_check).  The fused shape, tables and constants of a launch and the row planning come from launch_plan.h, the
// header the launchers take them from (the Stepper and emu_with_shape: emu_stepper.h).  One of the five objects of
// tests/emu/_build/libemu.so (tests/emu/Makefile); loaded by tests/conftest.py (Emu).  It is not a product path and nothing in
// tiny_ntt_amd/ loads it.
#include "emu_stepper.h"
#include "../../tiny_ntt_amd/csrc/cg_core.h"
#include "../../tiny_ntt_amd/csrc/api_checks.h"
#include <cstdio>

namespace {

// Same steps as polymul_fused_kernel (kernels.hip), one emulated thread at a time; BC: its base-case instantiation.
template <typename E, int LOGN, int LPT, bool LAZY, bool CIN = false, bool BC = false>
int fused_polymul_emu(const HostTables& t, const u64* a, const u64* b, u64* c, size_t batch, bool cyclic) {
  typedef Policy<E, LAZY, CIN> Pol;
  typedef Stepper<E, LOGN, LPT, Pol, BC> S;
  typedef typename S::Cfg Cfg;
  const FusedProductSetup<E> su = fused_product_setup(h_make_arith<E>(t), BC, cyclic);
  S wg{su.ar};
  const typename S::Table fwd(t, su.fwd), inv(t, su.inv);
  std::vector<typename S::Regs> xa(S::T), xb(S::T);
  for (size_t row = 0; row < batch; ++row) {
    const size_t off = row << LOGN;
    for (u32 tau = 0; tau < S::T; ++tau) {
      for (int r = 0; r < Cfg::R; ++r) {
        xa[tau].x[r] = (E)a[off + Cfg::jidx(0, tau, r)];
        xb[tau].x[r] = (E)b[off + Cfg::jidx(0, tau, r)];
      }
      load_reduce<E, Cfg, Pol>(xa[tau].x, wg.ar);
      load_reduce<E, Cfg, Pol>(xb[tau].x, wg.ar);
    }
    wg.forward(xa, fwd);
    wg.forward(xb, fwd);
    for (u32 tau = 0; tau < S::T; ++tau) {
      if constexpr (BC) basecase<Cfg, Pol>(xa[tau].x, xb[tau].x, wg.pre[tau].t + Cfg::pre_off(LOGN - 1), wg.ar);   // the zeta records came with the forward's
      else pointwise<E, Cfg, Pol>(xa[tau].x, xb[tau].x, wg.ar);
    }
    wg.inverse(xa, inv);
    for (u32 tau = 0; tau < S::T; ++tau)
      for (int r = 0; r < Cfg::R; ++r) c[off + Cfg::jidx(0, tau, r)] = xa[tau].x[r];
  }
  return 0;
}

// Same steps as ntt_fused_kernel (kernels.hip), one emulated thread at a time.
template <typename E, int LOGN, int LPT, bool LAZY>
int fused_ntt_emu(const HostTables& t, int mode, const u64* in, u64* out) {
  typedef Policy<E, LAZY> Pol;
  typedef Stepper<E, LOGN, LPT, Pol> S;
  typedef typename S::Cfg Cfg;
  const FusedNttSetup<E> su = fused_ntt_setup(h_make_arith<E>(t), mode);
  S wg{su.ar};
  const typename S::Table tab(t, su.tab);
  const Arith<E>& ar = wg.ar;
  std::vector<E> nat(Cfg::N);                                 // the natural-order image
  std::vector<typename S::Regs> x(S::T);
  constexpr int LAST = Cfg::PHASES - 1;
  const u32 T = S::T;
  if (mode == FNTT_CYCLIC_INV) {
    for (u32 tau = 0; tau < T; ++tau) for (int r = 0; r < Cfg::R; ++r) nat[Cfg::nat_addr(Cfg::jidx(0, tau, r))] = Pol::load((E)in[Cfg::jidx(0, tau, r)], ar);
    for (u32 tau = 0; tau < T; ++tau) for (int r = 0; r < Cfg::R; ++r) x[tau].x[r] = nat[Cfg::nat_addr(bitrev(Cfg::jidx(LAST, tau, r), LOGN))];
    wg.inverse(x, tab);
    for (u32 tau = 0; tau < T; ++tau) for (int r = 0; r < Cfg::R; ++r) out[Cfg::jidx(0, tau, r)] = x[tau].x[r];
    return 0;
  }
  for (u32 tau = 0; tau < T; ++tau) for (int r = 0; r < Cfg::R; ++r) {
    const u32 j = Cfg::jidx(0, tau, r);
    x[tau].x[r] = (LAZY && r >= Cfg::R / 2) ? (E)in[j] : Pol::load((E)in[j], ar);     // as ntt_fused_kernel: only the "u" half is reduced
  }
  wg.forward(x, tab);
  for (u32 tau = 0; tau < T; ++tau) for (int r = 0; r < Cfg::R; ++r)
    nat[Cfg::nat_addr(bitrev(Cfg::jidx(LAST, tau, r), LOGN))] = LAZY ? Pol::canon(x[tau].x[r], ar) : x[tau].x[r];
  for (u32 tau = 0; tau < T; ++tau) for (int r = 0; r < Cfg::R; ++r) out[Cfg::jidx(0, tau, r)] = nat[Cfg::nat_addr(Cfg::jidx(0, tau, r))];
  return 0;
}

// Sequential restatement of cg_kernel's arithmetic with the product's tables
// and modarith (thread mapping there is a plain strided loop).
template <typename E>
int cg_emu(const HostTables& t, int mode, const u64* a, const u64* b, u64* out, u64* trace) {
  typedef typename TwOf<E>::type Tw;
  const Arith<E> ar = h_make_arith<E>(t);
  const u32 n = t.n, logn = t.logn, pairs = n / 2;
  const std::vector<Tw> omega = h_tw_table<E>(t.omega_pow, t.q), omega_inv = h_tw_table<E>(t.omega_inv_pow, t.q),
                        psi_pow = h_tw_table<E>(t.psi_pow, t.q), psi_inv_ninv = h_tw_table<E>(t.psi_inv_ninv, t.q);
  auto load_brv = [&](const u64* in, const Tw* tw) {
    std::vector<E> buf(n);
    for (u32 i = 0; i < n; ++i) buf[h_brv(i, logn)] = tw ? mul_tw((E)in[i], tw[i], ar.q) : mul_tw((E)in[i], ar.one, ar.q);
    return buf;
  };
  auto stages = [&](std::vector<E> src, const Tw* tab, u64* tr) {
    std::vector<E> dst(n);
    for (u32 stage = 1; stage <= logn; ++stage) {
      const u32 k = n >> stage;
      for (u32 i = 0; i < pairs; ++i) {
        const E left = src[2 * i], right = src[2 * i + 1];
        const E tt = mul_tw(right, tab[i & ~(k - 1)], ar.q);
        dst[i] = csub((E)(left + tt), ar.q);
        dst[i + pairs] = left >= tt ? (E)(left - tt) : (E)(left + (ar.q - tt));
      }
      if (tr) for (u32 i = 0; i < n; ++i) tr[(size_t)(stage - 1) * n + i] = dst[i];
      src.swap(dst);
    }
    return src;
  };
  if (mode == 0 || mode == 3) {
    auto r = stages(load_brv(a, mode == 3 ? psi_pow.data() : nullptr), omega.data(), trace);
    for (u32 i = 0; i < n; ++i) out[i] = r[i];
  } else if (mode == 1) {
    auto r = stages(load_brv(a, nullptr), omega_inv.data(), nullptr);
    for (u32 i = 0; i < n; ++i) out[i] = mul_tw(r[i], ar.ninv, ar.q);
  } else {
    auto ra = stages(load_brv(a, psi_pow.data()), omega.data(), nullptr);
    auto rb = stages(load_brv(b, psi_pow.data()), omega.data(), nullptr);
    std::vector<E> cc(n);
    for (u32 i = 0; i < n; ++i) cc[h_brv(i, logn)] = mulmod_barrett(ra[i], rb[i], ar.q, ar.mu, ar.k);
    auto rc = stages(cc, omega_inv.data(), nullptr);
    for (u32 i = 0; i < n; ++i) out[i] = mul_tw(rc[i], psi_inv_ninv[i], ar.q);
  }
  return 0;
}


// The constant-geometry kernels' trips (cg_core.h / cg_kernels.hip), one emulated lane-step at a time with the LDS image and
// the LDS twiddle table between them.  mode: 0 cg_ntt, 1 cg_intt, 2 nwc_poly_mult, 3 twist + cg_ntt, 4 cyclic product.
// flags: bit 0 = wave-uniform trips take their twiddles from the global table (scalar loads in the kernel) instead of LDS;
//        bit 1 = no reversal: the inverse transform of a product reads a re-staged inverse table (plans whose omega is not a root)
template <typename E, int GROUP, int LAYOUT, int AM>
int cgm_emu(const HostTables& t, int mode, int flags, const u64* a, const u64* b, u64* out, u64* trace) {
  typedef CgGeom<GROUP> Ge;
  typedef CgMap<E, GROUP, LAYOUT> M;
  typedef CgArith<E, AM> A;
  typedef typename TwOf<E>::type Tw;
  constexpr int R = Ge::R, L = Ge::L;
  const u32 n = t.n, logn = t.logn;
  if ((int)logn < L) return 7;
  if (trace && (AM == CGA_SPLIT_LAZY || AM == CGA_SPLIT_SCHED)) return 7;
  if (AM == CGA_SPLIT_SCHED && !t.cg_sched) return 7;
  const Arith<E> ar = h_make_arith<E>(t);
  const u32 TP = n >> L, ntrips = Ge::ntrips(logn), r1 = Ge::first_stages(logn);
  const bool split = AM != CGA_SHOUP;
  auto table = [&](const std::vector<u64>& v) { return split ? h_fused_table<E>(v, t) : h_tw_table<E>(v, t.q); };
  const std::vector<Tw> fwd = table(t.omega_pow), inv = table(t.omega_inv_pow), psi_pow = table(t.psi_pow), psi_inv_ninv = table(t.psi_inv_ninv);
  const Tw ninv = split ? ar.fninv : ar.ninv;
  const bool big = n >= 512 && TP >= 256;
  std::vector<E> img(M::span(n) + 4, (E)0xDEADBEEFu);
  std::vector<Tw> ldstab(n / 2 + 1);
  auto stage_table = [&](const std::vector<Tw>& g) { for (u32 j = 0; j <= n / 2; ++j) ldstab[cg_twmap<GROUP, LAYOUT>(j, big)] = g[j]; };
  struct Regs { E x[R]; Tw w0[GROUP]; };
  constexpr bool CAN_MERGE = TN_CG_MERGE_TWIST && A::LAZY;           // cg_kernel_impl.h: the twist of stage 1's right inputs rides the butterflies

  // x: registers in bit-reversed order (x[brvL(e')] = element ls + e' TP of the input list) -> natural order (x[e] = output ls + e TP)
  auto transform = [&](std::vector<Regs>& x, bool inverse, bool rev, u64* tr, bool merged = false) {
    const Tw* glob = inverse ? inv.data() : fwd.data();
    auto run_first = [&](auto nst_) {
      constexpr int NST = decltype(nst_)::value;
      for (u32 ls = 0; ls < TP; ++ls) {
        const u32 T = h_brv(ls, logn - L);
        auto tw = [&](auto j_, auto h_) { return glob[(u32)decltype(h_)::value * (n >> (decltype(j_)::value + 1))]; };
        auto after = [&](auto j_) { if (tr) for (u32 e = 0; e < (u32)R; ++e) tr[(size_t)decltype(j_)::value * n + Ge::pos(logn, decltype(j_)::value + 1, T, e)] = x[ls].x[e]; };
        if constexpr (CAN_MERGE) {
          if (merged) cg_trip<E, GROUP, AM, NST, false, 0, true>(x[ls].x, ar, tw, after, [&](auto g_) { return x[ls].w0[decltype(g_)::value]; });
          else cg_trip<E, GROUP, AM, NST, false>(x[ls].x, ar, tw, after);
        } else cg_trip<E, GROUP, AM, NST, false>(x[ls].x, ar, tw, after);
        if (ntrips > 1) for (u32 e = 0; e < (u32)R; ++e) img[M::at(Ge::pos(logn, NST, T, e))] = x[ls].x[e];
      }
    };
    switch (r1) { case 1: run_first(std::integral_constant<int, 1>()); break;
                  case 2: if constexpr (L >= 2) run_first(std::integral_constant<int, 2>()); break;
                  case 3: if constexpr (L >= 3) run_first(std::integral_constant<int, 3>()); break;
                  case 4: if constexpr (L >= 4) run_first(std::integral_constant<int, 4>()); break; }
    u32 s0 = r1;
    for (u32 trip = 1; trip < ntrips; ++trip, s0 += L) {
      for (u32 ls = 0; ls < TP; ++ls) for (u32 e = 0; e < (u32)R; e += 2) {
        const CgPair<E> v = *reinterpret_cast<const CgPair<E>*>(&img[M::step(M::at(R * ls), e)]);
        x[ls].x[e] = v.lo; x[ls].x[e + 1] = v.hi;
      }
      for (auto& v : img) v = (E)0xDEADBEEFu;
      const bool uniform = (flags & 1) && (int)logn - (int)s0 - L >= 6;     // the trip's twiddles depend on T >> 6 only
      for (u32 ls = 0; ls < TP; ++ls) {
        const u32 T = ls, base0 = cg_tw_base0<GROUP>(logn, s0, T);
        auto after = [&](auto j_) { if (tr) for (u32 e = 0; e < (u32)R; ++e) tr[(size_t)(s0 + decltype(j_)::value) * n + Ge::pos(logn, decltype(j_)::value + 1, T, e)] = x[ls].x[e]; };
        auto idx = [&](int j, u32 h) { return h * (n >> (j + 1)) + (base0 >> j); };
        auto run = [&](auto par_) {
          constexpr int PAR = decltype(par_)::value;
          if (uniform) cg_trip<E, GROUP, AM, L, false, PAR>(x[ls].x, ar, [&](auto j_, auto h_) { return glob[idx(decltype(j_)::value, decltype(h_)::value)]; }, after);
          else if (rev) cg_trip<E, GROUP, AM, L, true, PAR>(x[ls].x, ar, [&](auto j_, auto h_) { return ldstab[cg_twmap<GROUP, LAYOUT>(n / 2 - idx(decltype(j_)::value, decltype(h_)::value), big)]; }, after);
          else cg_trip<E, GROUP, AM, L, false, PAR>(x[ls].x, ar, [&](auto j_, auto h_) { return ldstab[cg_twmap<GROUP, LAYOUT>(idx(decltype(j_)::value, decltype(h_)::value), big)]; }, after);
        };
        if (AM == CGA_SPLIT_SCHED && (s0 & 1u)) run(std::integral_constant<int, 1>()); else run(std::integral_constant<int, 0>());
      }
      if (trip + 1 < ntrips) for (u32 ls = 0; ls < TP; ++ls) for (u32 e = 0; e < (u32)R; ++e) img[M::at(Ge::pos(logn, L, ls, e))] = x[ls].x[e];
    }
  };
  auto load = [&](std::vector<Regs>& x, const u64* in, const Tw* twist) {       // returns: the first stage is the merged one
    for (u32 ls = 0; ls < TP; ++ls) for (u32 e = 0; e < (u32)R; ++e) {
      const u32 i = ls + e * TP;
      if (twist && CAN_MERGE && e >= (u32)GROUP) { x[ls].x[Ge::brvL(e)] = (E)in[i]; x[ls].w0[Ge::brvL(e) >> 1] = twist[i]; }
      else x[ls].x[Ge::brvL(e)] = twist ? A::in_mul((E)in[i], twist[i], ar) : A::in_red((E)in[i], ar);
    }
    return twist && CAN_MERGE;
  };
  std::vector<Regs> xa(TP), xb(TP);
  if (mode == 0 || mode == 3) {
    stage_table(fwd);
    const bool m = load(xa, a, mode == 3 ? psi_pow.data() : nullptr);
    transform(xa, false, false, trace, m);
    for (u32 ls = 0; ls < TP; ++ls) for (u32 e = 0; e < (u32)R; ++e) out[ls + e * TP] = A::out_canon(xa[ls].x[e], ar);
  } else if (mode == 1) {
    stage_table(inv);
    load(xa, a, nullptr);
    transform(xa, true, false, nullptr);
    for (u32 ls = 0; ls < TP; ++ls) for (u32 e = 0; e < (u32)R; ++e) out[ls + e * TP] = A::out_mul(xa[ls].x[e], ninv, ar);
  } else {
    const Tw* twist = mode == 4 ? nullptr : psi_pow.data();
    const bool rev = !(flags & 2);
    stage_table(fwd);
    const bool ma = load(xa, a, twist); transform(xa, false, false, nullptr, ma);
    const bool mb = load(xb, b, twist); transform(xb, false, false, nullptr, mb);
    for (u32 ls = 0; ls < TP; ++ls) {
      E c[R];
      for (u32 e = 0; e < (u32)R; ++e) c[e] = A::pointwise(xa[ls].x[e], xb[ls].x[e], ar);
      for (u32 e = 0; e < (u32)R; ++e) xa[ls].x[Ge::brvL(e)] = c[e];
    }
    if (!rev) stage_table(inv);
    transform(xa, true, rev, nullptr);
    for (u32 ls = 0; ls < TP; ++ls) for (u32 e = 0; e < (u32)R; ++e) {
      const u32 i = ls + e * TP;
      out[i] = A::out_mul(xa[ls].x[e], twist ? psi_inv_ninv[i] : ninv, ar);
    }
  }
  return 0;
}

template <typename E, int AM>
int cgm_dispatch(const HostTables& t, int mode, int group, int layout, int flags, const u64* a, const u64* b, u64* out, u64* trace) {
#define TN_CGM(G, LY) if (group == G && layout == LY) return cgm_emu<E, G, LY, AM>(t, mode, flags, a, b, out, trace);
  TN_CGM(1, 0) TN_CGM(1, 1) TN_CGM(1, 2) TN_CGM(2, 0) TN_CGM(2, 1) TN_CGM(2, 2)
  TN_CGM(4, 0) TN_CGM(4, 1) TN_CGM(4, 2) TN_CGM(8, 0) TN_CGM(8, 1) TN_CGM(8, 2)
#undef TN_CGM
  return 7;
}

// Layout probes for the LDS bank-conflict simulator (tests/test_lds_banks.py).
// what: 0 THREADS, 1 R, 2 PHASES, 3 lds_elems, 4 ex_wave_local(arg0), 5 jidx(arg0=phase, arg1=tau, arg2=r),
//       6 ex_addr(arg0=exchange, arg1=j), 7 pos(arg0)
template <typename E, int LOGN, int LPT> static long cfg_probe(int what, unsigned a0, unsigned a1, unsigned a2) {
  typedef FusedCfg<E, LOGN, LPT> C;
  switch (what) {
    case 0: return C::THREADS;
    case 1: return C::R;
    case 2: return C::PHASES;
    case 3: return C::lds_elems();
    case 4: return C::ex_wave_local((int)a0);
    case 5: return C::jidx((int)a0, a1, a2);
    case 6: return C::ex_addr((int)a0, a1);
    case 7: return C::pos((int)a0);
  }
  return -1;
}
}  // namespace

extern "C" {

// 0 ok, 2 bad params, 7 unsupported n.  Coefficients travel as uint64 regardless of lane width.
// flags: bit 0 = canonical policy, bit 1 = cyclic product (x^n - 1) instead of negacyclic, bit 2 = inputs promised canonical.
int emu_fused_poly_mult(uint32_t n, uint64_t q, uint64_t psi, int flags, const uint64_t* a, const uint64_t* b,
                        uint64_t* c, size_t batch) {
  if (!params_ok(n, q, psi)) return 2;
  const bool cyc = (flags & 2) != 0;
  const HostTables t = h_build_tables(n, q, psi, !(flags & 1));
  if (flags & 4) {                       // promised-canonical inputs (TN_PLAN_CANONICAL_INPUTS): n = 4096, lazy 64-bit lanes, schedule replayed
    if (!(t.cin_ok && t.logn == 12 && t.lazy && t.elem_bytes == 8) || cyc) return 7;
    return fused_polymul_emu<u64, 12, fused_lpt(12), true, true>(t, a, b, c, batch, false);
  }
  return emu_with_shape(t, [&](auto sh, auto) {           // (the base-case instantiation is stepped by bc_polymul)
    typedef decltype(sh) Sh;
    return fused_polymul_emu<typename Sh::E, Sh::LOGN, Sh::LPT, Sh::LAZY>(t, a, b, c, batch, cyc);
  });
}

// mode: 0 twist + forward (natural out), 1 cg_ntt, 2 cg_intt — the register-tiled standalone transforms
int emu_fused_ntt(uint32_t n, uint64_t q, uint64_t psi, int force_canonical, int mode, const uint64_t* in, uint64_t* out) {
  if (!params_ok(n, q, psi)) return 2;
  const HostTables t = h_build_tables(n, q, psi, !force_canonical);
  return emu_with_shape(t, [&](auto sh, auto) {
    typedef decltype(sh) Sh;
    return fused_ntt_emu<typename Sh::E, Sh::LOGN, Sh::LPT, Sh::LAZY>(t, mode, in, out);
  });
}

// ---- the product kernel's base-case instantiation (tests/test_basecase.py) ----
// 1 if a plan for (n, q, psi) runs the base-case product kernel
int bc_enabled(uint32_t n, uint64_t q, uint64_t psi) { return h_build_tables(n, q, psi, true).bc_ok ? 1 : 0; }

// exact replay of the base-case bound schedule for n = 2^logn, q = 2^k - c
int bc_sched_ok(uint32_t logn, int k, uint64_t c) { return h_bc_sched_ok(logn, k, c) ? 1 : 0; }
int split_sched_ok(uint32_t logn, int k, uint64_t c) { return h_split_sched_ok(logn, k, c) ? 1 : 0; }

// c = a * b in Z_q[x]/(x^n + 1) (or x^n - 1: cyclic) through the base-case path; -1 if the plan does not take it
int bc_polymul(uint32_t n, uint64_t q, uint64_t psi, const uint64_t* a, const uint64_t* b, uint64_t* c, size_t batch, int cyclic) {
  const HostTables t = h_build_tables(n, q, psi, true);
  if (!t.bc_ok) return -1;
  constexpr int L = FUSED_BC_LOGN;
  static_assert(fused_has_bc<u64, L, fused_lpt(L), true>(), "no base-case kernel is built");
  return fused_polymul_emu<u64, L, fused_lpt(L), true, false, true>(t, a, b, c, batch, cyclic != 0);
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

// ---- row planning of the persistent launches (launch_plan.h) ----
// which: 0 the fused kernels' policy, 1 the constant-geometry kernels'.  what: 0 chunk_bytes, 1 min_chunks, 2 enabled,
// 3 single_rows_without_slot
long emu_row_policy(int which, int what) {
  const RowPolicy& p = which ? CG_ROWS : FUSED_ROWS;
  return what == 0 ? (long)p.chunk_bytes : what == 1 ? (long)p.min_chunks : what == 2 ? (long)p.enabled : (long)p.single_rows_without_slot;
}
// returns 1 for dynamic rows, 0 for the fixed stride; *chunk = rows per hand-out
int emu_plan_rows(int which, size_t row_bytes, size_t batch, size_t resident, uint32_t* chunk) {
  const RowPlan rp = plan_rows(row_bytes, batch, resident, which ? CG_ROWS : FUSED_ROWS);
  *chunk = rp.chunk;
  return rp.dynamic ? 1 : 0;
}

int emu_is_lazy(uint32_t n, uint64_t q, uint64_t psi) {
  if (!params_ok(n, q, psi)) return -1;
  return h_build_tables(n, q, psi, true).lazy ? 1 : 0;
}

// The policy flags h_build_tables decides for a plan (n, q, psi): bit 0 lazy, 1 cg_lazy, 2 cg_sched, 3 cin_ok, 4 bc_ok; -1 for
// bad parameters.  (tests/policy_moduli.py's FLAG_ENTRIES and tools/find_policy_moduli.py read every flag from here.)
int emu_plan_flags(uint32_t n, uint64_t q, uint64_t psi) {
  if (!params_ok(n, q, psi)) return -1;
  const HostTables t = h_build_tables(n, q, psi, true);
  return (t.lazy ? 1 : 0) | (t.cg_lazy ? 2 : 0) | (t.cg_sched ? 4 : 0) | (t.cin_ok ? 8 : 0) | (t.bc_ok ? 16 : 0);
}

// mode: 0 cg_ntt, 1 cg_intt, 2 nwc_poly_mult, 3 twist + cg_ntt.  trace may be NULL ([logn][n] otherwise, mode 0/3).
int emu_cg(uint32_t n, uint64_t q, uint64_t psi, int mode, const uint64_t* a, const uint64_t* b, uint64_t* out, uint64_t* trace) {
  if (!params_ok(n, q, psi)) return 2;
  const HostTables t = h_build_tables(n, q, psi, true);
  return t.elem_bytes == 8 ? cg_emu<u64>(t, mode, a, b, out, trace) : cg_emu<u32>(t, mode, a, b, out, trace);
}

// The trips of cg_kernels.hip stepped on the CPU.  am: 0 Shoup records, 1 split records canonical, 2 split records lazy
// 3 split records lazy with the static fold schedule (1, 2, 3 need a plan that is lazy with 64-bit lanes; 3 an even log2 n).  7 = unsupported combination.
int emu_cgm(uint32_t n, uint64_t q, uint64_t psi, int mode, int group, int layout, int am, int flags, const uint64_t* a,
            const uint64_t* b, uint64_t* out, uint64_t* trace) {
  if (!params_ok(n, q, psi)) return 2;
  const HostTables t = h_build_tables(n, q, psi, true);
  if (am < 0 || am > 3 || (am != 0 && !(t.lazy && t.elem_bytes == 8 && (am == 1 || t.cg_lazy)))) return 7;
  if (t.elem_bytes == 8) {
    if (am == 0) return cgm_dispatch<u64, CGA_SHOUP>(t, mode, group, layout, flags, a, b, out, trace);
    if (am == 1) return cgm_dispatch<u64, CGA_SPLIT_CANON>(t, mode, group, layout, flags, a, b, out, trace);
    if (am == 2) return cgm_dispatch<u64, CGA_SPLIT_LAZY>(t, mode, group, layout, flags, a, b, out, trace);
    return cgm_dispatch<u64, CGA_SPLIT_SCHED>(t, mode, group, layout, flags, a, b, out, trace);
  }
  return cgm_dispatch<u32, CGA_SHOUP>(t, mode, group, layout, flags, a, b, out, trace);
}

// Layout probes of the constant-geometry kernels (64-bit lanes): what 0 = CgMap::at(x), 1 = cg_twmap(x) (n >= 512), 2 = CgMap::span(x)
long emu_cgm_probe(int group, int layout, int what, unsigned x) {
#define TN_CGP(G, LY) if (group == G && layout == LY) return what == 0 ? (long)CgMap<u64, G, LY>::at(x) : what == 1 ? (long)cg_twmap<G, LY>(x, true) : (long)CgMap<u64, G, LY>::span(x);
  TN_CGP(1, 0) TN_CGP(1, 1) TN_CGP(1, 2) TN_CGP(2, 0) TN_CGP(2, 1) TN_CGP(2, 2)
  TN_CGP(4, 0) TN_CGP(4, 1) TN_CGP(4, 2) TN_CGP(8, 0) TN_CGP(8, 1) TN_CGP(8, 2)
#undef TN_CGP
  return -1;
}

// see cfg_probe() above for `what`
long emu_cfg_probe(int logn, int elem_bytes, int what, unsigned a0, unsigned a1, unsigned a2) {
  return with_fused_shape(elem_bytes, false, (u32)logn, -1L, [&](auto sh) {
    typedef decltype(sh) Sh;
    return cfg_probe<typename Sh::E, Sh::LOGN, Sh::LPT>(what, a0, a1, a2);
  });
}

// Direct probes of the arithmetic primitives (for property tests).
uint64_t emu_mul_tw64(uint64_t a, uint64_t w, uint64_t q) { return mul_tw(a, h_make_tw64(w, q), q); }
uint64_t emu_mul_tw64_lazy(uint64_t a, uint64_t w, uint64_t q) { return mul_tw_lazy(a, h_make_tw64(w, q), q); }
uint32_t emu_mul_tw32(uint32_t a, uint32_t w, uint32_t q) { return mul_tw(a, h_make_tw32(w, q), q); }
uint64_t emu_barrett64(uint64_t a, uint64_t b, uint64_t q) {
  const int k = h_bitlen(q);
  return mulmod_barrett(a, b, q, (u64)((((unsigned __int128)1) << (2 * k)) / q), k);
}
uint32_t emu_barrett32(uint32_t a, uint32_t b, uint32_t q) {
  const int k = h_bitlen(q);
  return mulmod_barrett(a, b, q, (u64)((((unsigned __int128)1) << (2 * k)) / q), k);
}
uint64_t emu_fold64(uint64_t x, uint64_t q) { const int k = h_bitlen(q); return fold(x, k, (u32)((((u64)1) << k) - q)); }
// lazy 64-bit pointwise product on two ARBITRARY words (folds them first, as pointwise() does); -1 if (k, c) is not admissible
int emu_pw_fast_ok(uint64_t q) { const int k = h_bitlen(q); return h_pw_fast_ok(q, k, (((u64)1) << k) - q) ? 1 : 0; }
uint64_t emu_pointwise_lazy64(uint64_t a, uint64_t b, uint64_t q) {
  const int k = h_bitlen(q);
  Arith<u64> ar; ar.q = q; ar.k = k; ar.fold_c = (u32)((((u64)1) << k) - q); ar.mu = 0;
  return pointwise_lazy(a, b, ar);
}
// split-constant product (lazy 64-bit lanes): u + a*w as mul_sp_acc computes it; *ok = 0 if (k, c) is not admissible
uint64_t emu_mul_sp_acc(uint64_t u, uint64_t a, uint64_t w, uint64_t q) {
  const int k = h_bitlen(q), p = k - 31;
  SplitK sk; sk.mulp = (u32)1 << p; sk.cf = (u32)((((unsigned __int128)1) << (p + 32)) % q);
  return mul_sp_acc(u, a, h_make_tw64_split(w, q, k), sk);
}
int emu_split_sched_ok(uint32_t logn, uint64_t q) { const int k = h_bitlen(q); return h_split_sched_ok(logn, k, (((u64)1) << k) - q) ? 1 : 0; }
// schedule statistics for one shape: what 0 folds in a forward transform per thread, 1 folds in an inverse, 2 forward output bound (units of 2^k/4096), 3 pw_fold_b
long emu_split_sched_stat(int logn, int what) {
  auto stat = [&](auto cfg) -> long {
    typedef decltype(cfg) C; typedef SplitSched<C> S;
    long f = 0, i = 0;
    for (int s = 0; s < C::LOGN; ++s) for (int r = 0; r < C::R; ++r) { f += S::D.ffold[s][r]; i += S::D.ifold[s][r]; }
    return what == 0 ? f : what == 1 ? i : what == 2 ? S::D.fout : (long)S::D.pw_fold_b;
  };
  return with_fused_shape(8, true, (u32)logn, -1L, [&](auto sh) { return stat(typename decltype(sh)::Cfg()); });
}
uint32_t emu_fold32(uint32_t x, uint32_t q) { const int k = h_bitlen(q); return fold(x, k, (u32)((((u64)1) << k) - q)); }

// The argument checks of the device entry point `entry` (api_checks.h: the step list capi.cpp runs before its launch) on a plan
// view made of (n, elem_bytes, has_fused, omega_only, q); n == 0 is a NULL plan.  a, b: the inputs in the order of the C
// signature (b unused where there is one); out: the output; sets: bhat_rows / bhat_sets.  Returns the status, or -1 for an
// unknown entry; *launch = 1 when the call would go on to its launch; msg receives the text tn_last_error would give.
int emu_api_check(const char* entry, uint32_t n, int elem_bytes, int has_fused, int omega_only, uint64_t q, const void* a, const void* b,
                  const void* out, size_t sets, size_t batch, size_t terms, int out_prepared, uint32_t base_log, uint32_t flags, int* launch,
                  char* msg, size_t msg_len) {
  ApiCheck k{ApiPlan{n, elem_bytes, has_fused != 0, omega_only != 0, q}, entry};
  const std::string e = entry;
  bool go;
  if (e == "tn_poly_mult_dev" || e == "tn_cyclic_poly_mult_dev") go = check_product(k, a, b, out, batch, e == "tn_cyclic_poly_mult_dev");
  else if (e == "tn_ntt_forward_dev" || e == "tn_ntt_inverse_dev" || e == "tn_twisted_ntt_forward_dev")
    go = check_transform(k, a, out, batch, e == "tn_twisted_ntt_forward_dev");
  else if (e == "tn_prepare_dev" || e == "tn_unprepare_dev") go = check_prepare(k, a, out, batch);
  else if (e == "tn_schoolbook_dev") go = check_rows(k, a, b, out, batch);
  else if (e == "tn_pointwise_mul_dev") go = check_pointwise(k, a, b, out, batch);
  else if (e == "tn_poly_mult_prepared_dev") go = check_mult_prepared(k, a, b, sets, out, batch);
  else if (e == "tn_poly_dot_prepared_dev") go = check_dot(k, a, b, sets, out, batch, terms, 0, "rows of a");
  else if (e == "tn_poly_dot_hat_dev") go = check_dot(k, a, b, sets, out, batch, terms, out_prepared, "rows of ahat");
  else if (e == "tn_gadget_decompose_dev") go = check_gadget_decompose(k, a, out, batch, terms, base_log, flags);
  else if (e == "tn_poly_gadget_dot_prepared_dev") go = check_gadget_dot(k, a, b, sets, out, batch, terms, base_log, flags);
  else if (e == "tn_fill_lcg_dev") go = check_fill(k, out != nullptr, batch);
  else if (e == "tn_checksum_rows_dev") go = check_fill(k, a && out, batch);
  else return -1;
  return api_answer(k, go, launch, msg, msg_len);
}

}  // extern "C"
