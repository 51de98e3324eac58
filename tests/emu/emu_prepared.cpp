// emu_prepared.cpp — TEST INFRASTRUCTURE: steps the prepared-operand kernels (prepare_fused_kernel, polymul_prepared_kernel:
// tiny_ntt_amd/csrc/kernels_prepared.hip) on the CPU, one emulated thread at a time, with the Stepper of emu_stepper.h, the headers
// the gfx950 kernels are compiled from and the prepared-order index map the kernels use (FusedCfg::prep_idx).  Shape and base
// case come from emu_with_shape, tables and constants from fused_product_setup (launch_plan.h), as in the launchers.  Part of
// tests/emu/_build/libemu.so; used by tests/test_prepared_emu.py and tests/test_gpu_prepared.py.
#include "emu_stepper.h"

namespace {

// Same steps as prepare_fused_kernel, one emulated thread at a time; BC: the plan's product runs the base case.
template <typename Sh, bool BC>
int prepare_emu(const HostTables& t, const u64* b, u64* bhat, size_t rows) {
  typedef typename Sh::E E;
  constexpr int LOGN = Sh::LOGN;
  typedef Policy<E, Sh::LAZY> Pol;
  typedef Stepper<E, LOGN, Sh::LPT, Pol, BC> S;
  typedef typename S::Cfg Cfg;
  const FusedProductSetup<E> su = fused_product_setup(h_make_arith<E>(t), BC, false);
  S wg{su.ar};
  const typename S::Table fwd(t, su.fwd);
  std::vector<typename S::Regs> x(S::T);
  for (size_t row = 0; row < rows; ++row) {
    const size_t off = row << LOGN;
    for (u32 tau = 0; tau < S::T; ++tau) {
      for (int r = 0; r < Cfg::R; ++r) x[tau].x[r] = (E)b[off + Cfg::jidx(0, tau, r)];
      load_reduce<E, Cfg, Pol>(x[tau].x, wg.ar);
    }
    wg.forward(x, fwd);
    for (u32 tau = 0; tau < S::T; ++tau)
      for (int r = 0; r < Cfg::R; ++r) bhat[off + Cfg::prep_idx(tau, (u32)r)] = Pol::canon(x[tau].x[r], wg.ar);
  }
  return 0;
}

// Same steps as polymul_prepared_kernel (bhat_rows == 1: its SHARED instantiation, whose registers are loaded once).
template <typename Sh, bool BC>
int polymul_prepared_emu(const HostTables& t, const u64* a, const u64* bhat, size_t bhat_rows, u64* c, size_t batch) {
  typedef typename Sh::E E;
  constexpr int LOGN = Sh::LOGN;
  typedef Policy<E, Sh::LAZY> Pol;
  typedef Stepper<E, LOGN, Sh::LPT, Pol, BC> S;
  typedef typename S::Cfg Cfg;
  const FusedProductSetup<E> su = fused_product_setup(h_make_arith<E>(t), BC, false);
  S wg{su.ar};
  const typename S::Table fwd(t, su.fwd), inv(t, su.inv);
  std::vector<typename S::Regs> xa(S::T), xb(S::T);
  auto load_bhat = [&](size_t row) {
    for (u32 tau = 0; tau < S::T; ++tau)
      for (int r = 0; r < Cfg::R; ++r) xb[tau].x[r] = (E)bhat[(row << LOGN) + Cfg::prep_idx(tau, (u32)r)];
  };
  if (bhat_rows == 1) load_bhat(0);
  for (size_t row = 0; row < batch; ++row) {
    const size_t off = row << LOGN;
    for (u32 tau = 0; tau < S::T; ++tau) {
      for (int r = 0; r < Cfg::R; ++r) xa[tau].x[r] = (E)a[off + Cfg::jidx(0, tau, r)];
      load_reduce<E, Cfg, Pol>(xa[tau].x, wg.ar);
    }
    if (bhat_rows != 1) load_bhat(row);
    wg.forward(xa, fwd);
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

// a == nullptr: prepare (in = b, out = bhat); otherwise the product.
int prepared_any(uint32_t n, uint64_t q, uint64_t psi, int flags, const u64* a, const u64* in, size_t in_rows, u64* out, size_t batch) {
  if (!params_ok(n, q, psi)) return 2;
  const HostTables t = h_build_tables(n, q, psi, !(flags & 1));
  return emu_with_shape(t, [&](auto sh, auto bc) {
    typedef decltype(sh) Sh;
    constexpr bool BC = decltype(bc)::value;
    return a ? polymul_prepared_emu<Sh, BC>(t, a, in, in_rows, out, batch) : prepare_emu<Sh, BC>(t, in, out, batch);
  });
}

}  // namespace

extern "C" {

// 0 ok, 2 bad params, 7 unsupported n.  Coefficients and prepared words travel as uint64 regardless of lane width.
// flags: bit 0 = canonical policy (TN_PLAN_FORCE_CANONICAL).
int emu_prepare(uint32_t n, uint64_t q, uint64_t psi, int flags, const uint64_t* b, uint64_t* bhat, size_t rows) {
  return prepared_any(n, q, psi, flags, nullptr, b, rows, bhat, rows);
}

// c[r] = a[r] * b[bhat_rows == 1 ? 0 : r]; 3: bhat_rows is neither 1 nor batch
int emu_poly_mult_prepared(uint32_t n, uint64_t q, uint64_t psi, int flags, const uint64_t* a, const uint64_t* bhat, size_t bhat_rows,
                           uint64_t* c, size_t batch) {
  if (bhat_rows != 1 && bhat_rows != batch) return 3;
  if (!a) return 3;
  return prepared_any(n, q, psi, flags, a, bhat, bhat_rows, c, batch);
}

}  // extern "C"
