// emu_dot.cpp — TEST INFRASTRUCTURE: steps the prepared dot-product kernel (polydot_prepared_kernel: tiny_ntt_amd/csrc/kernels_prepared.hip)
// on the CPU, one emulated thread at a time, with the Stepper of emu_stepper.h, the headers the gfx950 kernel is compiled from,
// its accumulate function (fused_core.h: dot_accumulate) and the prepared-order index map (FusedCfg::prep_idx).  Shape and base
// case come from emu_with_shape, tables and constants from fused_product_setup (launch_plan.h), as in the launcher.  Part of
// tests/emu/_build/libemu.so; used by tests/test_dot_emu.py and tests/test_gpu_dot.py.
#include "emu_stepper.h"

namespace {

// Same steps as polydot_prepared_kernel: per output row, every term runs load_reduce, one forward transform and the product
// against its prepared row, the products are summed by dot_accumulate and one inverse transform runs on the sum.
template <typename Sh, bool BC>
int polydot_prepared_emu(const HostTables& t, const u64* a, const u64* bhat, size_t bhat_sets, u64* c, size_t batch, size_t terms) {
  typedef typename Sh::E E;
  constexpr int LOGN = Sh::LOGN;
  typedef Policy<E, Sh::LAZY> Pol;
  typedef Stepper<E, LOGN, Sh::LPT, Pol, BC> S;
  typedef typename S::Cfg Cfg;
  const FusedProductSetup<E> su = fused_product_setup(h_make_arith<E>(t), BC, false);
  S wg{su.ar};
  const typename S::Table fwd(t, su.fwd), inv(t, su.inv);
  std::vector<typename S::Regs> xa(S::T), xb(S::T), acc(S::T);
  for (size_t row = 0; row < batch; ++row) {
    for (u32 tau = 0; tau < S::T; ++tau)
      for (int r = 0; r < Cfg::R; ++r) acc[tau].x[r] = 0;
    for (size_t j = 0; j < terms; ++j) {
      const size_t aoff = (row * terms + j) << LOGN, boff = ((bhat_sets == 1 ? 0 : row) * terms + j) << LOGN;
      for (u32 tau = 0; tau < S::T; ++tau) {
        for (int r = 0; r < Cfg::R; ++r) xa[tau].x[r] = (E)a[aoff + Cfg::jidx(0, tau, r)];
        load_reduce<E, Cfg, Pol>(xa[tau].x, wg.ar);
        for (int r = 0; r < Cfg::R; ++r) xb[tau].x[r] = (E)bhat[boff + Cfg::prep_idx(tau, (u32)r)];
      }
      wg.forward(xa, fwd);
      for (u32 tau = 0; tau < S::T; ++tau) {
        if constexpr (BC) basecase<Cfg, Pol>(xa[tau].x, xb[tau].x, wg.pre[tau].t + Cfg::pre_off(LOGN - 1), wg.ar);   // the zeta records came with the forward's
        else pointwise<E, Cfg, Pol>(xa[tau].x, xb[tau].x, wg.ar);
        dot_accumulate<E, Cfg, Pol>(acc[tau].x, xa[tau].x, wg.ar);
      }
    }
    wg.inverse(acc, inv);
    for (u32 tau = 0; tau < S::T; ++tau)
      for (int r = 0; r < Cfg::R; ++r) c[(row << LOGN) + Cfg::jidx(0, tau, r)] = acc[tau].x[r];
  }
  return 0;
}

template <typename E, bool LAZY>
void accumulate_words(const HostTables& t, const u64* acc, const u64* x, u64* out, size_t count) {
  const Arith<E> ar = h_make_arith<E>(t);
  for (size_t i = 0; i < count; ++i) out[i] = dot_accumulate_one<E, Policy<E, LAZY>>((E)acc[i], (E)x[i], ar);
}

}  // namespace

extern "C" {

// c[r] = sum_j a[r][j] * b[bhat_sets == 1 ? 0 : r][j].  0 ok, 2 bad params, 3 bad bhat_sets / terms / a, 7 unsupported n.
// Coefficients and prepared words travel as uint64 regardless of lane width.  canonical: the canonical policy
// (TN_PLAN_FORCE_CANONICAL).
int emu_poly_dot_prepared(uint32_t n, uint64_t q, uint64_t psi, int canonical, const uint64_t* a, const uint64_t* bhat, size_t bhat_sets,
                          uint64_t* c, size_t batch, size_t terms) {
  if (bhat_sets != 1 && bhat_sets != batch) return 3;
  if (!a || terms == 0) return 3;
  if (!params_ok(n, q, psi)) return 2;
  const HostTables t = h_build_tables(n, q, psi, !(canonical & 1));
  return emu_with_shape(t, [&](auto sh, auto bc) { return polydot_prepared_emu<decltype(sh), decltype(bc)::value>(t, a, bhat, bhat_sets, c, batch, terms); });
}

// out[i] = dot_accumulate_one(acc[i], x[i]) with the lane width, policy and constants of the plan (n, q, psi, canonical).
// Returns 0, or 2 for bad params; *lane_bytes / *lazy tell which instantiation ran.
int emu_dot_accumulate(uint32_t n, uint64_t q, uint64_t psi, int canonical, const uint64_t* acc, const uint64_t* x, uint64_t* out, size_t count,
                       int* lane_bytes, int* lazy) {
  if (!params_ok(n, q, psi)) return 2;
  const HostTables t = h_build_tables(n, q, psi, !(canonical & 1));
  if (lane_bytes) *lane_bytes = t.elem_bytes;
  if (lazy) *lazy = t.lazy ? 1 : 0;
  return with_lane_policy(t.elem_bytes, t.lazy, [&](auto e, auto lz) { accumulate_words<decltype(e), decltype(lz)::value>(t, acc, x, out, count); return 0; });
}

}  // extern "C"
