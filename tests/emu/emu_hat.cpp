// emu_hat.cpp — TEST INFRASTRUCTURE: steps the transform-domain kernels (unprepare_fused_kernel, polydot_hat_kernel:
// tiny_ntt_amd/csrc/kernels_hat.hip) on the CPU, one emulated thread at a time, with the Stepper of emu_stepper.h, the headers the
// gfx950 kernels are compiled from, their product and accumulate functions (fused_core.h: pointwise, basecase_each,
// dot_accumulate) and the prepared-order index map (FusedCfg::prep_idx).  Shape and base case come from emu_with_shape, tables
// and constants from fused_product_setup (launch_plan.h), as in the launcher.  Part of tests/emu/_build/libemu.so; used by
// tests/test_hat_emu.py and tests/test_gpu_hat.py.
#include "emu_stepper.h"

namespace {

// Same steps as unprepare_fused_kernel: the R words at prep_idx are the last phase's registers; the inverse runs on them.
template <typename Sh, bool BC>
int unprepare_emu(const HostTables& t, const u64* xhat, u64* x, size_t rows) {
  typedef typename Sh::E E;
  constexpr int LOGN = Sh::LOGN;
  typedef Policy<E, Sh::LAZY> Pol;
  typedef Stepper<E, LOGN, Sh::LPT, Pol, BC> S;
  typedef typename S::Cfg Cfg;
  const FusedProductSetup<E> su = fused_product_setup(h_make_arith<E>(t), BC, false);
  S wg{su.ar};
  const typename S::Table inv(t, su.inv);
  std::vector<typename S::Regs> v(S::T);
  for (size_t row = 0; row < rows; ++row) {
    const size_t off = row << LOGN;
    for (u32 tau = 0; tau < S::T; ++tau)
      for (int r = 0; r < Cfg::R; ++r) v[tau].x[r] = (E)xhat[off + Cfg::prep_idx(tau, (u32)r)];
    wg.inverse(v, inv);
    for (u32 tau = 0; tau < S::T; ++tau)
      for (int r = 0; r < Cfg::R; ++r) x[off + Cfg::jidx(0, tau, r)] = v[tau].x[r];
  }
  return 0;
}

// Same steps as polydot_hat_kernel: per output row, every term loads its two prepared rows and runs the product, the products
// are summed as canonical residues; then one inverse transform and a natural-order store, or (out_prepared) the sum stored at
// prep_idx.  The zeta records of the base case are fetched once, from stage LOGN - 1 of the forward table, as in the kernel.
template <typename Sh, bool BC>
int polydot_hat_emu(const HostTables& t, const u64* ahat, const u64* bhat, size_t bhat_sets, u64* out, size_t batch, size_t terms, bool out_prepared) {
  typedef typename Sh::E E;
  constexpr int LOGN = Sh::LOGN;
  typedef Policy<E, Sh::LAZY> Pol;
  typedef Stepper<E, LOGN, Sh::LPT, Pol, BC> S;
  typedef typename S::Cfg Cfg;
  typedef typename S::Tw Tw;
  const FusedProductSetup<E> su = fused_product_setup(h_make_arith<E>(t), BC, false);
  S wg{su.ar};
  const typename S::Table fwd(t, su.fwd), inv(t, su.inv);
  std::vector<Tw> zeta((size_t)(Cfg::R / 2) * S::T);       // record i of thread tau at [i * T + tau], the kernel's LDS layout
  if constexpr (BC) {
    for (u32 tau = 0; tau < S::T; ++tau) {
      Tw zt[Cfg::NPRE];
      tw_prefetch_stages<E, Cfg, LOGN - 1, LOGN>(zt, tau, fwd.glob.data());
      for (int i = 0; i < Cfg::R / 2; ++i) zeta[(size_t)i * S::T + tau] = zt[Cfg::pre_off(LOGN - 1) + i];
    }
  }
  std::vector<typename S::Regs> xa(S::T), xb(S::T), acc(S::T);
  for (size_t row = 0; row < batch; ++row) {
    for (u32 tau = 0; tau < S::T; ++tau)
      for (int r = 0; r < Cfg::R; ++r) acc[tau].x[r] = 0;
    for (size_t j = 0; j < terms; ++j) {
      const size_t aoff = (row * terms + j) << LOGN, boff = ((bhat_sets == 1 ? 0 : row) * terms + j) << LOGN;
      for (u32 tau = 0; tau < S::T; ++tau) {
        for (int r = 0; r < Cfg::R; ++r) {
          xa[tau].x[r] = (E)ahat[aoff + Cfg::prep_idx(tau, (u32)r)];
          xb[tau].x[r] = (E)bhat[boff + Cfg::prep_idx(tau, (u32)r)];
        }
        if constexpr (BC) {
          E (&a_)[Cfg::R] = xa[tau].x;
          E (&s_)[Cfg::R] = acc[tau].x;
          basecase_each<Cfg, Pol, (int)S::T>(a_, xb[tau].x, zeta.data() + tau, wg.ar, [&](auto i_) {
            constexpr int r = 2 * decltype(i_)::value;
            s_[r] = dot_accumulate_one<E, Pol>(s_[r], a_[r], wg.ar);
            s_[r + 1] = dot_accumulate_one<E, Pol>(s_[r + 1], a_[r + 1], wg.ar);
          });
        } else {
          pointwise<E, Cfg, Pol>(xa[tau].x, xb[tau].x, wg.ar);
          dot_accumulate<E, Cfg, Pol>(acc[tau].x, xa[tau].x, wg.ar);
        }
      }
    }
    if (out_prepared) {
      for (u32 tau = 0; tau < S::T; ++tau)
        for (int r = 0; r < Cfg::R; ++r) out[(row << LOGN) + Cfg::prep_idx(tau, (u32)r)] = acc[tau].x[r];
      continue;
    }
    wg.inverse(acc, inv);
    for (u32 tau = 0; tau < S::T; ++tau)
      for (int r = 0; r < Cfg::R; ++r) out[(row << LOGN) + Cfg::jidx(0, tau, r)] = acc[tau].x[r];
  }
  return 0;
}

// bhat == nullptr: unprepare.
int hat_any(uint32_t n, uint64_t q, uint64_t psi, int canonical, const u64* in, const u64* bhat, size_t bhat_sets, u64* out, size_t batch, size_t terms,
            bool out_prepared) {
  if (!params_ok(n, q, psi)) return 2;
  const HostTables t = h_build_tables(n, q, psi, !(canonical & 1));
  return emu_with_shape(t, [&](auto sh, auto bc) {
    typedef decltype(sh) Sh;
    constexpr bool BC = decltype(bc)::value;
    return bhat ? polydot_hat_emu<Sh, BC>(t, in, bhat, bhat_sets, out, batch, terms, out_prepared) : unprepare_emu<Sh, BC>(t, in, out, batch);
  });
}

}  // namespace

extern "C" {

// x[r] = the polynomial whose prepared form is xhat[r].  0 ok, 2 bad params, 3 NULL buffer, 7 unsupported n.  Words travel as
// uint64 regardless of lane width.  canonical: the canonical policy (TN_PLAN_FORCE_CANONICAL).
int emu_unprepare(uint32_t n, uint64_t q, uint64_t psi, int canonical, const uint64_t* xhat, uint64_t* x, size_t rows) {
  if (!xhat || !x) return 3;
  return hat_any(n, q, psi, canonical, xhat, nullptr, 1, x, rows, 1, false);
}

// out[r] = sum_j a[r][j] * b[bhat_sets == 1 ? 0 : r][j], both operands prepared; out_prepared: out holds prepared words.
// 0 ok, 2 bad params, 3 bad bhat_sets / terms / out_prepared / NULL buffer, 7 unsupported n.
int emu_poly_dot_hat(uint32_t n, uint64_t q, uint64_t psi, int canonical, const uint64_t* ahat, const uint64_t* bhat, size_t bhat_sets, uint64_t* out,
                     size_t batch, size_t terms, int out_prepared) {
  if (bhat_sets != 1 && bhat_sets != batch) return 3;
  if (!ahat || !bhat || !out || terms == 0 || (out_prepared != 0 && out_prepared != 1)) return 3;
  return hat_any(n, q, psi, canonical, ahat, bhat, bhat_sets, out, batch, terms, out_prepared == 1);
}

}  // extern "C"
