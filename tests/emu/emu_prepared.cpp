// emu_prepared.cpp — TEST INFRASTRUCTURE: steps the prepared-operand kernels (prepare_fused_kernel, polymul_prepared_kernel:
// tiny_ntt_amd/csrc/kernels_prepared.hip) on the CPU, one emulated thread at a time, with the Stepper of emu_kernels.cpp, the headers
// the gfx950 kernels are compiled from and the prepared-order index map the kernels use (FusedCfg::prep_idx).  Kernel
// variant, tables and constants come from fused_product_setup (launch_plan.h), as in the launchers.  Built into its own
// library by tests/emu/Makefile.prepared; loaded by tests/test_prepared_emu.py and tests/test_gpu_prepared.py.
#include "emu_kernels.cpp"

namespace {

// Same steps as prepare_fused_kernel, one emulated thread at a time; BC: the plan's product runs the base case.
template <typename E, int LOGN, int LPT, bool LAZY, bool BC>
int prepare_emu(const HostTables& t, const u64* b, u64* bhat, size_t rows) {
  typedef Policy<E, LAZY> Pol;
  typedef Stepper<E, LOGN, LPT, Pol, BC> S;
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
template <typename E, int LOGN, int LPT, bool LAZY, bool BC>
int polymul_prepared_emu(const HostTables& t, const u64* a, const u64* bhat, size_t bhat_rows, u64* c, size_t batch) {
  typedef Policy<E, LAZY> Pol;
  typedef Stepper<E, LOGN, LPT, Pol, BC> S;
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

// a == nullptr: prepare (in = b, out = bhat); otherwise the product.  The base case exactly where the launchers select it.
template <typename E, int LOGN, bool LAZY>
int prepared_shape(const HostTables& t, const u64* a, const u64* in, size_t in_rows, u64* out, size_t batch) {
  constexpr int LPT = fused_lpt(LOGN);
  if constexpr (fused_has_bc<E, LOGN, LPT, LAZY>()) {
    if (t.bc_ok) return a ? polymul_prepared_emu<E, LOGN, LPT, LAZY, true>(t, a, in, in_rows, out, batch) : prepare_emu<E, LOGN, LPT, LAZY, true>(t, in, out, batch);
  }
  return a ? polymul_prepared_emu<E, LOGN, LPT, LAZY, false>(t, a, in, in_rows, out, batch) : prepare_emu<E, LOGN, LPT, LAZY, false>(t, in, out, batch);
}

template <typename E, bool LAZY>
int prepared_dispatch(const HostTables& t, const u64* a, const u64* in, size_t in_rows, u64* out, size_t batch) {
  switch (t.logn) {
    case 8: return prepared_shape<E, 8, LAZY>(t, a, in, in_rows, out, batch);
    case 9: return prepared_shape<E, 9, LAZY>(t, a, in, in_rows, out, batch);
    case 10: return prepared_shape<E, 10, LAZY>(t, a, in, in_rows, out, batch);
    case 11: return prepared_shape<E, 11, LAZY>(t, a, in, in_rows, out, batch);
    case 12: return prepared_shape<E, 12, LAZY>(t, a, in, in_rows, out, batch);
    case 13: return prepared_shape<E, 13, LAZY>(t, a, in, in_rows, out, batch);
    default: return 7;
  }
}

int prepared_any(uint32_t n, uint64_t q, uint64_t psi, int flags, const u64* a, const u64* in, size_t in_rows, u64* out, size_t batch) {
  if (!params_ok(n, q, psi)) return 2;
  const HostTables t = h_build_tables(n, q, psi, !(flags & 1));
  if (t.elem_bytes == 8) return t.lazy ? prepared_dispatch<u64, true>(t, a, in, in_rows, out, batch) : prepared_dispatch<u64, false>(t, a, in, in_rows, out, batch);
  return t.lazy ? prepared_dispatch<u32, true>(t, a, in, in_rows, out, batch) : prepared_dispatch<u32, false>(t, a, in, in_rows, out, batch);
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
