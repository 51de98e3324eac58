// emu_gadget.cpp — TEST INFRASTRUCTURE: steps the gadget dot-product kernel (polydot_gadget_kernel: tiny_ntt_amd/csrc/kernels_gadget.hip)
// on the CPU, one emulated thread at a time, with the Stepper of emu_stepper.h, the headers the gfx950 kernel is compiled from,
// its canonicalise-and-digit functions (fused_core.h: gadget_canon, gadget_digit), its accumulate function (dot_accumulate) and
// the prepared-order index map (FusedCfg::prep_idx).  Shape and base case come from emu_with_shape, tables and constants from
// fused_product_setup (launch_plan.h), as in the launcher.  Part of tests/emu/_build/libemu.so; used by
// tests/test_gadget_emu.py and tests/test_gpu_gadget.py.
#include "emu_stepper.h"

namespace {

// Same steps as polydot_gadget_kernel: per output row the words of a are made canonical once (gadget_canon); every term is
// one gadget_term_step (emu_stepper.h) of one component; one inverse runs on the sum.
template <typename Sh, bool BC>
int polydot_gadget_emu(const HostTables& t, const u64* a, const u64* bhat, size_t bhat_sets, u64* c, size_t batch, size_t terms, u32 base_log,
                       bool balanced) {
  typedef typename Sh::E E;
  constexpr int LOGN = Sh::LOGN;
  typedef Policy<E, Sh::LAZY> Pol;
  typedef Stepper<E, LOGN, Sh::LPT, Pol, BC> S;
  typedef typename S::Cfg Cfg;
  const FusedProductSetup<E> su = fused_product_setup(h_make_arith<E>(t), BC, false);
  S wg{su.ar};
  const typename S::Table fwd(t, su.fwd), inv(t, su.inv);
  std::vector<typename S::Regs> xw(S::T), acc(S::T);
  std::vector<typename S::Regs>* const sum[1] = {&acc};
  std::vector<u32> carries(S::T);
  for (size_t row = 0; row < batch; ++row) {
    for (u32 tau = 0; tau < S::T; ++tau) {
      for (int r = 0; r < Cfg::R; ++r) {
        xw[tau].x[r] = gadget_canon<E, Pol>((E)a[(row << LOGN) + Cfg::jidx(0, tau, r)], wg.ar);
        acc[tau].x[r] = 0;
      }
      carries[tau] = 0;
    }
    for (size_t j = 0; j < terms; ++j) {
      const size_t boff = (bhat_sets == 1 ? 0 : row) * terms + j;
      gadget_term_step(wg, fwd, xw, carries, j, base_log, balanced, bhat, 1, &boff, sum);
    }
    wg.inverse(acc, inv);
    for (u32 tau = 0; tau < S::T; ++tau)
      for (int r = 0; r < Cfg::R; ++r) c[(row << LOGN) + Cfg::jidx(0, tau, r)] = acc[tau].x[r];
  }
  return 0;
}

// digits[i * terms + j] = digit j of word x[i]: the kernel's two functions in the kernel's order
template <typename E, bool LAZY>
void digit_words(const HostTables& t, const u64* x, u64* digits, size_t count, size_t terms, u32 base_log, bool balanced) {
  const Arith<E> ar = h_make_arith<E>(t);
  for (size_t i = 0; i < count; ++i) {
    const E xc = gadget_canon<E, Policy<E, LAZY>>((E)x[i], ar);
    u32 carry = 0;
    for (size_t j = 0; j < terms; ++j) digits[i * terms + j] = gadget_digit<E>(xc, (u32)j * base_log, base_log, balanced, carry, ar.q);
  }
}

}  // namespace

extern "C" {

// c[r] = sum_j digit_j(a[r]) * b[bhat_sets == 1 ? 0 : r][j].  0 ok, 2 bad params, 3 bad bhat_sets / a, 4 what the gadget calls
// refuse (terms, base_log, flags), 7 unsupported n.  Coefficients and prepared words travel as uint64 regardless of lane
// width.  canonical: the canonical policy (TN_PLAN_FORCE_CANONICAL).  flags: bit 0 = balanced digits (TN_GADGET_BALANCED).
int emu_poly_gadget_dot_prepared(uint32_t n, uint64_t q, uint64_t psi, int canonical, const uint64_t* a, const uint64_t* bhat, size_t bhat_sets,
                                 uint64_t* c, size_t batch, size_t terms, uint32_t base_log, uint32_t flags) {
  if (bhat_sets != 1 && bhat_sets != batch) return 3;
  if (!a) return 3;
  if (!params_ok(n, q, psi)) return 2;
  const HostTables t = h_build_tables(n, q, psi, !(canonical & 1));
  if (!gadget_ok(t, terms, base_log, flags)) return 4;
  const bool bal = (flags & 1u) != 0;
  return emu_with_shape(t, [&](auto sh, auto bc) {
    return polydot_gadget_emu<decltype(sh), decltype(bc)::value>(t, a, bhat, bhat_sets, c, batch, terms, base_log, bal);
  });
}

// digits[i][j] = gadget_digit(gadget_canon(x[i]), j) for j < terms, with the lane width, policy and constants of the plan
// (n, q, psi, canonical); x[i] is truncated to the lane.  Returns 0, 2 for bad params, 4 for what the gadget calls refuse;
// *lane_bytes / *lazy tell which instantiation ran.
int emu_gadget_digits(uint32_t n, uint64_t q, uint64_t psi, int canonical, const uint64_t* x, uint64_t* digits, size_t count, size_t terms,
                      uint32_t base_log, uint32_t flags, int* lane_bytes, int* lazy) {
  if (!params_ok(n, q, psi)) return 2;
  const HostTables t = h_build_tables(n, q, psi, !(canonical & 1));
  if (!gadget_ok(t, terms, base_log, flags)) return 4;
  if (lane_bytes) *lane_bytes = t.elem_bytes;
  if (lazy) *lazy = t.lazy ? 1 : 0;
  const bool bal = (flags & 1u) != 0;
  return with_lane_policy(t.elem_bytes, t.lazy, [&](auto e, auto lz) { digit_words<decltype(e), decltype(lz)::value>(t, x, digits, count, terms, base_log, bal); return 0; });
}

}  // extern "C"
