// emu_gadget2.cpp — TEST INFRASTRUCTURE: steps the two-component gadget kernel (polydot_gadget2_kernel:
// tiny_ntt_amd/csrc/kernels_gadget.hip) on the CPU, one emulated thread at a time, with the Stepper of emu_stepper.h and
// the headers the gfx950 kernel is compiled from: gadget_canon; per term (gadget_term_step) gadget_digit, ONE forward transform, component 0's
// product through dot_product_into (the digit row left as it is), component 1's through the gadget kernel's in-place product,
// two sums (dot_accumulate_one) and two inverses.  Also the new entry point's argument list (csrc/api_checks.h:
// check_gadget_multidot) for the CPU.  Part of tests/emu/_build/libemu.so (tests/test_gadget2_emu.py,
// tests/test_gpu_gadget2.py); with -DEMU_SANITIZE_CASES its cases for tests/emu/sanitize_driver.cpp (make sanitize).
#include "emu_stepper.h"
#include <string>

namespace {

// bhat: [sets][outs][terms][n]; c: [batch][outs][n].  outs == 1 is the gadget kernel's flow (one in-place product per term).
template <typename Sh, bool BC>
int polydot_gadget2_emu(const HostTables& t, const u64* a, const u64* bhat, size_t bhat_sets, u64* c, size_t batch, size_t outs, size_t terms,
                        u32 base_log, bool balanced) {
  typedef typename Sh::E E;
  constexpr int LOGN = Sh::LOGN;
  typedef Policy<E, Sh::LAZY> Pol;
  typedef Stepper<E, LOGN, Sh::LPT, Pol, BC> S;
  typedef typename S::Cfg Cfg;
  const FusedProductSetup<E> su = fused_product_setup(h_make_arith<E>(t), BC, false);
  S wg{su.ar};
  const typename S::Table fwd(t, su.fwd), inv(t, su.inv);
  std::vector<typename S::Regs> xw(S::T), acc0(S::T), acc1(S::T);
  std::vector<typename S::Regs>* const sums[2] = {&acc0, &acc1};
  std::vector<u32> carries(S::T);
  for (size_t row = 0; row < batch; ++row) {
    for (u32 tau = 0; tau < S::T; ++tau) {
      for (int r = 0; r < Cfg::R; ++r) {
        xw[tau].x[r] = gadget_canon<E, Pol>((E)a[(row << LOGN) + Cfg::jidx(0, tau, r)], wg.ar);
        acc0[tau].x[r] = 0;
        acc1[tau].x[r] = 0;
      }
      carries[tau] = 0;
    }
    const size_t set = (bhat_sets == 1 ? 0 : row) * outs * terms;
    for (size_t j = 0; j < terms; ++j) {
      const size_t boff[2] = {set + j, set + terms + j};
      gadget_term_step(wg, fwd, xw, carries, j, base_log, balanced, bhat, outs, boff, sums);
    }
    for (size_t o = 0; o < outs; ++o) {
      std::vector<typename S::Regs>& acc = *sums[o];
      wg.inverse(acc, inv);
      for (u32 tau = 0; tau < S::T; ++tau)
        for (int r = 0; r < Cfg::R; ++r) c[((row * outs + o) << LOGN) + Cfg::jidx(0, tau, r)] = acc[tau].x[r];
    }
  }
  return 0;
}

}  // namespace

extern "C" {

// c[r][o] = sum_j digit_j(a[r]) * b[bhat_sets == 1 ? 0 : r][o][j], o < outs (1 or 2).  0 ok, 2 bad params, 3 bad bhat_sets / a,
// 4 what the gadget calls refuse (terms, base_log, flags), 5 outs neither 1 nor 2, 7 unsupported n.  Words travel as uint64
// regardless of lane width.  canonical: the canonical policy (TN_PLAN_FORCE_CANONICAL).  flags: bit 0 = balanced digits.
int emu_poly_gadget_multidot_prepared(uint32_t n, uint64_t q, uint64_t psi, int canonical, const uint64_t* a, const uint64_t* bhat, size_t bhat_sets,
                                      uint64_t* c, size_t batch, size_t outs, size_t terms, uint32_t base_log, uint32_t flags) {
  if (bhat_sets != 1 && bhat_sets != batch) return 3;
  if (!a) return 3;
  if (outs != 1 && outs != 2) return 5;
  if (!params_ok(n, q, psi)) return 2;
  const HostTables t = h_build_tables(n, q, psi, !(canonical & 1));
  if (!gadget_ok(t, terms, base_log, flags)) return 4;
  const bool bal = (flags & 1u) != 0;
  return emu_with_shape(t, [&](auto sh, auto bc) {
    return polydot_gadget2_emu<decltype(sh), decltype(bc)::value>(t, a, bhat, bhat_sets, c, batch, outs, terms, base_log, bal);
  });
}

// The argument checks of tn_poly_gadget_multidot_prepared_dev (api_checks.h: check_gadget_multidot, the list capi.cpp runs) on
// a plan view made of (n, elem_bytes, has_fused, omega_only, q); n == 0 is a NULL plan.  No pointer is read.  Returns the
// status; *launch = 1 when the call would go on to its launch; msg receives the text tn_last_error would give.
int emu_gadget2_api_check(uint32_t n, int elem_bytes, int has_fused, int omega_only, uint64_t q, const void* a, const void* bhat, const void* c,
                          size_t sets, size_t batch, size_t outs, size_t terms, uint32_t base_log, uint32_t flags, int* launch, char* msg,
                          size_t msg_len) {
  ApiCheck k{ApiPlan{n, elem_bytes, has_fused != 0, omega_only != 0, q}, "tn_poly_gadget_multidot_prepared_dev"};
  return api_answer(k, check_gadget_multidot(k, a, bhat, sets, c, batch, outs, terms, base_log, flags), launch, msg, msg_len);
}

}  // extern "C"

#ifdef EMU_SANITIZE_CASES
#include "sanitize_cases.h"
// The cases sanitize_driver.cpp runs (gadget2_cases): the stepping at the smallest shape of either lane width and at the base-case
// shape, both policies, batch 2 x 2 terms, one shared set and one per row, both digit modes, each pair compared with the
// one-component stepping of its slices; then the argument list on made-up addresses.
namespace {

void stepping_cases(uint32_t n, uint64_t q, uint64_t psi) {
  const size_t batch = 2, terms = 2;
  uint64_t lcg = 88172645463325252ull ^ q;
  auto rnd = [&]() { lcg = lcg * 6364136223846793005ull + 1442695040888963407ull; return lcg; };
  std::vector<uint64_t> a(batch * n), bh(batch * 2 * terms * n), c2(batch * 2 * n), c1(batch * n), one(batch * terms * n);
  for (auto& v : a) v = q < ((uint64_t)1 << 31) ? (rnd() >> 32) : rnd();       // any word of the lane
  for (auto& v : bh) v = rnd() % q;                                          // prepared rows hold canonical words
  a[0] = q - 1; a[1] = q; a[2] = 0;
  const uint32_t w = (uint32_t)((64 - __builtin_clzll(q)) + 1) / 2;
  for (int canonical = 0; canonical < 2; ++canonical)
    for (size_t sets : {(size_t)1, batch})
      for (uint32_t flags = 0; flags < 2; ++flags) {
        expect(emu_poly_gadget_multidot_prepared(n, q, psi, canonical, a.data(), bh.data(), sets, c2.data(), batch, 2, terms, w, flags) == 0, "pair runs");
        for (size_t o = 0; o < 2; ++o) {
          for (size_t s = 0; s < sets; ++s)                                   // component o's rows of every set, as a set of the one-component call
            for (size_t i = 0; i < terms * n; ++i) one[s * terms * n + i] = bh[(s * 2 + o) * terms * n + i];
          expect(emu_poly_gadget_multidot_prepared(n, q, psi, canonical, a.data(), one.data(), sets, c1.data(), batch, 1, terms, w, flags) == 0, "one runs");
          bool same = true;
          for (size_t r = 0; r < batch; ++r)
            for (size_t i = 0; i < n; ++i) same = same && c2[(r * 2 + o) * n + i] == c1[r * n + i] && c1[r * n + i] < q;
          expect(same, "component equals the one-component stepping");
        }
      }
}

void api_cases() {
  const uint32_t n = 4;
  const uint64_t q = 7681;
  const uintptr_t row = n * 4, base = 1 << 20, far = (uintptr_t)1 << 40;
  auto at = [](uintptr_t x) { return reinterpret_cast<const void*>(x); };
  auto run = [&](uintptr_t a, uintptr_t b, uintptr_t c, size_t sets, size_t batch, size_t outs, size_t terms, uint32_t w = 4, uint32_t flags = 0, int fused = 1) {
    int launch = -1;
    char msg[256];
    const int st = emu_gadget2_api_check(n, 4, fused, 0, q, at(a), at(b), at(c), sets, batch, outs, terms, w, flags, &launch, msg, sizeof msg);
    return st == TN_OK ? (launch ? 0 : -1) : st;
  };
  expect(run(base, far, 2 * far, 1, 3, 2, 2) == 0, "ok");
  expect(run(base, far, 2 * far, 1, 3, 1, 2) == 0, "one component ok");
  expect(run(base, far, 2 * far, 1, 3, 0, 2) == TN_EINVAL, "outs 0");
  expect(run(base, far, 2 * far, 1, 3, 3, 2) == TN_EUNSUPPORTED, "outs 3");
  expect(run(base, far, 2 * far, 1, 3, 2, 2, 4, 0, 0) == TN_EUNSUPPORTED, "no fused kernels");
  expect(run(base, far, 2 * far, 1, 0, 2, 2) == -1, "batch 0 launches nothing");
  expect(run(4096, 4096, 4096, 1, (size_t)1 << 29, 2, 2, 1) == TN_EINVAL, "2^31 rows");
  expect(run(4096, 4096, 4096, 1, ~(size_t)0 / 2 + 1, 2, 1, 1) == TN_EINVAL, "a batch whose double wraps");
  // byte by byte: c's batch * outs rows against a's batch rows and against the set's sets * outs * terms rows
  for (size_t batch = 1; batch <= 2; ++batch)
    for (size_t terms = 1; terms <= 2; ++terms)
      for (int which = 0; which < 2; ++which)
        for (long off = -5 * (long)row; off <= 9 * (long)row; off += (long)row / 2) {
          const size_t in_rows = which == 0 ? batch : 2 * terms;
          const uintptr_t out = base + off;
          const bool want = out < base + in_rows * row && base < out + batch * 2 * row;
          const int st = which == 0 ? run(base, far, out, 1, batch, 2, terms) : run(far, base, out, 1, batch, 2, terms);
          expect(st == (want ? (int)TN_EINVAL : 0), "overlap is the intersection of the byte ranges");
        }
}

}  // namespace

void gadget2_cases() {
  const uint64_t q60 = 1152921504606830593ull, psi4096 = 431606828070683274ull;
  stepping_cases(256, 8380417, 1239911);
  stepping_cases(256, q60, h_powmod(psi4096, 16, q60));
  stepping_cases(4096, q60, psi4096);
  api_cases();
}
#endif
