// emu_extprod.cpp — TEST INFRASTRUCTURE: steps the external-product kernel (polydot_extprod_kernel:
// tiny_ntt_amd/csrc/kernels_extprod.hip) on the CPU, one emulated thread at a time, with the Stepper of emu_stepper.h and
// the headers the gfx950 kernel is compiled from: two sums cleared once per output row; per input polynomial gadget_canon and
// a carry mask of its own; per term (gadget_term_step) gadget_digit, ONE forward transform, component 0's product through dot_product_into (the
// digit row left as it is) and component 1's in place (dot_accumulate); two inverses behind the last term of the last input.
// Also the entry point's argument list (csrc/api_checks.h: check_external_product) for the CPU.  Part of
// tests/emu/_build/libemu.so (tests/test_extprod_emu.py, tests/test_gpu_extprod.py); with -DEMU_SANITIZE_CASES its cases for
// tests/emu/sanitize_driver.cpp (make sanitize).
#include "emu_stepper.h"
#include <string>

namespace {

// a: [batch][ins][n]; bhat: [sets][2][ins][terms][n]; c: [batch][2][n]
template <typename Sh, bool BC>
int polydot_extprod_emu(const HostTables& t, const u64* a, const u64* bhat, size_t bhat_sets, u64* c, size_t batch, size_t ins, size_t terms,
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
  const size_t comp = ins * terms;                           // prepared rows of one component of a set
  for (size_t row = 0; row < batch; ++row) {
    for (u32 tau = 0; tau < S::T; ++tau)
      for (int r = 0; r < Cfg::R; ++r) { acc0[tau].x[r] = 0; acc1[tau].x[r] = 0; }      // once per output row
    const size_t set = (bhat_sets == 1 ? 0 : row) * 2 * comp;
    size_t term = 0;                                         // i * terms + j
    for (size_t i = 0; i < ins; ++i) {
      for (u32 tau = 0; tau < S::T; ++tau) {
        for (int r = 0; r < Cfg::R; ++r) xw[tau].x[r] = gadget_canon<E, Pol>((E)a[((row * ins + i) << LOGN) + Cfg::jidx(0, tau, r)], wg.ar);
        carries[tau] = 0;                                    // carries never run from one polynomial into the next
      }
      for (size_t j = 0; j < terms; ++j, ++term) {
        const size_t boff[2] = {set + term, set + comp + term};
        gadget_term_step(wg, fwd, xw, carries, j, base_log, balanced, bhat, 2, boff, sums);
      }
    }
    for (size_t o = 0; o < 2; ++o) {
      std::vector<typename S::Regs>& acc = *sums[o];
      wg.inverse(acc, inv);
      for (u32 tau = 0; tau < S::T; ++tau)
        for (int r = 0; r < Cfg::R; ++r) c[((row * 2 + o) << LOGN) + Cfg::jidx(0, tau, r)] = acc[tau].x[r];
    }
  }
  return 0;
}

}  // namespace

extern "C" {

// c[r][o] = sum_{i < ins} sum_{j < terms} digit_j(a[r][i]) * b[bhat_sets == 1 ? 0 : r][o][i][j], o < 2: the kernel's flow, for
// any ins >= 1 (the entry point sends ins == 1 to the pair kernel, whose stepping is emu_gadget2.cpp).  0 ok, 2 bad params,
// 3 bad bhat_sets / a, 4 what the gadget calls refuse (terms, base_log, flags), 5 ins == 0, 7 unsupported n.  Words travel as
// uint64 regardless of lane width.  canonical: the canonical policy (TN_PLAN_FORCE_CANONICAL).  flags: bit 0 = balanced digits.
int emu_poly_external_product_prepared(uint32_t n, uint64_t q, uint64_t psi, int canonical, const uint64_t* a, const uint64_t* bhat, size_t bhat_sets,
                                       uint64_t* c, size_t batch, size_t ins, size_t terms, uint32_t base_log, uint32_t flags) {
  if (bhat_sets != 1 && bhat_sets != batch) return 3;
  if (!a) return 3;
  if (ins == 0) return 5;
  if (!params_ok(n, q, psi)) return 2;
  const HostTables t = h_build_tables(n, q, psi, !(canonical & 1));
  if (!gadget_ok(t, terms, base_log, flags)) return 4;
  const bool bal = (flags & 1u) != 0;
  return emu_with_shape(t, [&](auto sh, auto bc) {
    return polydot_extprod_emu<decltype(sh), decltype(bc)::value>(t, a, bhat, bhat_sets, c, batch, ins, terms, base_log, bal);
  });
}

// The argument checks of tn_poly_external_product_prepared_dev (api_checks.h: check_external_product, the list capi.cpp runs)
// on a plan view made of (n, elem_bytes, has_fused, omega_only, q); n == 0 is a NULL plan.  No pointer is read.  Returns the
// status; *launch = 1 when the call would go on to its launch; msg receives the text tn_last_error would give.
int emu_extprod_api_check(uint32_t n, int elem_bytes, int has_fused, int omega_only, uint64_t q, const void* a, const void* bhat, const void* c,
                          size_t sets, size_t batch, size_t ins, size_t outs, size_t terms, uint32_t base_log, uint32_t flags, int* launch,
                          char* msg, size_t msg_len) {
  ApiCheck k{ApiPlan{n, elem_bytes, has_fused != 0, omega_only != 0, q}, "tn_poly_external_product_prepared_dev"};
  return api_answer(k, check_external_product(k, a, bhat, sets, c, batch, ins, outs, terms, base_log, flags), launch, msg, msg_len);
}

}  // extern "C"

#ifdef EMU_SANITIZE_CASES
#include "sanitize_cases.h"
// The cases sanitize_driver.cpp runs (extprod_cases): the stepping at the smallest shape of either lane width and at the base-case
// shape, both policies, batch 2 x ins 2 and 3 x 2 terms, one shared set and one per row, both digit modes.  Each result is
// compared with the sum mod q of the steppings of the inputs taken one at a time (ins = 1 on input i's slice of the set: the
// products are linear in the sums, which stay canonical); then the argument list on made-up addresses.
namespace {

void stepping_cases(uint32_t n, uint64_t q, uint64_t psi) {
  const size_t batch = 2, terms = 2;
  uint64_t lcg = 88172645463325252ull ^ q;
  auto rnd = [&]() { lcg = lcg * 6364136223846793005ull + 1442695040888963407ull; return lcg; };
  const uint32_t w = (uint32_t)((64 - __builtin_clzll(q)) + 1) / 2;
  for (size_t ins : {(size_t)2, (size_t)3}) {
    std::vector<uint64_t> a(batch * ins * n), bh(batch * 2 * ins * terms * n), c(batch * 2 * n), sum(batch * 2 * n), c1(batch * 2 * n);
    std::vector<uint64_t> a1(batch * n), b1(batch * 2 * terms * n);
    for (auto& v : a) v = q < ((uint64_t)1 << 31) ? (rnd() >> 32) : rnd();       // any word of the lane
    for (auto& v : bh) v = rnd() % q;                                          // prepared rows hold canonical words
    a[0] = q - 1; a[1] = q; a[2] = 0;
    for (int canonical = 0; canonical < 2; ++canonical)
      for (size_t sets : {(size_t)1, batch})
        for (uint32_t flags = 0; flags < 2; ++flags) {
          expect(emu_poly_external_product_prepared(n, q, psi, canonical, a.data(), bh.data(), sets, c.data(), batch, ins, terms, w, flags) == 0, "runs");
          std::fill(sum.begin(), sum.end(), 0);
          for (size_t i = 0; i < ins; ++i) {
            for (size_t r = 0; r < batch; ++r)
              for (size_t x = 0; x < n; ++x) a1[r * n + x] = a[(r * ins + i) * n + x];
            for (size_t s = 0; s < sets; ++s)
              for (size_t o = 0; o < 2; ++o)
                for (size_t x = 0; x < terms * n; ++x) b1[((s * 2 + o) * terms) * n + x] = bh[(((s * 2 + o) * ins + i) * terms) * n + x];
            expect(emu_poly_external_product_prepared(n, q, psi, canonical, a1.data(), b1.data(), sets, c1.data(), batch, 1, terms, w, flags) == 0, "one input runs");
            for (size_t x = 0; x < sum.size(); ++x) sum[x] = (uint64_t)(((unsigned __int128)sum[x] + c1[x]) % q);
          }
          bool same = true;
          for (size_t x = 0; x < sum.size(); ++x) same = same && c[x] == sum[x] && c[x] < q;
          expect(same, "equals the sum over the inputs taken one at a time");
        }
  }
}

void api_cases() {
  const uint32_t n = 4;
  const uint64_t q = 7681;
  const uintptr_t row = n * 4, base = 1 << 20, far = (uintptr_t)1 << 40;
  auto at = [](uintptr_t x) { return reinterpret_cast<const void*>(x); };
  auto run = [&](uintptr_t a, uintptr_t b, uintptr_t c, size_t sets, size_t batch, size_t ins, size_t outs, size_t terms, uint32_t w = 4, uint32_t flags = 0,
                 int fused = 1) {
    int launch = -1;
    char msg[256];
    const int st = emu_extprod_api_check(n, 4, fused, 0, q, at(a), at(b), at(c), sets, batch, ins, outs, terms, w, flags, &launch, msg, sizeof msg);
    return st == TN_OK ? (launch ? 0 : -1) : st;
  };
  expect(run(base, far, 2 * far, 1, 3, 2, 2, 2) == 0, "ok");
  expect(run(base, far, 2 * far, 1, 3, 3, 2, 2) == 0, "three inputs ok");
  expect(run(base, far, 2 * far, 1, 3, 1, 1, 2) == 0, "one input, one component ok");
  expect(run(base, far, 2 * far, 1, 3, 1, 2, 2) == 0, "one input, two components ok");
  expect(run(base, far, 2 * far, 1, 3, 0, 2, 2) == TN_EINVAL, "ins 0");
  expect(run(base, far, 2 * far, 1, 3, 2, 0, 2) == TN_EINVAL, "outs 0");
  expect(run(base, far, 2 * far, 1, 3, 2, 3, 2) == TN_EUNSUPPORTED, "outs 3");
  expect(run(base, far, 2 * far, 1, 3, 2, 1, 2) == TN_EUNSUPPORTED, "two inputs into one component");
  expect(run(base, far, 2 * far, 1, 3, 2, 2, 2, 4, 0, 0) == TN_EUNSUPPORTED, "no fused kernels");
  expect(run(base, far, 2 * far, 1, 0, 2, 2, 2) == -1, "batch 0 launches nothing");
  expect(run(4096, 4096, 4096, 1, (size_t)1 << 28, 2, 2, 2, 1) == TN_EINVAL, "2^31 rows");
  expect(run(4096, 4096, 4096, 1, ~(size_t)0 / 2 + 1, 2, 2, 1, 1) == TN_EINVAL, "a batch whose double wraps");
  expect(run(4096, 4096, 4096, 1, 2, ~(size_t)0 / 4 + 1, 2, 1, 1) == TN_EINVAL, "an input count whose product with batch * outs wraps");
  // byte by byte: c's batch * 2 rows against a's batch * ins rows and against the set's 2 * ins * terms rows
  for (size_t batch = 1; batch <= 2; ++batch)
    for (size_t ins = 2; ins <= 3; ++ins)
      for (int which = 0; which < 2; ++which)
        for (long off = -5 * (long)row; off <= 13 * (long)row; off += (long)row / 2) {
          const size_t terms = 2, in_rows = which == 0 ? batch * ins : 2 * ins * terms;
          const uintptr_t out = base + off;
          const bool want = out < base + in_rows * row && base < out + batch * 2 * row;
          const int st = which == 0 ? run(base, far, out, 1, batch, ins, 2, terms) : run(far, base, out, 1, batch, ins, 2, terms);
          expect(st == (want ? (int)TN_EINVAL : 0), "overlap is the intersection of the byte ranges");
        }
}

}  // namespace

void extprod_cases() {
  const uint64_t q60 = 1152921504606830593ull, psi4096 = 431606828070683274ull;
  stepping_cases(256, 8380417, 1239911);
  stepping_cases(256, q60, h_powmod(psi4096, 16, q60));
  stepping_cases(4096, q60, psi4096);
  api_cases();
}
#endif
