// emu_cmux.cpp — TEST INFRASTRUCTURE: steps the CMux rotation kernel (polydot_cmux_kernel: tiny_ntt_amd/csrc/kernels_cmux.hip) on
// the CPU, one emulated thread at a time, with the Stepper of emu_stepper.h and the headers the gfx950 kernel is compiled
// from (fused_core.h, cmux_core.h): the exponent masked to 2n; per input polynomial the rotated-minus-own words (cmux_word on
// the word at the masked rotated index and the thread's own word) and a carry mask of its own; per term (gadget_term_step) gadget_digit, ONE
// forward transform, component 0's product through dot_product_into and component 1's in place; two inverses; the add-in of
// a[row][o] (cmux_add_in).  Also the monomial product in plain C++ from the definition of include/tinyntt.h, and the two entry
// points' argument lists (csrc/api_checks.h: check_monomial, check_cmux_rotate) for the CPU.  Part of
// tests/emu/_build/libemu.so (tests/test_cmux_emu.py, tests/test_gpu_cmux.py); with -DEMU_SANITIZE_CASES its cases for
// tests/emu/sanitize_driver.cpp (make sanitize).
#include "emu_stepper.h"
#include "../../tiny_ntt_amd/csrc/cmux_core.h"
#include <string>

namespace {

// a, c: [batch][2][n]; exps: [batch]; bhat: [sets][2][2][terms][n]
template <typename Sh, bool BC>
int polydot_cmux_emu(const HostTables& t, const u64* a, const u32* exps, const u64* bhat, size_t bhat_sets, u64* c, size_t batch, size_t terms,
                     u32 base_log, bool balanced) {
  typedef typename Sh::E E;
  constexpr int LOGN = Sh::LOGN;
  typedef Policy<E, Sh::LAZY> Pol;
  typedef Stepper<E, LOGN, Sh::LPT, Pol, BC> S;
  typedef typename S::Cfg Cfg;
  constexpr u32 EMASK = 2u * (u32)Cfg::N - 1u;
  const FusedProductSetup<E> su = fused_product_setup(h_make_arith<E>(t), BC, false);
  S wg{su.ar};
  const typename S::Table fwd(t, su.fwd), inv(t, su.inv);
  std::vector<typename S::Regs> xw(S::T), acc0(S::T), acc1(S::T);
  std::vector<typename S::Regs>* const sums[2] = {&acc0, &acc1};
  std::vector<u32> carries(S::T);
  const size_t ins = 2, comp = ins * terms;                  // prepared rows of one component of a set
  for (size_t row = 0; row < batch; ++row) {
    const u32 e = exps[row] & EMASK;                          // the kernel's scalar
    for (u32 tau = 0; tau < S::T; ++tau)
      for (int r = 0; r < Cfg::R; ++r) { acc0[tau].x[r] = 0; acc1[tau].x[r] = 0; }      // once per output row
    const size_t set = (bhat_sets == 1 ? 0 : row) * 2 * comp;
    size_t term = 0;                                         // i * terms + j
    for (size_t i = 0; i < ins; ++i) {
      const u64* arow = a + ((row * ins + i) << LOGN);
      for (u32 tau = 0; tau < S::T; ++tau) {
        const u32 t0 = (tau - e) & EMASK;                    // request_words / put_away
        for (int r = 0; r < Cfg::R; ++r) {
          const u32 v = t0 + (u32)r * Cfg::THREADS;
          const E own = (E)arow[Cfg::jidx(0, tau, r)], rot = (E)arow[monomial_index(v, LOGN)];
          xw[tau].x[r] = cmux_word<E, Pol>(own, rot, monomial_negated(v, LOGN), wg.ar);
        }
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
      const u64* arow = a + ((row * 2 + o) << LOGN);         // read again for the add-in
      for (u32 tau = 0; tau < S::T; ++tau)
        for (int r = 0; r < Cfg::R; ++r) {
          const u32 j = Cfg::jidx(0, tau, r);
          c[((row * 2 + o) << LOGN) + j] = cmux_add_in<E, Pol>(acc[tau].x[r], (E)arow[j], wg.ar);
        }
    }
  }
  return 0;
}

}  // namespace

extern "C" {

// c[r][o] = a[r][o] + sum_{i < 2} sum_{j < terms} digit_j((X^e_r - 1) a[r][i]) * b[bhat_sets == 1 ? 0 : r][o][i][j], o < 2: the
// kernel's flow.  0 ok, 2 bad params, 3 bad bhat_sets / a / exps, 4 what the gadget calls refuse (terms, base_log, flags),
// 7 unsupported n.  Words travel as uint64 regardless of lane width.  canonical: the canonical policy
// (TN_PLAN_FORCE_CANONICAL).  flags: bit 0 = balanced digits.
int emu_poly_cmux_rotate_prepared(uint32_t n, uint64_t q, uint64_t psi, int canonical, const uint64_t* a, const uint32_t* exps, const uint64_t* bhat,
                                  size_t bhat_sets, uint64_t* c, size_t batch, size_t terms, uint32_t base_log, uint32_t flags) {
  if (bhat_sets != 1 && bhat_sets != batch) return 3;
  if (!a || !exps) return 3;
  if (!params_ok(n, q, psi)) return 2;
  const HostTables t = h_build_tables(n, q, psi, !(canonical & 1));
  if (!gadget_ok(t, terms, base_log, flags)) return 4;
  const bool bal = (flags & 1u) != 0;
  return emu_with_shape(t, [&](auto sh, auto bc) {
    return polydot_cmux_emu<decltype(sh), decltype(bc)::value>(t, a, exps, bhat, bhat_sets, c, batch, terms, base_log, bal);
  });
}

// tn_monomial_mul_dev in plain C++ from the definition (include/tinyntt.h): a, out [batch][group][n] of any words (below 2^64),
// exps [batch], flags bit 0 = TN_MONOMIAL_MINUS_ONE.  0 ok, 2 n not a power of two or q == 0, 3 a NULL argument or group == 0.
int emu_monomial_mul(uint32_t n, uint64_t q, const uint64_t* a, const uint32_t* exps, uint64_t* out, size_t batch, size_t group, uint32_t flags) {
  if (n == 0 || (n & (n - 1)) || q == 0) return 2;
  if (!a || !exps || !out || group == 0) return 3;
  for (size_t r = 0; r < batch; ++r) {
    const uint32_t e = exps[r] & (2 * n - 1);
    for (size_t g = 0; g < group; ++g) {
      const uint64_t* x = a + (r * group + g) * n;
      uint64_t* y = out + (r * group + g) * n;
      for (uint32_t t = 0; t < n; ++t) {
        const uint32_t s = (t - e) & (2 * n - 1);
        const uint64_t v = x[s < n ? s : s - n] % q;
        uint64_t rot = s < n ? v : (q - v) % q;
        if (flags & 1u) rot = (rot + (q - x[t] % q)) % q;      // q < 2^63: the sum fits
        y[t] = rot;
      }
    }
  }
  return 0;
}

// The argument checks of the two entry points (api_checks.h: check_monomial, check_cmux_rotate, the lists capi.cpp runs) on a
// plan view made of (n, elem_bytes, has_fused, omega_only, q); n == 0 is a NULL plan.  No pointer is read.  Returns the status;
// *launch = 1 when the call would go on to its launch; msg receives the text tn_last_error would give.
int emu_monomial_api_check(uint32_t n, int elem_bytes, int has_fused, int omega_only, uint64_t q, const void* a, const void* exps, const void* out,
                           size_t batch, size_t group, uint32_t flags, int* launch, char* msg, size_t msg_len) {
  ApiCheck k{ApiPlan{n, elem_bytes, has_fused != 0, omega_only != 0, q}, "tn_monomial_mul_dev"};
  return api_answer(k, check_monomial(k, a, exps, out, batch, group, flags), launch, msg, msg_len);
}

int emu_cmux_api_check(uint32_t n, int elem_bytes, int has_fused, int omega_only, uint64_t q, const void* a, const void* exps, const void* bhat,
                       const void* c, size_t sets, size_t batch, size_t comps, size_t terms, uint32_t base_log, uint32_t flags, int* launch, char* msg,
                       size_t msg_len) {
  ApiCheck k{ApiPlan{n, elem_bytes, has_fused != 0, omega_only != 0, q}, "tn_poly_cmux_rotate_prepared_dev"};
  return api_answer(k, check_cmux_rotate(k, a, exps, bhat, sets, c, batch, comps, terms, base_log, flags), launch, msg, msg_len);
}

}  // extern "C"

#ifdef EMU_SANITIZE_CASES
#include "sanitize_cases.h"
// The cases sanitize_driver.cpp runs (cmux_cases): the stepping at the smallest shape of either lane width and at the base-case
// shape, both policies, batch 5 x 2 terms, one shared set and one per row, both digit modes, with the exponents 0, 1, n,
// 2n - 1 and an unreduced one.  Two properties that need no second implementation of the transforms: with a key of zero rows
// the step returns a mod q; and the step is linear in the key, c(b) + c(b') - a = c(b + b') mod q (prepared rows add
// word-wise).  Then the monomial product against a second statement of the definition, and both argument lists on made-up
// addresses.
namespace {

void stepping_cases(uint32_t n, uint64_t q, uint64_t psi) {
  const size_t batch = 5, terms = 2;
  uint64_t lcg = 88172645463325252ull ^ q;
  auto rnd = [&]() { lcg = lcg * 6364136223846793005ull + 1442695040888963407ull; return lcg; };
  const uint32_t w = (uint32_t)((64 - __builtin_clzll(q)) + 1) / 2;
  const std::vector<uint32_t> exps = {0u, 1u, n, 2 * n - 1, 0x80000000u + 2 * n + 3};
  const size_t set = 4 * terms * n;
  std::vector<uint64_t> a(batch * 2 * n), b0(batch * set), b1(batch * set), b2(batch * set), zero(batch * set, 0);
  std::vector<uint64_t> c0(batch * 2 * n), c1(batch * 2 * n), c2(batch * 2 * n);
  for (auto& v : a) v = q < ((uint64_t)1 << 31) ? (rnd() >> 32) : rnd();       // any word of the lane
  for (size_t x = 0; x < b0.size(); ++x) { b0[x] = rnd() % q; b1[x] = rnd() % q; b2[x] = (uint64_t)(((unsigned __int128)b0[x] + b1[x]) % q); }
  a[0] = q - 1; a[1] = q; a[2] = 0;
  for (int canonical = 0; canonical < 2; ++canonical)
    for (size_t sets : {(size_t)1, batch})
      for (uint32_t flags = 0; flags < 2; ++flags) {
        expect(emu_poly_cmux_rotate_prepared(n, q, psi, canonical, a.data(), exps.data(), zero.data(), sets, c0.data(), batch, terms, w, flags) == 0, "runs");
        bool same = true;
        for (size_t x = 0; x < c0.size(); ++x) same = same && c0[x] == a[x] % q;
        expect(same, "a key of zero rows returns a mod q");
        expect(emu_poly_cmux_rotate_prepared(n, q, psi, canonical, a.data(), exps.data(), b0.data(), sets, c0.data(), batch, terms, w, flags) == 0, "runs");
        expect(emu_poly_cmux_rotate_prepared(n, q, psi, canonical, a.data(), exps.data(), b1.data(), sets, c1.data(), batch, terms, w, flags) == 0, "runs");
        expect(emu_poly_cmux_rotate_prepared(n, q, psi, canonical, a.data(), exps.data(), b2.data(), sets, c2.data(), batch, terms, w, flags) == 0, "runs");
        same = true;
        for (size_t x = 0; x < c0.size(); ++x) {
          const unsigned __int128 lhs = (unsigned __int128)c0[x] + c1[x] + (q - a[x] % q);
          same = same && c2[x] < q && (uint64_t)(lhs % q) == c2[x];
        }
        expect(same, "linear in the key");
        // exponent 0: (X^0 - 1) a = 0, so row 0 is a mod q whatever the key
        same = true;
        for (size_t x = 0; x < 2 * (size_t)n; ++x) same = same && c0[x] == a[x] % q;
        expect(same, "exponent 0 returns a mod q");
      }
}

void monomial_cases(uint32_t n, uint64_t q) {
  uint64_t lcg = 1234567ull ^ q;
  auto rnd = [&]() { lcg = lcg * 6364136223846793005ull + 1442695040888963407ull; return lcg; };
  const std::vector<uint32_t> exps = {0u, 1u, n, 2 * n - 1, 0xfffffff0u + 5};
  for (size_t group : {(size_t)1, (size_t)2}) {
    const size_t batch = exps.size();
    std::vector<uint64_t> a(batch * group * n), y(a.size()), z(a.size());
    for (auto& v : a) v = rnd();
    a[0] = 0; a[1] = q; a[2] = q - 1;
    expect(emu_monomial_mul(n, q, a.data(), exps.data(), y.data(), batch, group, 0) == 0, "monomial runs");
    expect(emu_monomial_mul(n, q, a.data(), exps.data(), z.data(), batch, group, 1) == 0, "monomial minus one runs");
    bool ok = true;
    for (size_t r = 0; r < batch; ++r)
      for (size_t g = 0; g < group; ++g)
        for (uint32_t i = 0; i < n; ++i) {             // scatter form: word i goes to (i + e) mod 2n
          const size_t row = (r * group + g) * n;
          const uint64_t e = exps[r] % (2 * (uint64_t)n), t = (i + e) % (2 * (uint64_t)n), v = a[row + i] % q;
          const uint64_t want = t < n ? v : (q - v) % q;
          const size_t at = row + (size_t)(t < n ? t : t - n);
          ok = ok && y[at] == want && y[at] < q;
          ok = ok && z[at] == (uint64_t)(((unsigned __int128)want + q - a[at] % q) % q);
        }
    expect(ok, "gather form equals scatter form");
  }
}

void api_cases() {
  const uint32_t n = 4;
  const uint64_t q = 7681;
  const uintptr_t row = n * 4, base = 1 << 20, far = (uintptr_t)1 << 40, ex = (uintptr_t)1 << 44;
  auto at = [](uintptr_t x) { return reinterpret_cast<const void*>(x); };
  auto run = [&](uintptr_t a, uintptr_t e, uintptr_t b, uintptr_t c, size_t sets, size_t batch, size_t comps, size_t terms, uint32_t w = 4, uint32_t flags = 0,
                 int fused = 1) {
    int launch = -1;
    char msg[256];
    const int st = emu_cmux_api_check(n, 4, fused, 0, q, at(a), at(e), at(b), at(c), sets, batch, comps, terms, w, flags, &launch, msg, sizeof msg);
    return st == TN_OK ? (launch ? 0 : -1) : st;
  };
  auto mono = [&](uintptr_t a, uintptr_t e, uintptr_t o, size_t batch, size_t group, uint32_t flags = 0) {
    int launch = -1;
    char msg[256];
    const int st = emu_monomial_api_check(n, 4, 0, 1, q, at(a), at(e), at(o), batch, group, flags, &launch, msg, sizeof msg);
    return st == TN_OK ? (launch ? 0 : -1) : st;
  };
  expect(run(base, ex, far, 2 * far, 1, 3, 2, 2) == 0, "ok");
  expect(run(base, ex, far, 2 * far, 3, 3, 2, 2) == 0, "a key per row ok");
  expect(run(base, ex, far, 2 * far, 1, 3, 0, 2) == TN_EINVAL, "comps 0");
  expect(run(base, ex, far, 2 * far, 1, 3, 1, 2) == TN_EUNSUPPORTED, "comps 1");
  expect(run(base, ex, far, 2 * far, 1, 3, 3, 2) == TN_EUNSUPPORTED, "comps 3");
  expect(run(base, ex, far, 2 * far, 1, 3, 2, 2, 4, 0, 0) == TN_EUNSUPPORTED, "no fused kernels");
  expect(run(base, ex, far, 2 * far, 1, 0, 2, 2) == -1, "batch 0 launches nothing");
  expect(run(base, 0, far, 2 * far, 1, 3, 2, 2) == TN_EINVAL, "NULL exps");
  expect(run(base, ex, far, 2 * far, 2, 3, 2, 2) == TN_EINVAL, "sets 2");
  expect(run(4096, 4096, 4096, 4096, 1, (size_t)1 << 28, 2, 2, 1) == TN_EINVAL, "2^31 rows");
  expect(run(4096, 4096, 4096, 4096, 1, ~(size_t)0 / 2 + 1, 2, 1, 1) == TN_EINVAL, "a batch whose double wraps");
  expect(mono(base, ex, far, 3, 2) == 0, "monomial ok on an omega-only plan");
  expect(mono(base, ex, far, 3, 2, 1) == 0, "monomial minus one ok");
  expect(mono(base, ex, far, 3, 0) == TN_EINVAL, "group 0");
  expect(mono(base, ex, far, 3, 2, 2) == TN_EINVAL, "flag 2");
  expect(mono(base, ex, far, (size_t)1 << 30, 2) == TN_EINVAL, "2^31 rows");
  expect(mono(base, ex, far, 0, 2) == -1, "batch 0 launches nothing");
  expect(mono(base, 0, far, 3, 2) == TN_EINVAL, "NULL exps");
  // byte by byte: c's batch * 2 rows against a's batch * 2 rows and against the set's 4 * terms rows; out against a
  for (size_t batch = 1; batch <= 2; ++batch)
    for (int which = 0; which < 3; ++which)
      for (long off = -5 * (long)row; off <= 13 * (long)row; off += (long)row / 2) {
        const size_t terms = 2, in_rows = which == 1 ? 4 * terms : batch * 2;
        const uintptr_t out = base + off;
        const bool want = out < base + in_rows * row && base < out + batch * 2 * row;
        const int st = which == 0 ? run(base, ex, far, out, 1, batch, 2, terms) : which == 1 ? run(far, ex, base, out, 1, batch, 2, terms) : mono(base, ex, out, batch, 2);
        expect(st == (want ? (int)TN_EINVAL : 0), "overlap is the intersection of the byte ranges");
      }
}

}  // namespace

void cmux_cases() {
  const uint64_t q60 = 1152921504606830593ull, psi4096 = 431606828070683274ull;
  stepping_cases(256, 8380417, 1239911);
  stepping_cases(256, q60, h_powmod(psi4096, 16, q60));
  stepping_cases(4096, q60, psi4096);
  monomial_cases(16, 8380417);
  monomial_cases(256, q60);
  api_cases();
}
#endif
