// Test infrastructure: the CPU stepping of the kernels' per-thread code (every emu_*.cpp of this directory: the product's own
// headers compiled for the host) run under AddressSanitizer + UndefinedBehaviorSanitizer, one program with one tally.  The
// cases of the first five families are below; those of emu_gadget2, emu_galois, emu_extprod, emu_cmux and emu_blindrot stand
// in their sources (sanitize_cases.h) and are called from main, which prints one "<family>: N checks" line each.  GPU sanitizers are not available on the GPU pool, so this is where an
// out-of-bounds LDS image / table index or a shift by the word size in fused_core.h / cg_core.h / plan_tables.h would show:
// the prepared-order index map (prep_idx), the zeta-record LDS layout of basecase_each and the carry mask of gadget_digit included.
// Built and run by tests/test_emu.py::test_kernel_bodies_under_address_and_ub_sanitizers (tests/emu/Makefile: sanitize).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "sanitize_cases.h"

extern "C" {
int emu_fused_poly_mult(uint32_t n, uint64_t q, uint64_t psi, int flags, const uint64_t* a, const uint64_t* b, uint64_t* c, size_t batch);
int emu_fused_ntt(uint32_t n, uint64_t q, uint64_t psi, int force_canonical, int mode, const uint64_t* in, uint64_t* out);
int emu_cg(uint32_t n, uint64_t q, uint64_t psi, int mode, const uint64_t* a, const uint64_t* b, uint64_t* out, uint64_t* trace);
int emu_cgm(uint32_t n, uint64_t q, uint64_t psi, int mode, int group, int layout, int am, int flags, const uint64_t* a, const uint64_t* b,
            uint64_t* out, uint64_t* trace);
int bc_polymul(uint32_t n, uint64_t q, uint64_t psi, const uint64_t* a, const uint64_t* b, uint64_t* c, size_t batch, int cyclic);
int emu_prepare(uint32_t n, uint64_t q, uint64_t psi, int flags, const uint64_t* b, uint64_t* bhat, size_t rows);
int emu_poly_mult_prepared(uint32_t n, uint64_t q, uint64_t psi, int flags, const uint64_t* a, const uint64_t* bhat, size_t bhat_rows, uint64_t* c,
                           size_t batch);
int emu_poly_dot_prepared(uint32_t n, uint64_t q, uint64_t psi, int canonical, const uint64_t* a, const uint64_t* bhat, size_t bhat_sets, uint64_t* c,
                          size_t batch, size_t terms);
int emu_unprepare(uint32_t n, uint64_t q, uint64_t psi, int canonical, const uint64_t* xhat, uint64_t* x, size_t rows);
int emu_poly_dot_hat(uint32_t n, uint64_t q, uint64_t psi, int canonical, const uint64_t* ahat, const uint64_t* bhat, size_t bhat_sets, uint64_t* out,
                     size_t batch, size_t terms, int out_prepared);
int emu_poly_gadget_dot_prepared(uint32_t n, uint64_t q, uint64_t psi, int canonical, const uint64_t* a, const uint64_t* bhat, size_t bhat_sets,
                                 uint64_t* c, size_t batch, size_t terms, uint32_t base_log, uint32_t flags);
int emu_gadget_digits(uint32_t n, uint64_t q, uint64_t psi, int canonical, const uint64_t* x, uint64_t* digits, size_t count, size_t terms,
                      uint32_t base_log, uint32_t flags, int* lane_bytes, int* lazy);
int emu_api_check(const char* entry, uint32_t n, int elem_bytes, int has_fused, int omega_only, uint64_t q, const void* a, const void* b,
                  const void* out, size_t sets, size_t batch, size_t terms, int out_prepared, uint32_t base_log, uint32_t flags, int* launch,
                  char* msg, size_t msg_len);
}

namespace {
uint64_t lcg = 0x9E3779B97F4A7C15ull;
uint64_t next() { lcg = lcg * 6364136223846793005ull + 1442695040888963407ull; return lcg; }
uint64_t mulmod(uint64_t a, uint64_t b, uint64_t q) { return (uint64_t)(((unsigned __int128)a * b) % q); }
uint64_t powmod(uint64_t b, uint64_t e, uint64_t q) { uint64_t r = 1; b %= q; while (e) { if (e & 1) r = mulmod(r, b, q); b = mulmod(b, b, q); e >>= 1; } return r; }
void expect(bool ok, const char* what, unsigned n, int a, int b, int c, int d) {
  ++tally.checks;
  if (!ok) { ++tally.failures; std::fprintf(stderr, "MISMATCH %s n=%u (%d %d %d %d)\n", what, n, a, b, c, d); }
}
struct P { uint32_t n; uint64_t q, psi; };
typedef std::vector<uint64_t> Rows;

// The prepared-operand, dot-product, transform-domain and gadget steppings of one plan under both policies: batch 2, terms 2,
// one shared prepared set and one set per row, each result cross-checked against the stepping it is defined by.
void family_cases(const P& p) {
  const uint32_t n = p.n;
  const uint64_t q = p.q;
  const size_t batch = 2, terms = 2, rows = batch * terms;
  const bool narrow = q < (1ull << 32);
  Rows a(rows * n), b(rows * n);
  for (size_t i = 0; i < rows * n; ++i) { a[i] = next() >> (narrow ? 32 : 0); b[i] = next() >> (narrow ? 32 : 0); }      // any word of the lane
  a[0] = q - 1; b[0] = q - 1; a[1] = 0; b[n - 1] = ~0ull >> (narrow ? 32 : 0);
  auto row = [n](const Rows& v, size_t r) { return v.data() + r * n; };
  // references from the constant-geometry stepping: products of single rows and their sums mod q.  set 0: b shared, 1: per row
  auto product = [&](size_t ar, size_t br) {
    Rows c(n);
    const int rc = emu_cg(n, q, p.psi, 2, row(a, ar), row(b, br), c.data(), nullptr);
    expect(rc == 0, "emu_cg rc", n, rc, (int)ar, (int)br, 0);
    return c;
  };
  Rows prod[2] = {Rows(rows * n), Rows(rows * n)}, dot[2] = {Rows(batch * n), Rows(batch * n)};
  for (int per_row = 0; per_row < 2; ++per_row)
    for (size_t r = 0; r < batch; ++r) for (size_t j = 0; j < terms; ++j) {
      const Rows c = product(r * terms + j, per_row ? r * terms + j : j);
      for (uint32_t i = 0; i < n; ++i) {
        prod[per_row][(r * terms + j) * n + i] = c[i];
        uint64_t& s = dot[per_row][r * n + i];
        s = (uint64_t)(((unsigned __int128)s + c[i]) % q);
      }
    }
  const uint32_t base_log = narrow ? 12 : 30;              // two digits cover q: 2^base_log < q and 2 base_log >= bits of q
  for (int canon : {0, 1}) {
    Rows ahat(rows * n), bhat(rows * n), out(rows * n), x(rows * n);
    int r = emu_prepare(n, q, p.psi, canon, a.data(), ahat.data(), rows);
    r |= emu_prepare(n, q, p.psi, canon, b.data(), bhat.data(), rows);
    expect(r == 0, "prepare", n, canon, r, 0, 0);
    // hat: unprepare(prepare(x)) = x mod q
    r = emu_unprepare(n, q, p.psi, canon, ahat.data(), x.data(), rows);
    bool ok = r == 0;
    for (size_t i = 0; i < rows * n && ok; ++i) ok = x[i] == a[i] % q;
    expect(ok, "unprepare(prepare)", n, canon, r, 0, 0);
    for (int per_row = 0; per_row < 2; ++per_row) {
      const size_t sets = per_row ? batch : 1;
      // prepared: every product against b's prepared row(s).  Shared: ONE prepared row, so row j of the shared set is stepped
      // as its own call over the a-rows that meet it.
      if (per_row) {
        std::fill(out.begin(), out.end(), 0);
        r = emu_poly_mult_prepared(n, q, p.psi, canon, a.data(), bhat.data(), rows, out.data(), rows);
        expect(r == 0 && out == prod[1], "prepared product, a row each", n, canon, r, 0, 0);
      } else {
        for (size_t j = 0; j < terms; ++j) {
          Rows aj(batch * n), cj(batch * n), want(batch * n);
          for (size_t rr = 0; rr < batch; ++rr) {
            std::memcpy(aj.data() + rr * n, row(a, rr * terms + j), n * sizeof(uint64_t));
            std::memcpy(want.data() + rr * n, row(prod[0], rr * terms + j), n * sizeof(uint64_t));
          }
          r = emu_poly_mult_prepared(n, q, p.psi, canon, aj.data(), row(bhat, j), 1, cj.data(), batch);
          expect(r == 0 && cj == want, "prepared product, shared row", n, canon, r, (int)j, 0);
        }
      }
      // dot: the sum mod q of those products
      Rows c(batch * n), chat(batch * n), want_hat(batch * n);
      r = emu_poly_dot_prepared(n, q, p.psi, canon, a.data(), bhat.data(), sets, c.data(), batch, terms);
      expect(r == 0 && c == dot[per_row], "prepared dot product", n, canon, per_row, r, 0);
      // hat: the same from prepared operands, and left prepared
      std::fill(c.begin(), c.end(), 0);
      r = emu_poly_dot_hat(n, q, p.psi, canon, ahat.data(), bhat.data(), sets, c.data(), batch, terms, 0);
      expect(r == 0 && c == dot[per_row], "transform-domain dot product", n, canon, per_row, r, 0);
      r = emu_poly_dot_hat(n, q, p.psi, canon, ahat.data(), bhat.data(), sets, chat.data(), batch, terms, 1);
      r |= emu_prepare(n, q, p.psi, canon, dot[per_row].data(), want_hat.data(), batch);
      expect(r == 0 && chat == want_hat, "transform-domain dot product, prepared out", n, canon, per_row, r, 0);
      // gadget: the kernel that cuts the digits itself against the dot product on the rows of emu_gadget_digits
      for (uint32_t balanced : {0u, 1u}) {
        Rows words(batch * n), digits(batch * n * terms), drows(rows * n), want(batch * n), got(batch * n);
        for (size_t rr = 0; rr < batch; ++rr) std::memcpy(words.data() + rr * n, row(a, rr * terms), n * sizeof(uint64_t));
        r = emu_gadget_digits(n, q, p.psi, canon, words.data(), digits.data(), batch * n, terms, base_log, balanced, nullptr, nullptr);
        for (size_t rr = 0; rr < batch; ++rr) for (size_t j = 0; j < terms; ++j) for (uint32_t i = 0; i < n; ++i)
          drows[(rr * terms + j) * n + i] = digits[(rr * n + i) * terms + j];
        r |= emu_poly_dot_prepared(n, q, p.psi, canon, drows.data(), bhat.data(), sets, want.data(), batch, terms);
        const int r2 = emu_poly_gadget_dot_prepared(n, q, p.psi, canon, words.data(), bhat.data(), sets, got.data(), batch, terms, base_log, balanced);
        expect(r == 0 && r2 == 0 && got == want, "gadget dot product", n, canon, per_row, (int)balanced, r | r2);
      }
    }
  }
}

// The argument checks of the entry points (csrc/api_checks.h) on made-up addresses: the overlap rows of tests/api_cases.py as a
// sweep at the smallest plan (n = 4, 4-byte words) with the input 4 rows above address 8, against the intersection of the byte
// ranges counted byte by byte; and its row-limit rows, (3, 2^63) at address 4096 among them.  Address arithmetic that wraps or
// leaves the object a pointer came from would be reported here.
void api_check_cases() {
  const uint32_t n = 4;
  const uintptr_t row = n * 4, base = 4 * row + 8, far = (uintptr_t)1 << 40;
  auto at = [](uintptr_t x) { return (const void*)x; };
  auto meet = [](uintptr_t x, size_t xb, uintptr_t y, size_t yb) {
    for (uintptr_t i = x; i < x + xb; ++i) if (i >= y && i < y + yb) return true;
    return false;
  };
  struct Shape { const char* entry; int shared, out_terms, a_terms, b_terms; };      // rows = batch * (terms or 1); b_terms -1: no b
  const Shape shapes[] = {{"tn_poly_mult_dev", 0, 0, 0, 0}, {"tn_ntt_forward_dev", 0, 0, 0, -1}, {"tn_unprepare_dev", 0, 0, 0, -1},
                          {"tn_gadget_decompose_dev", 0, 1, 0, -1}, {"tn_poly_mult_prepared_dev", 0, 0, 0, 0}, {"tn_poly_mult_prepared_dev", 1, 0, 0, 0},
                          {"tn_poly_dot_prepared_dev", 0, 0, 1, 1}, {"tn_poly_dot_prepared_dev", 1, 0, 1, 1}, {"tn_poly_dot_hat_dev", 0, 0, 1, 1},
                          {"tn_poly_dot_hat_dev", 1, 0, 1, 1}, {"tn_poly_gadget_dot_prepared_dev", 0, 0, 0, 1}, {"tn_poly_gadget_dot_prepared_dev", 1, 0, 0, 1}};
  for (const Shape& sh : shapes)
    for (size_t batch = 1; batch <= 3; ++batch) for (size_t terms = 1; terms <= 3; ++terms) for (int which = 0; which < (sh.b_terms < 0 ? 1 : 2); ++which) {
      const size_t out_rows = batch * (sh.out_terms ? terms : 1);
      const bool mult = std::strcmp(sh.entry, "tn_poly_mult_prepared_dev") == 0;
      const size_t in_rows = which == 0 ? batch * (sh.a_terms ? terms : 1) : (sh.shared ? 1 : batch) * (sh.b_terms && !mult ? terms : 1);
      bool ok = true;
      for (int off = -4; off <= 7; ++off) {
        const uintptr_t out = base + (uintptr_t)((intptr_t)off * (intptr_t)row);
        int launch = -1;
        const int st = emu_api_check(sh.entry, n, 4, 1, 0, 7681, at(which == 0 ? base : far), at(which == 0 ? far : base), at(out), sh.shared ? 1 : batch, batch,
                                     terms, 0, 4, 0, &launch, nullptr, 0);
        const bool want = meet(out, out_rows * row, base, in_rows * row);
        ok = ok && st == (want ? 6 : 0) && launch == (want ? 0 : 1);
      }
      expect(ok, sh.entry, n, sh.shared, (int)batch, (int)terms, which);
    }
  const size_t M = (size_t)1 << 31;
  const size_t pairs[][2] = {{M - 2, 1}, {M - 1, 1}, {M, 1}, {1, M - 2}, {1, M - 1}, {1, M}, {(size_t)1 << 16, (size_t)1 << 15}, {(size_t)1 << 15, ((size_t)1 << 16) - 1},
                             {(size_t)1 << 30, 2}, {3, (size_t)1 << 63}};
  for (const char* entry : {"tn_poly_dot_prepared_dev", "tn_poly_dot_hat_dev"})
    for (const auto& pr : pairs) {
      const bool fits = pr[0] <= M - 1 && pr[1] <= M - 1 && pr[0] * pr[1] <= M - 1;          // (no wrap: both factors are below 2^31 here)
      const bool dummy = !fits;                                                              // refused rows: every pointer at address 4096
      const int st = emu_api_check(entry, n, 4, 1, 0, 7681, at(dummy ? 4096 : (uintptr_t)1 << 44), at(dummy ? 4096 : (uintptr_t)1 << 48),
                                   at(dummy ? 4096 : (uintptr_t)1 << 52), 1, pr[0], pr[1], 0, 0, 0, nullptr, nullptr, 0);
      expect(st == (fits ? 0 : 6), entry, n, (int)(pr[0] >> 16), (int)(pr[1] >> 16), st, 0);
    }
}
}  // namespace

Tally tally;

int main() {
  // psi of the full-size sets squared down to smaller n (psi^(N/n) is a primitive 2n-th root)
  const P base24 = {4096, 8380417ull, 283817ull}, base60 = {4096, 1152921504606830593ull, 431606828070683274ull};
  std::vector<P> sets;
  for (uint32_t n : {16u, 64u, 256u, 1024u, 4096u}) {
    sets.push_back({n, base24.q, powmod(base24.psi, base24.n / n, base24.q)});
    sets.push_back({n, base60.q, powmod(base60.psi, base60.n / n, base60.q)});
  }
  for (const P& p : sets) {
    const uint32_t n = p.n;
    std::vector<uint64_t> a(n), b(n), ref(n), out(n), t1(n), t2(n);
    for (uint32_t i = 0; i < n; ++i) { a[i] = next(); b[i] = next(); }            // any 64-bit word: the kernels reduce
    if (p.q < (1ull << 32)) for (uint32_t i = 0; i < n; ++i) { a[i] &= 0xffffffffull; b[i] &= 0xffffffffull; }
    a[0] = p.q - 1; b[0] = p.q - 1; a[1] = 0; b[n - 1] = ~0ull >> (p.q < (1ull << 32) ? 32 : 0);
    // reference for this row: the one-stage-per-trip constant-geometry stepping (mode 2 = nwc_poly_mult)
    const int rc = emu_cg(n, p.q, p.psi, 2, a.data(), b.data(), ref.data(), nullptr);
    expect(rc == 0, "emu_cg rc", n, rc, 0, 0, 0);
    if (n >= 256) {
      for (int flags : {0, 1}) {
        std::fill(out.begin(), out.end(), 0);
        const int r = emu_fused_poly_mult(n, p.q, p.psi, flags, a.data(), b.data(), out.data(), 1);
        expect(r == 0 && out == ref, "fused product", n, flags, r, 0, 0);
      }
      if (n == base60.n && p.q == base60.q) {                                      // the plan that runs the base-case product kernel
        std::fill(out.begin(), out.end(), 0);
        const int r = bc_polymul(n, p.q, p.psi, a.data(), b.data(), out.data(), 1, 0);
        expect(r == 0 && out == ref, "base-case product", n, r, 0, 0, 0);
      }
      for (int fc : {0, 1}) {
        int r = emu_fused_ntt(n, p.q, p.psi, fc, 1, a.data(), t1.data());
        r |= emu_fused_ntt(n, p.q, p.psi, fc, 2, t1.data(), t2.data());
        bool ok = r == 0;
        for (uint32_t i = 0; i < n && ok; ++i) ok = t2[i] == a[i] % p.q;
        expect(ok, "fused ntt round trip", n, fc, r, 0, 0);
        r = emu_fused_ntt(n, p.q, p.psi, fc, 0, a.data(), t1.data());
        expect(r == 0, "fused twisted ntt", n, fc, r, 0, 0);
      }
    }
    for (int group : {1, 2, 4, 8}) for (int layout : {0, 1, 2}) for (int am : {0, 1, 2, 3}) for (int flags : {0, 1, 3}) {
      std::fill(out.begin(), out.end(), 0);
      const int r = emu_cgm(n, p.q, p.psi, 2, group, layout, am, flags, a.data(), b.data(), out.data(), nullptr);
      if (r == 7) continue;                                                        // combination not built (e.g. split records on 32-bit lanes)
      expect(r == 0 && out == ref, "cg trips product", n, group, layout, am, flags);
      int r2 = emu_cgm(n, p.q, p.psi, 0, group, layout, am, flags, a.data(), nullptr, t1.data(), nullptr);
      r2 |= emu_cgm(n, p.q, p.psi, 1, group, layout, am, flags, t1.data(), nullptr, t2.data(), nullptr);
      bool ok = r2 == 0;
      for (uint32_t i = 0; i < n && ok; ++i) ok = t2[i] == a[i] % p.q;
      expect(ok, "cg trips ntt round trip", n, group, layout, am, flags);
      const int r3 = emu_cgm(n, p.q, p.psi, 3, group, layout, am, flags, a.data(), nullptr, t1.data(), nullptr);
      expect(r3 == 0, "cg trips twisted ntt", n, group, layout, am, flags);
      if (am <= 1) {                                                               // per-stage traces (canonical arithmetic)
        unsigned logn = 0; while ((1u << logn) < n) ++logn;
        std::vector<uint64_t> tr((size_t)logn * n);
        const int r4 = emu_cgm(n, p.q, p.psi, 0, group, layout, am, flags, a.data(), nullptr, t1.data(), tr.data());
        expect(r4 == 0, "cg trips trace", n, group, layout, am, flags);
      }
    }
  }
  // the four later families at their smallest shapes: 32-bit lanes, 64-bit lanes, and the one base-case shape
  for (const P& p : sets)
    if ((p.n == 256) || (p.n == base60.n && p.q == base60.q)) family_cases(p);
  api_check_cases();
  int counted = 0;
  auto family = [&](const char* name, void (*cases)()) {
    if (cases) cases();
    std::printf("%s: %d checks\n", name, tally.checks - counted);
    counted = tally.checks;
  };
  family("base", nullptr);                                                         // everything above
  family("gadget2", gadget2_cases);
  family("galois", galois_cases);
  family("extprod", extprod_cases);
  family("cmux", cmux_cases);
  family("blindrot", blindrot_cases);
  std::printf("sanitize_driver: %zu parameter sets, %d checks, %d failures\n", sets.size(), tally.checks, tally.failures);
  return tally.failures ? 1 : 0;
}
