// emu_galois.cpp — TEST INFRASTRUCTURE: steps the two automorphism kernels (automorphism_kernel, automorphism_hat_kernel:
// tiny_ntt_amd/csrc/kernels_galois.hip) on the CPU with the header they are compiled from (csrc/galois_core.h): per tile of rows
// the staging half for every thread of the workgroup, then the gather half for every thread, on an LDS image of exactly the
// size the launcher asks for.  Also the index maps by themselves and the entry points' argument list (csrc/api_checks.h:
// check_automorphism) for the CPU.  Part of tests/emu/_build/libemu.so (tests/test_galois_emu.py,
// tests/test_gpu_galois.py); with -DEMU_SANITIZE_CASES its cases for tests/emu/sanitize_driver.cpp (make sanitize).
#include "emu_stepper.h"
#include "../../tiny_ntt_amd/csrc/galois_core.h"
#include <string>

namespace {

bool elements_ok(u32 logn, const uint32_t* galois, size_t count) {
  if (!galois || count < 1 || count > GALOIS_MAX) return false;
  for (size_t m = 0; m < count; ++m)
    if (!(galois[m] & 1u) || galois[m] >= (2u << logn)) return false;
  return true;
}

// The kernels' tile loop (galois_core.h: galois_tiles, galois_tile) as a grid of EMU_GRID workgroups runs it, one workgroup after
// the other, each with an image of its own.  stage(img, tile, tid), gather(img, tile, tid).
constexpr u32 EMU_GRID = 3;
template <typename E, typename Stage, typename Gather>
void step_tiles(u32 logn, size_t rows_total, u32 count, Stage&& stage, Gather&& gather) {
  const u32 tiles = galois_tiles((u32)rows_total, logn);
  for (u32 wg = 0; wg < EMU_GRID; ++wg) {
    std::vector<E> img(galois_tile_words(logn));            // the launcher's dynamic LDS: an access outside it is a fault here
    for (u32 tile = wg; tile < tiles; tile += EMU_GRID) {
      const GaloisTile t = galois_tile(tile, (u32)rows_total, logn, count);
      for (auto& v : img) v = (E)0xDEADBEEFu;               // what the previous tile left is not this tile's to read
      for (u32 tid = 0; tid < GALOIS_THREADS; ++tid) stage(img.data(), t, tid);
      for (u32 tid = 0; tid < GALOIS_THREADS; ++tid) gather(img.data(), t, tid);
    }
  }
}

template <typename E>
int automorphism_emu(u32 logn, u64 q, const u64* a, u64* out, size_t batch, const uint32_t* galois, size_t count) {
  const size_t n = (size_t)1 << logn;
  GaloisList gl = {};
  gl.count = (u32)count;
  for (size_t m = 0; m < count; ++m) gl.v[m] = galois_inverse(galois[m], logn);
  std::vector<E> in(a, a + batch * n), res(batch * count * n, (E)~(E)0);       // words of the lane: what the device buffers hold
  const typename TwOf<E>::type one = h_make_tw<E>(1, q);
  step_tiles<E>(logn, batch, gl.count,
                [&](E* img, const GaloisTile& t, u32 tid) { galois_stage<E, true>(in.data() + t.in_offset, img, t.words, tid, (E)q, one); },
                [&](E* img, const GaloisTile& t, u32 tid) { galois_gather<E>(img, res.data() + t.out_offset, t.words, logn, gl, (E)q, tid); });
  for (size_t i = 0; i < res.size(); ++i) out[i] = res[i];
  return 0;
}

template <typename Sh, bool BC>
int automorphism_hat_emu(const HostTables& t, const u64* xhat, u64* out, size_t rows, const uint32_t* galois, size_t count) {
  typedef typename Sh::E E;
  const u32 logn = t.logn, lpt = (u32)Sh::LPT;
  const size_t n = t.n;
  GaloisList gl = {};
  gl.count = (u32)count;
  for (size_t m = 0; m < count; ++m) gl.v[m] = galois[m];
  const Arith<E> ar = h_make_arith<E>(t);
  const std::vector<typename TwOf<E>::type> psi_pow = h_fused_table<E>(t.psi_pow, t);       // capi.cpp: upload_tw(..., fused = true)
  std::vector<typename TwOf<E>::type> ftab(BC ? galois_factor_records(logn) : 0);           // the kernel's LDS copy of the factor records
  if (BC) for (u32 tid = 0; tid < GALOIS_THREADS; ++tid) galois_stage_factors<E>(psi_pow.data(), ftab.data(), logn, tid);
  std::vector<E> in(xhat, xhat + rows * n), res(rows * count * n, (E)~(E)0);
  step_tiles<E>(logn, rows, gl.count,
                [&](E* img, const GaloisTile& t, u32 tid) { galois_stage<E, false>(in.data() + t.in_offset, img, t.words, tid, ar.q, ar.one); },
                [&](E* img, const GaloisTile& t, u32 tid) {
                  galois_gather_hat<E, BC>(img, res.data() + t.out_offset, t.words, logn, lpt, gl, ar, ftab.data(), tid);
                });
  for (size_t i = 0; i < res.size(); ++i) out[i] = res[i];
  return 0;
}

}  // namespace

extern "C" {

// out[r][m] = sigma_{galois[m]}(a[r]).  0 ok, 1 bad n / q, 4 what the entry point refuses of the elements.  Words travel as
// uint64 regardless of lane width (the lane is 32 bits for q < 2^31); every n >= 4, no psi: every kind of plan.
int emu_automorphism(uint32_t n, uint64_t q, const uint64_t* a, uint64_t* out, size_t batch, const uint32_t* galois, size_t count) {
  u32 logn = 0;
  while (((u32)1 << logn) < n) ++logn;
  if (n < 4 || ((u32)1 << logn) != n || n > 8192 || q < 2 || q >= ((u64)1 << 62)) return 1;
  if (!elements_ok(logn, galois, count)) return 4;
  return q < ((u64)1 << 31) ? automorphism_emu<u32>(logn, q, a, out, batch, galois, count) : automorphism_emu<u64>(logn, q, a, out, batch, galois, count);
}

// out[r][m] = the prepared form of sigma_{galois[m]} of the polynomial behind xhat[r].  0 ok, 2 bad params, 4 bad elements,
// 7 an n without fused kernels.  flags: bit 0 = canonical policy (TN_PLAN_FORCE_CANONICAL).  *base_case (may be NULL): 1 when
// the plan's prepared rows are in the base-case format.
int emu_automorphism_prepared(uint32_t n, uint64_t q, uint64_t psi, int flags, const uint64_t* xhat, uint64_t* out, size_t rows,
                              const uint32_t* galois, size_t count, int* base_case) {
  if (!params_ok(n, q, psi)) return 2;
  const HostTables t = h_build_tables(n, q, psi, !(flags & 1));
  if (!elements_ok(t.logn, galois, count)) return 4;
  return emu_with_shape(t, [&](auto sh, auto bc) {
    if (base_case) *base_case = decltype(bc)::value ? 1 : 0;
    return automorphism_hat_emu<decltype(sh), decltype(bc)::value>(t, xhat, out, rows, galois, count);
  });
}

// The maps alone.  Coefficients: the source index of destination d (bit 31 set: negated) for the element g.
uint32_t emu_galois_src(uint32_t logn, uint32_t g, uint32_t d) {
  bool negate;
  const u32 s = galois_src(d, galois_inverse(g, logn), logn, negate);
  return s | (negate ? 0x80000000u : 0u);
}
// Prepared rows: the source word of destination word `word`; *fexp: the exponent of psi of the base case's factor.
uint32_t emu_galois_hat_src(uint32_t logn, uint32_t lpt, int base_case, uint32_t g, uint32_t word, uint32_t* fexp) {
  u32 f = 0;
  const u32 s = base_case ? galois_hat_src<true>(word, g, logn, lpt, f) : galois_hat_src<false>(word, g, logn, lpt, f);
  if (fexp) *fexp = f;
  return s;
}
// ... for every destination of a row at once: src[n] (and fexp[n], may be NULL)
void emu_galois_src_row(uint32_t logn, uint32_t g, uint32_t* src) {
  for (u32 d = 0; d < (1u << logn); ++d) src[d] = emu_galois_src(logn, g, d);
}
void emu_galois_hat_src_row(uint32_t logn, uint32_t lpt, int base_case, uint32_t g, uint32_t* src, uint32_t* fexp) {
  for (u32 w = 0; w < (1u << logn); ++w) src[w] = emu_galois_hat_src(logn, lpt, base_case, g, w, fexp ? fexp + w : nullptr);
}
uint32_t emu_galois_lpt(uint32_t logn) { return (uint32_t)fused_lpt((int)logn); }
uint32_t emu_galois_tile_rows(uint32_t logn) { return galois_tile_rows(logn); }

// The argument checks of tn_automorphism_dev (prepared == 0) and tn_automorphism_prepared_dev (api_checks.h:
// check_automorphism, the list capi.cpp runs) on a plan view made of (n, elem_bytes, has_fused, omega_only, q); n == 0 is a
// NULL plan.  in / out are addresses that are never read; galois is a real host array or NULL.  Returns the status; *launch = 1
// when the call would go on to its launch; msg receives the text tn_last_error would give.
int emu_galois_api_check(uint32_t n, int elem_bytes, int has_fused, int omega_only, uint64_t q, int prepared, const void* in, const void* out,
                         size_t batch, const uint32_t* galois, size_t count, int* launch, char* msg, size_t msg_len) {
  ApiCheck k{ApiPlan{n, elem_bytes, has_fused != 0, omega_only != 0, q}, prepared ? "tn_automorphism_prepared_dev" : "tn_automorphism_dev"};
  return api_answer(k, check_automorphism(k, in, out, batch, galois, count, prepared != 0), launch, msg, msg_len);
}

}  // extern "C"

#ifdef EMU_SANITIZE_CASES
#include "sanitize_cases.h"
// The cases sanitize_driver.cpp runs (galois_cases): both kernels stepped over every tile shape (several rows per tile with a last
// tile that is not full, one row per tile) at both lane widths, the prepared kernel on every fused n = 256 .. 8192, both policies
// and the base case, every named element and a repeated one; then the argument list.  The coefficient results are compared
// with the definition written out here.  The prepared results are only checked to come back under sigma_{g^-1}: any invertible
// wrong permutation would pass that, so for the prepared kernel this program is a MEMORY-SAFETY run (every index inside the
// image, the factor table, the input and the output); that its words are right is tests/test_galois_emu.py's to show.
namespace {

uint64_t lcg = 88172645463325252ull;
uint64_t rnd() { lcg = lcg * 6364136223846793005ull + 1442695040888963407ull; return lcg; }

std::vector<uint32_t> elements(uint32_t n, size_t count) {
  const uint32_t named[] = {1, 3, 5, n - 1, n + 1, 2 * n - 1};
  std::vector<uint32_t> g;
  for (size_t m = 0; m < count; ++m) g.push_back(m < 6 ? named[m] : (uint32_t)(rnd() >> 40) % (2 * n) | 1u);
  if (count > 2) g[count - 1] = g[1];                                         // a repeated element
  return g;
}

void coefficient_cases(uint32_t n, uint64_t q) {
  const size_t rpp = emu_galois_tile_rows((uint32_t)__builtin_ctz(n));
  for (size_t batch : {(size_t)1, (size_t)3, 2 * rpp + 1})
    for (size_t count : {(size_t)1, (size_t)3, (size_t)16}) {
      const std::vector<uint32_t> g = elements(n, count);
      std::vector<uint64_t> a(batch * n), out(batch * count * n);
      for (auto& v : a) v = q < ((uint64_t)1 << 31) ? (rnd() >> 32) : rnd();    // any word of the lane
      a[0] = q; a[1] = 2 * q; a[2] = q - 1; a[3] = 0;
      expect(emu_automorphism(n, q, a.data(), out.data(), batch, g.data(), count) == 0, "coefficient kernel runs");
      bool same = true;
      for (size_t r = 0; r < batch; ++r)
        for (size_t m = 0; m < count; ++m)
          for (uint32_t i = 0; i < n; ++i) {                                  // the definition, scatter form
            const uint32_t t = (uint32_t)(((uint64_t)i * g[m]) % (2 * n));
            const uint64_t x = a[r * n + i] % q, want = t < n ? x : (q - x) % q;
            same = same && out[(r * count + m) * n + (t < n ? t : t - n)] == want;
          }
      expect(same, "coefficient stepping equals the definition");
    }
}

void prepared_cases(uint32_t n, uint64_t q, uint64_t psi) {
  const uint32_t logn = (uint32_t)__builtin_ctz(n);
  const int before = tally.failures;
  for (int canonical = 0; canonical < 2; ++canonical)
    for (size_t rows : {(size_t)1, (size_t)5})
      for (size_t count : {(size_t)1, (size_t)3}) {
        const std::vector<uint32_t> g = elements(n, count);
        std::vector<uint32_t> ginv;
        for (uint32_t x : g) ginv.push_back(galois_inverse(x, logn));
        std::vector<uint64_t> x(rows * n), y(rows * count * n), z(count * n);
        for (auto& v : x) v = rnd() % q;                                      // prepared rows hold canonical words
        expect(emu_automorphism_prepared(n, q, psi, canonical, x.data(), y.data(), rows, g.data(), count, nullptr) == 0, "prepared kernel runs");
        bool back = true;
        for (size_t r = 0; r < rows; ++r)
          for (size_t m = 0; m < count; ++m) {
            expect(emu_automorphism_prepared(n, q, psi, canonical, y.data() + (r * count + m) * n, z.data(), 1, ginv.data() + m, 1, nullptr) == 0, "inverse runs");
            for (uint32_t i = 0; i < n; ++i) back = back && z[i] == x[r * n + i];
          }
        expect(back, "sigma_g then sigma_{g^-1} gives the prepared row back");
      }
  std::printf("prepared n=%u q=%llu both policies: %s\n", n, (unsigned long long)q, tally.failures == before ? "ok" : "FAILED");
}

void api_cases() {
  const uint32_t n = 4;
  const uint64_t q = 7681;
  const uintptr_t row = n * 4, base = 1 << 20, far = (uintptr_t)1 << 40;
  auto at = [](uintptr_t x) { return reinterpret_cast<const void*>(x); };
  const uint32_t g3[] = {3, 5, 7}, even[] = {3, 4, 7}, big[] = {3, 5, 8};
  auto run = [&](uintptr_t in, uintptr_t out, size_t batch, const uint32_t* g, size_t count, int prepared = 0, int fused = 1) {
    int launch = -1;
    char msg[256];
    const int st = emu_galois_api_check(n, 4, fused, 0, q, prepared, at(in), at(out), batch, g, count, &launch, msg, sizeof msg);
    return st == TN_OK ? (launch ? 0 : -1) : st;
  };
  expect(run(base, far, 3, g3, 3) == 0, "ok");
  expect(run(base, far, 3, g3, 3, 1) == 0, "prepared ok");
  expect(run(base, far, 3, g3, 3, 1, 0) == TN_EUNSUPPORTED, "prepared call without fused kernels");
  expect(run(base, far, 3, g3, 3, 0, 0) == 0, "coefficient call without fused kernels");
  expect(run(base, far, 3, g3, 0) == TN_EINVAL, "count 0");
  expect(run(base, far, 3, g3, 17) == TN_EINVAL, "count 17");
  expect(run(base, far, 3, even, 3) == TN_EINVAL, "even element");
  expect(run(base, far, 3, big, 3) == TN_EINVAL, "element 2n");
  expect(run(base, far, 0, g3, 3) == -1, "batch 0 launches nothing");
  expect(run(4096, 4096, (size_t)1 << 30, g3, 2) == TN_EINVAL, "2^31 rows");
  expect(run(base, far, 3, nullptr, 3) == TN_EINVAL, "NULL galois");
  expect(run(0, far, 3, g3, 3) == TN_EINVAL, "NULL input");
  for (size_t batch = 1; batch <= 2; ++batch)
    for (size_t count = 1; count <= 3; ++count)
      for (long off = -8 * (long)row; off <= 4 * (long)row; off += (long)row / 2) {
        const uintptr_t out = base + off;
        const bool want = out < base + batch * row && base < out + batch * count * row;
        expect(run(base, out, batch, g3, count) == (want ? (int)TN_EINVAL : 0), "overlap is the intersection of the byte ranges");
      }
}

}  // namespace

void galois_cases() {
  const uint64_t q23 = 8380417, q60 = 1152921504606830593ull, psi4096 = 431606828070683274ull;
  for (uint32_t n : {4u, 8u, 64u, 256u, 1024u, 4096u, 8192u}) {
    coefficient_cases(n, q23);                                                // (no psi: the kernel needs n and q alone)
    coefficient_cases(n, q60);
  }
  for (uint32_t n = 256; n <= 4096; n *= 2) {
    prepared_cases(n, q60, h_powmod(psi4096, 4096 / n, q60));                 // n = 4096: the base case (lazy) and the complete form (canonical)
    prepared_cases(n, q23, h_powmod(283817, 4096 / n, q23));
  }
  prepared_cases(8192, q60, 458558429756866ull);                             // the largest image: 64 KiB
  prepared_cases(8192, 2147352577ull, 44302);                                // 2^31 - 131071 = 1 mod 16384
  api_cases();
}
#endif
