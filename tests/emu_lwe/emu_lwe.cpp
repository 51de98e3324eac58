// emu_lwe.cpp — TEST INFRASTRUCTURE: steps the three LWE kernels (tiny_ntt_amd/csrc/kernels_lwe.hip: lwe_modswitch_kernel,
// lwe_sample_extract_kernel, lwe_keyswitch_kernel) on the CPU, tile by tile and one emulated thread at a time, with the header the
// gfx950 kernels are compiled from (lwe_core.h).  One emulated workgroup takes the tiles in turn, as a workgroup of the grid-stride
// loops does; every loop over the threads below ends where the kernel has a workgroup barrier, and the LDS images are arrays of the
// kernels' sizes.  The plan is (n, q) alone: the kernels read q and the `one` record of the plan's constants, nothing else.
// Also the three entry points' argument lists (csrc/api_checks.h) for the CPU.  A library of its own,
// tests/emu_lwe/_build/libemu_lwe.so (tests/test_lwe_emu.py, tests/test_lwe_api_emu.py, tests/test_gpu_lwe.py); with
// -DEMU_SANITIZE_CASES its cases for sanitize_lwe.cpp (make -C tests/emu_lwe sanitize).
#include "../emu/emu_stepper.h"
#include "../../tiny_ntt_amd/csrc/lwe_core.h"
#include <string>

namespace {

template <typename E> Arith<E> lwe_arith(u64 q) {
  Arith<E> ar = {};
  ar.q = (E)q;
  ar.one = h_lwe_tw(1 % q, q, (E)0);
  return ar;
}
template <typename E> std::vector<E> lane_words(const u64* x, size_t count) {      // words travel as uint64; a 32-bit lane sees the low half
  std::vector<E> v(count);
  for (size_t i = 0; i < count; ++i) v[i] = (E)x[i];
  return v;
}
bool plan_ok(u32 n, u64 q) { return n >= 4 && !(n & (n - 1)) && n <= 8192 && q >= 2 && q < ((u64)1 << 62); }
u32 log2_of(u32 n) { u32 l = 0; while ((1u << l) < n) ++l; return l; }
template <typename F> int with_lane(u64 q, F&& f) { return q < ((u64)1 << 31) ? f((u32)0) : f((u64)0); }

template <typename E> int modswitch_emu(u32 n, u64 q, const u64* lwe64, u32* exps, size_t batch, size_t dim) {
  const Arith<E> ar = lwe_arith<E>(q);
  const std::vector<E> lwe = lane_words<E>(lwe64, batch * (dim + 1));
  std::vector<u32> img(LWE_MS_IMAGE);
  const u32 tiles = lwe_ms_tiles((u32)batch, (u32)dim);
  for (u32 tile = 0; tile < tiles; ++tile) {
    const LweMsTile t = lwe_ms_tile(tile, (u32)batch, (u32)dim);
    for (u32 tid = 0; tid < LWE_THREADS; ++tid) lwe_ms_stage<E>(lwe.data(), img.data(), t, (u32)dim, tid, ar, log2_of(n));
    // ---- __syncthreads() ----
    for (u32 tid = 0; tid < LWE_THREADS; ++tid) lwe_ms_store(img.data(), exps, t, (u32)batch, tid);
    // ---- __syncthreads() ----
  }
  return 0;
}

template <typename E> int extract_emu(u32 n, u64 q, const u64* a64, u64* lwe64, size_t batch, u32 index) {
  const Arith<E> ar = lwe_arith<E>(q);
  const u32 logn = log2_of(n);
  const std::vector<E> a = lane_words<E>(a64, batch * 2 * n);
  std::vector<E> lwe(batch * ((size_t)n + 1)), img(galois_tile_words(logn));
  const u32 tiles = galois_tiles((u32)batch, logn);
  for (u32 tile = 0; tile < tiles; ++tile) {
    const GaloisTile t = galois_tile(tile, (u32)batch, logn, 1);
    for (u32 tid = 0; tid < LWE_THREADS; ++tid) lwe_extract_stage<E>(a.data(), img.data(), t.row0, t.words, logn, tid, ar);
    // ---- __syncthreads() ----
    for (u32 tid = 0; tid < LWE_THREADS; ++tid) lwe_extract_gather<E>(a.data(), img.data(), lwe.data(), t.row0, t.words, logn, index, tid, ar);
    // ---- __syncthreads() ----
  }
  for (size_t i = 0; i < lwe.size(); ++i) lwe64[i] = lwe[i];
  return 0;
}

template <typename E, bool BAL>
int keyswitch_emu(u64 q, const u64* lwe64, const u64* ksk64, u64* out64, size_t batch, size_t n_in, size_t n_out, size_t terms, u32 w) {
  const Arith<E> ar = lwe_arith<E>(q);
  const LweRed<E> red = h_lwe_red<E>(q);
  const size_t pitch = n_out + 1;
  const std::vector<E> lwe = lane_words<E>(lwe64, batch * (n_in + 1)), ksk = lane_words<E>(ksk64, n_in * terms * pitch);
  std::vector<E> out(batch * pitch);
  std::vector<u32> dig((size_t)LWE_KS_SLOTS * LWE_KS_ROWS);
  std::vector<LweAcc> acc((size_t)LWE_THREADS * LWE_KS_ROWS);
  const u32 tiles = lwe_ks_tiles((u32)batch, (u32)n_out), chunk = lwe_ks_chunk((u32)terms);
  for (u32 tile = 0; tile < tiles; ++tile) {
    const LweKsTile t = lwe_ks_tile(tile, (u32)batch);
    for (auto& s : acc) s = {0, 0};
    for (u32 i0 = 0; i0 < n_in; i0 += chunk) {
      const u32 len = (u32)n_in - i0 < chunk ? (u32)n_in - i0 : chunk;
      for (u32 tid = 0; tid < LWE_THREADS; ++tid) lwe_ks_cut<E>(lwe.data(), dig.data(), t, (u32)n_in, i0, len, (u32)terms, w, BAL, tid, ar);
      // ---- __syncthreads() ----
      for (u32 tid = 0; tid < LWE_THREADS; ++tid)
        if (t.col0 + tid <= n_out)
          lwe_ks_accumulate<E, BAL>(ksk.data() + t.col0 + tid, pitch, (size_t)i0 * terms, dig.data(), len * (u32)terms, &acc[(size_t)tid * LWE_KS_ROWS], ar);
      // ---- __syncthreads() ----
    }
    for (u32 tid = 0; tid < LWE_THREADS; ++tid)
      if (t.col0 + tid <= n_out)
        lwe_ks_finish<E>(lwe.data(), out.data(), t, (u32)n_in, (u32)n_out, t.col0 + tid, &acc[(size_t)tid * LWE_KS_ROWS], red, ar);
  }
  for (size_t i = 0; i < out.size(); ++i) out64[i] = out[i];
  return 0;
}

}  // namespace

extern "C" {

// The kernels' tile sizes, for the tests that choose shapes around them.
uint32_t emu_lwe_ks_rows(void) { return LWE_KS_ROWS; }
uint32_t emu_lwe_ks_cols(void) { return LWE_KS_COLS; }

// exps[i][r] = round(2n lwe[r][i] / q) mod 2n: lwe [batch][dim + 1] -> exps [dim + 1][batch].  0 ok, 2 a plan the library has not
// (n, q), 4 a dim or a word count the entry point refuses.  Words travel as uint64 regardless of lane width.
int emu_lwe_modswitch(uint32_t n, uint64_t q, const uint64_t* lwe, uint32_t* exps, size_t batch, size_t dim) {
  if (!plan_ok(n, q)) return 2;
  ApiCheck k{ApiPlan{n, q < ((u64)1 << 31) ? 4 : 8, false, false, q}, "emu"};
  if (!(k.lwe_dim(dim, "dim") && k.rows(batch, dim + 1, "batch * (dim + 1)", "words"))) return 4;
  return with_lane(q, [&](auto e) { return modswitch_emu<decltype(e)>(n, q, lwe, exps, batch, dim); });
}

// a [batch][2][n] -> lwe [batch][n + 1], coefficient `index`.  0 ok, 2 a plan the library has not, 4 index >= n.
int emu_sample_extract(uint32_t n, uint64_t q, const uint64_t* a, uint64_t* lwe, size_t batch, uint32_t index) {
  if (!plan_ok(n, q)) return 2;
  ApiCheck k{ApiPlan{n, q < ((u64)1 << 31) ? 4 : 8, false, false, q}, "emu"};
  if (!(k.lwe_index(index) && k.rows(batch, (size_t)n + 1, "batch * (n + 1)", "words"))) return 4;
  return with_lane(q, [&](auto e) { return extract_emu<decltype(e)>(n, q, a, lwe, batch, index); });
}

// out[r][k] = [k == n_out] b_r + sum_i sum_j digit_j(a_r[i]) ksk[i][j][k]: lwe [batch][n_in + 1], ksk [n_in][terms][n_out + 1],
// out [batch][n_out + 1].  0 ok, 2 a modulus the library has not, 4 what the entry point refuses.  flags: bit 0 = balanced digits.
int emu_lwe_keyswitch(uint64_t q, const uint64_t* lwe, const uint64_t* ksk, uint64_t* out, size_t batch, size_t n_in, size_t n_out, size_t terms,
                      uint32_t base_log, uint32_t flags) {
  if (!plan_ok(4, q)) return 2;
  ApiCheck k{ApiPlan{4, q < ((u64)1 << 31) ? 4 : 8, false, false, q}, "emu"};
  if (!(k.lwe_dim(n_in, "n_in") && k.lwe_dim(n_out, "n_out") && k.gadget(n_in, terms, base_log, flags, "n_in * terms", "key rows") &&
        k.lwe_digits(base_log) && k.lwe_sum(n_in, terms) && k.rows(batch, n_in + 1, "", "") && k.rows(batch, n_out + 1, "", "")))
    return 4;
  return with_lane(q, [&](auto e) {
    typedef decltype(e) E;
    return (flags & 1u) ? keyswitch_emu<E, true>(q, lwe, ksk, out, batch, n_in, n_out, terms, base_log)
                        : keyswitch_emu<E, false>(q, lwe, ksk, out, batch, n_in, n_out, terms, base_log);
  });
}

// The argument checks of the three entry points (api_checks.h, the lists capi.cpp runs) on a plan view made of (n, elem_bytes,
// has_fused, omega_only, q); n == 0 is a NULL plan.  No pointer is read.  Returns the status; *launch = 1 when the call would go
// on to its launch; msg receives the text tn_last_error would give.
int emu_lwe_modswitch_api_check(uint32_t n, int elem_bytes, int has_fused, int omega_only, uint64_t q, const void* lwe, const void* exps, size_t batch,
                                size_t dim, int* launch, char* msg, size_t msg_len) {
  ApiCheck k{ApiPlan{n, elem_bytes, has_fused != 0, omega_only != 0, q}, "tn_lwe_modswitch_dev"};
  return api_answer(k, check_lwe_modswitch(k, lwe, exps, batch, dim), launch, msg, msg_len);
}
int emu_sample_extract_api_check(uint32_t n, int elem_bytes, int has_fused, int omega_only, uint64_t q, const void* a, const void* lwe, size_t batch,
                                 uint32_t index, int* launch, char* msg, size_t msg_len) {
  ApiCheck k{ApiPlan{n, elem_bytes, has_fused != 0, omega_only != 0, q}, "tn_sample_extract_dev"};
  return api_answer(k, check_sample_extract(k, a, lwe, batch, index), launch, msg, msg_len);
}
int emu_lwe_keyswitch_api_check(uint32_t n, int elem_bytes, int has_fused, int omega_only, uint64_t q, const void* lwe, const void* ksk, const void* out,
                                size_t batch, size_t n_in, size_t n_out, size_t terms, uint32_t base_log, uint32_t flags, int* launch, char* msg,
                                size_t msg_len) {
  ApiCheck k{ApiPlan{n, elem_bytes, has_fused != 0, omega_only != 0, q}, "tn_lwe_keyswitch_dev"};
  return api_answer(k, check_lwe_keyswitch(k, lwe, ksk, out, batch, n_in, n_out, terms, base_log, flags), launch, msg, msg_len);
}

}  // extern "C"

#ifdef EMU_SANITIZE_CASES
#include "../emu/sanitize_cases.h"
// The cases sanitize_lwe.cpp runs (lwe_cases): the three steppings at either lane width on exactly sized buffers (the sanitizer
// sees every access past one), shapes with ragged tiles, against 128-bit host arithmetic written here; then the argument lists on
// made-up addresses.
void lwe_cases();
namespace {

typedef unsigned __int128 u128;

void stepping_cases(uint32_t n, uint64_t q) {
  uint64_t lcg = 88172645463325252ull ^ q;
  auto rnd = [&]() { lcg = lcg * 6364136223846793005ull + 1442695040888963407ull; return lcg; };
  auto word = [&]() { return q < ((uint64_t)1 << 31) ? (rnd() >> 32) : rnd(); };       // any word of the lane
  // modulus switch: tiles ragged on both sides
  for (size_t batch : {(size_t)1, (size_t)70})
    for (size_t dim : {(size_t)1, (size_t)64, (size_t)67}) {
      std::vector<uint64_t> lwe(batch * (dim + 1));
      for (auto& v : lwe) v = word();
      lwe[0] = q - 1;
      std::vector<uint32_t> exps((dim + 1) * batch);
      expect(emu_lwe_modswitch(n, q, lwe.data(), exps.data(), batch, dim) == 0, "modswitch runs");
      bool same = true;
      for (size_t r = 0; r < batch; ++r)
        for (size_t i = 0; i <= dim; ++i)
          same = same && exps[i * batch + r] == (uint32_t)((((u128)(lwe[r * (dim + 1) + i] % q) * (2 * n) + q / 2) / q) % (2 * n));
      expect(same, "modswitch equals the definition");
    }
  // sample extraction
  for (size_t batch : {(size_t)1, (size_t)5})
    for (uint32_t index : {0u, 1u, n / 2, n - 1}) {
      std::vector<uint64_t> a(batch * 2 * n), lwe(batch * (n + 1));
      for (auto& v : a) v = word();
      a[n] = 0; a[n + 1] = q;
      expect(emu_sample_extract(n, q, a.data(), lwe.data(), batch, index) == 0, "extract runs");
      bool same = true;
      for (size_t r = 0; r < batch; ++r) {
        const uint64_t* c0 = &a[r * 2 * n];
        const uint64_t* c1 = c0 + n;
        for (uint32_t i = 0; i < n; ++i) {
          const uint64_t x = i <= index ? c1[index - i] % q : (q - c1[n + index - i] % q) % q;
          same = same && lwe[r * (n + 1) + i] == x;
        }
        same = same && lwe[r * (n + 1) + n] == c0[index] % q;
      }
      expect(same, "extract equals the definition");
    }
  expect(emu_sample_extract(n, q, nullptr, nullptr, 1, n) == 4, "index n is refused");
  // key switch: a slab with a ragged tail, more rows than a tile, several passes of the digit slab
  const uint32_t bits = (uint32_t)(64 - __builtin_clzll(q));
  const uint32_t w = bits > 12 ? 7 : 3, terms = 3;
  for (uint32_t flags = 0; flags < 2; ++flags)
    for (size_t n_out : {(size_t)3, (size_t)LWE_KS_COLS}) {
      const size_t batch = LWE_KS_ROWS + 1, n_in = LWE_KS_SLOTS / terms + 5, pitch = n_out + 1;
      std::vector<uint64_t> lwe(batch * (n_in + 1)), ksk(n_in * terms * pitch), out(batch * pitch);
      for (auto& v : lwe) v = word();
      for (auto& v : ksk) v = word();
      expect(emu_lwe_keyswitch(q, lwe.data(), ksk.data(), out.data(), batch, n_in, n_out, terms, w, flags) == 0, "keyswitch runs");
      bool same = true;
      for (size_t r = 0; r < batch; ++r)
        for (size_t c = 0; c < pitch; ++c) {
          u128 sum = c == n_out ? lwe[r * (n_in + 1) + n_in] % q : 0;
          for (size_t i = 0; i < n_in; ++i) {
            const uint64_t x = lwe[r * (n_in + 1) + i] % q;
            uint64_t carry = 0;
            for (uint32_t j = 0; j < terms; ++j) {
              const uint64_t B = (uint64_t)1 << w, t = ((x >> (j * w)) & (B - 1)) + carry;
              const bool neg = flags && t >= B / 2;
              carry = neg ? 1 : 0;
              const uint64_t k = ksk[(i * terms + j) * pitch + c] % q;
              sum = (sum + (u128)(neg ? B - t : t) * (neg ? q - k : k)) % q;
            }
          }
          same = same && out[r * pitch + c] == (uint64_t)sum;
        }
      expect(same, "keyswitch equals the definition");
    }
}

void api_cases() {
  const uint32_t n = 4;
  const uint64_t q = 7681;
  const uintptr_t base = 1 << 20, far = (uintptr_t)1 << 40;
  auto at = [](uintptr_t x) { return reinterpret_cast<const void*>(x); };
  char msg[256];
  int launch = -1;
  auto ms = [&](uintptr_t lwe, uintptr_t exps, size_t batch, size_t dim, uint32_t plan_n = 4) {
    const int st = emu_lwe_modswitch_api_check(plan_n, 4, 0, 0, q, at(lwe), at(exps), batch, dim, &launch, msg, sizeof msg);
    return st == TN_OK ? (launch ? 0 : -1) : st;
  };
  auto se = [&](uintptr_t a, uintptr_t lwe, size_t batch, uint32_t index) {
    const int st = emu_sample_extract_api_check(n, 4, 0, 0, q, at(a), at(lwe), batch, index, &launch, msg, sizeof msg);
    return st == TN_OK ? (launch ? 0 : -1) : st;
  };
  auto ks = [&](uintptr_t lwe, uintptr_t ksk, uintptr_t out, size_t batch, size_t n_in, size_t n_out, size_t terms, uint32_t w = 4, uint32_t flags = 0,
                uint64_t q_ = 7681, int bytes = 4) {
    const int st = emu_lwe_keyswitch_api_check(n, bytes, 0, 0, q_, at(lwe), at(ksk), at(out), batch, n_in, n_out, terms, w, flags, &launch, msg, sizeof msg);
    return st == TN_OK ? (launch ? 0 : -1) : st;
  };
  expect(ms(base, far, 3, 5) == 0, "modswitch ok");
  expect(ms(base, far, 3, 5, 0) == TN_EINVAL, "modswitch NULL plan");
  expect(ms(base, far, 3, 0) == TN_EINVAL, "dim 0");
  expect(ms(base, far, 3, 65537) == TN_EINVAL, "dim above the maximum");
  expect(ms(base, far, (size_t)1 << 30, 1) == TN_EINVAL, "2^31 words");
  expect(ms(0, 0, 0, 5) == -1, "batch 0 launches nothing");
  expect(ms(0, far, 3, 5) == TN_EINVAL, "NULL lwe");
  expect(ms(base, base + 3 * 6 * 4 - 1, 3, 5) == TN_EINVAL, "exps over the last byte of lwe");
  expect(ms(base, base + 3 * 6 * 4, 3, 5) == 0, "exps just past lwe");
  expect(se(base, far, 3, 0) == 0 && se(base, far, 3, 3) == 0, "extract ok");
  expect(se(base, far, 3, 4) == TN_EINVAL, "index n");
  expect(se(base, far, 0, 4) == TN_EINVAL, "index n before batch 0");
  expect(se(0, 0, 0, 0) == -1, "extract batch 0");
  expect(se(base, 0, 3, 0) == TN_EINVAL, "NULL out");
  expect(se(base, base + 3 * 2 * 4 * 4 - 1, 3, 0) == TN_EINVAL && se(base, base + 3 * 2 * 4 * 4, 3, 0) == 0, "extract overlap");
  expect(ks(base, far, 2 * far, 3, 8, 5, 2) == 0, "keyswitch ok");
  expect(ks(base, far, 2 * far, 3, 0, 5, 2) == TN_EINVAL && ks(base, far, 2 * far, 3, 8, 65537, 2) == TN_EINVAL, "dimensions");
  expect(ks(base, far, 2 * far, 3, 8, 5, 0) == TN_EINVAL && ks(base, far, 2 * far, 3, 8, 5, 2, 4, 2) == TN_EINVAL, "terms 0, flag 2");
  expect(ks(base, far, 2 * far, 3, 8, 5, 2, 13) == TN_EINVAL, "2^base_log above q");
  expect(ks(base, far, 2 * far, 3, 8, 5, 1, 33, 0, (uint64_t)1 << 61, 8) == TN_EUNSUPPORTED, "base_log 33");
  expect(ks(base, far, 2 * far, 3, 8, 5, 1, 32, 0, (uint64_t)1 << 61, 8) == 0, "base_log 32");
  expect(ks(base, far, 2 * far, 3, 65536, 5, 64, 1) == 0 && ks(base, far, 2 * far, 3, 65536, 5, 65, 1) == TN_EINVAL, "2^22 terms fit");
  expect(ks(base, far, 2 * far, 3, 65536, 5, 33, 1) == 0 && ks(base, far, 2 * far, 3, 65535, 5, 65, 1) == TN_EINVAL, "shift rule first");
  expect(ks(base, far, 2 * far, (size_t)1 << 28, 8, 5, 2) == TN_EINVAL, "batch * (n_in + 1)");
  expect(ks(0, 0, 0, 0, 8, 5, 2) == -1, "keyswitch batch 0");
  expect(ks(base, 0, 2 * far, 3, 8, 5, 2) == TN_EINVAL, "NULL ksk");
  for (long off = -80; off <= 120; off += 2) {
    const uintptr_t out = base + off;
    const bool want_lwe = out < base + 3 * 9 * 4 && base < out + 3 * 6 * 4, want_ksk = out < base + 8 * 2 * 6 * 4 && base < out + 3 * 6 * 4;
    expect(ks(base, far, out, 3, 8, 5, 2) == (want_lwe ? (int)TN_EINVAL : 0), "out against lwe: the intersection of the byte ranges");
    expect(ks(far, base, out, 3, 8, 5, 2) == (want_ksk ? (int)TN_EINVAL : 0), "out against ksk: the intersection of the byte ranges");
  }
}

}  // namespace

void lwe_cases() {
  stepping_cases(4, 7681);
  stepping_cases(256, 8380417);
  stepping_cases(256, 1152921504606830593ull);
  stepping_cases(256, 4611686018427387904ull - 58);      // an even composite below 2^62: a general plan's modulus
  api_cases();
}
#endif
