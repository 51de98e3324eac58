// emu_lwe_mfma.cpp — TEST INFRASTRUCTURE: steps the two kernels of the matrix-core key switch
// (tiny_ntt_amd/csrc/kernels_lwe_mfma.hip: lwe_ksk_prepare_kernel, lwe_keyswitch_mfma_kernel) on the CPU, tile by tile and wave by
// wave, with the header the gfx950 kernels are compiled from (lwe_mfma_core.h).  One emulated workgroup takes the tiles in turn;
// every loop over the threads below ends where the kernel has a workgroup barrier; the LDS images are arrays of the kernels'
// sizes; the matrix step is the header's host loop over the lane -> element map (lwe_mfma_step_wave), which
// tests/test_gpu_lwe_mfma.py checks against the instruction itself.  Also the three entry points' argument lists
// (csrc/api_checks.h).  A library of its own, tests/emu_lwe_mfma/_build/libemu_lwe_mfma.so (tests/test_lwe_mfma_emu.py,
// tests/test_lwe_mfma_api_emu.py, tests/test_gpu_lwe_mfma.py); with -DEMU_SANITIZE_CASES its cases for sanitize_lwe_mfma.cpp
// (make -C tests/emu_lwe_mfma sanitize).
#include "../emu/emu_stepper.h"
#include "../../tiny_ntt_amd/csrc/lwe_mfma_core.h"
#include <string>
#include <cstring>

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
bool modulus_ok(u64 q) { return q >= 2 && q < ((u64)1 << 62); }
template <typename F> int with_lane(u64 q, F&& f) { return q < ((u64)1 << 31) ? f((u32)0) : f((u64)0); }

// an LDS image or a device buffer of bytes at the alignment the kernels rely on
struct Bytes {
  std::vector<LweFrag> store;
  explicit Bytes(size_t bytes) : store((bytes + 15) / 16) {}
  signed char* data() { return reinterpret_cast<signed char*>(store.data()); }
};

template <typename E> int prepare_emu(u64 q, const u64* ksk64, signed char* kprep, size_t n_in, size_t n_out, size_t terms) {
  const Arith<E> ar = lwe_arith<E>(q);
  const u32 slots = (u32)(n_in * terms), limbs = lwe_mfma_limbs(q);
  const std::vector<E> ksk = lane_words<E>(ksk64, (size_t)slots * (n_out + 1));
  Bytes img(LWE_MFMA_PREP_IMAGE);
  const u32 steps = (u32)lwe_mfma_steps(slots, 1), cts = (u32)lwe_mfma_col_tiles(n_out), tiles = lwe_mfma_prep_tiles(steps, cts);
  for (u32 tile = 0; tile < tiles; ++tile) {
    const LwePrepTile t = lwe_mfma_prep_tile(tile, steps);
    for (u32 tid = 0; tid < LWE_THREADS; ++tid) lwe_mfma_prep_stage<E>(ksk.data(), img.data(), t, slots, (u32)n_out, limbs, tid, ar);
    // ---- __syncthreads() ----
    for (u32 tid = 0; tid < LWE_THREADS; ++tid) lwe_mfma_prep_store(img.data(), kprep, t, steps, cts, limbs, tid);
    // ---- __syncthreads() ----
  }
  return 0;
}

// the kernel's tile loop; L is the kernel's template parameter, a run-time count here (lwe_mfma_fold's loop bound is all it is)
template <typename E, u32 L>
int keyswitch_emu_l(u64 q, const u64* lwe64, const signed char* kprep, u64* out64, size_t batch, size_t n_in_, size_t n_out_, size_t terms_, u32 w,
                    bool balanced) {
  const Arith<E> ar = lwe_arith<E>(q);
  const LweRed<E> red = h_lwe_red<E>(q);
  const LweAcc offset = h_lwe_mfma_offset(q, (int)sizeof(E));
  const u32 n_in = (u32)n_in_, n_out = (u32)n_out_, terms = (u32)terms_;
  const std::vector<E> lwe = lane_words<E>(lwe64, batch * ((size_t)n_in + 1));
  std::vector<E> out(batch * ((size_t)n_out + 1));
  Bytes img(LWE_MFMA_IMAGE);
  const u32 slots = n_in * terms, steps = (u32)lwe_mfma_steps(slots, 1), cts = (u32)lwe_mfma_col_tiles(n_out);
  const u32 tiles = lwe_mfma_tiles((u32)batch, n_out);
  struct Lane { LweTile acc[LWE_MFMA_ROW_TILES][L]; LweAcc wide[LWE_MFMA_ROW_TILES][4]; };
  std::vector<Lane> regs((size_t)LWE_THREADS);
  for (u32 tile = 0; tile < tiles; ++tile) {
    const LweMfmaTile t = lwe_mfma_tile(tile, (u32)batch);
    const u32 rts = (t.rows + 15) / 16;
    std::memset(regs.data(), 0, regs.size() * sizeof(Lane));
    u32 chunks = 0;
    for (u32 k0 = 0; k0 < slots; k0 += LWE_MFMA_CHUNK) {
      for (u32 tid = 0; tid < LWE_THREADS; ++tid) lwe_mfma_cut<E>(lwe.data(), img.data(), t, n_in, slots, k0, terms, w, balanced, tid, ar);
      // ---- __syncthreads() ----
      ++chunks;
      for (u32 wave = 0; wave < LWE_MFMA_WAVES; ++wave) {
        const u32 ct = t.ct0 + wave;
        if (ct >= cts) continue;
        Lane* lanes = &regs[(size_t)wave * LWE_MFMA_LANES];
        const u32 cs = lwe_mfma_chunk_steps(slots, k0), step0 = k0 / LWE_MFMA_K_STEP;
        for (u32 s = 0; s < cs; ++s) {
          LweFrag a[LWE_MFMA_ROW_TILES][LWE_MFMA_LANES], b[LWE_MFMA_LANES];
          LweTile c[LWE_MFMA_LANES];
          for (u32 rt = 0; rt < LWE_MFMA_ROW_TILES; ++rt)
            for (u32 lane = 0; lane < LWE_MFMA_LANES; ++lane) a[rt][lane] = lwe_mfma_a_frag(img.data(), s, rt, lane);
          for (u32 l = 0; l < L; ++l) {
            for (u32 lane = 0; lane < LWE_MFMA_LANES; ++lane) b[lane] = lwe_mfma_b_frag(kprep, ct, step0 + s, l, steps, L, lane);
            for (u32 rt = 0; rt < rts; ++rt) {
              for (u32 lane = 0; lane < LWE_MFMA_LANES; ++lane) c[lane] = lanes[lane].acc[rt][l];
              lwe_mfma_step_wave(a[rt], b, c);                                 // one matrix instruction of the wave
              for (u32 lane = 0; lane < LWE_MFMA_LANES; ++lane) lanes[lane].acc[rt][l] = c[lane];
            }
          }
        }
        if (chunks == LWE_MFMA_FLUSH_CHUNKS)
          for (u32 lane = 0; lane < LWE_MFMA_LANES; ++lane)
            for (u32 rt = 0; rt < LWE_MFMA_ROW_TILES; ++rt) lwe_mfma_fold<L>(lanes[lane].acc[rt], lanes[lane].wide[rt]);
      }
      if (chunks == LWE_MFMA_FLUSH_CHUNKS) chunks = 0;
      // ---- __syncthreads() ----
    }
    for (u32 wave = 0; wave < LWE_MFMA_WAVES; ++wave) {
      const u32 ct = t.ct0 + wave;
      if (ct >= cts) continue;
      for (u32 lane = 0; lane < LWE_MFMA_LANES; ++lane) {
        Lane& r = regs[(size_t)wave * LWE_MFMA_LANES + lane];
        for (u32 rt = 0; rt < rts; ++rt) {
          lwe_mfma_fold<L>(r.acc[rt], r.wide[rt]);
          lwe_mfma_finish<E>(lwe.data(), out.data(), t, rt, lane, ct * LWE_MFMA_COL_TILE + (lane & 15), n_in, n_out, r.wide[rt], offset, red, ar);
        }
      }
    }
  }
  for (size_t i = 0; i < out.size(); ++i) out64[i] = out[i];
  return 0;
}
template <typename E, typename... A> int keyswitch_emu(u32 limbs, A... args) {
  switch (limbs) {          // the launcher's dispatch (kernels_lwe_mfma.hip), every count for either lane
    case 1: return keyswitch_emu_l<E, 1>(args...);
    case 2: return keyswitch_emu_l<E, 2>(args...);
    case 3: return keyswitch_emu_l<E, 3>(args...);
    case 4: return keyswitch_emu_l<E, 4>(args...);
    case 5: return keyswitch_emu_l<E, 5>(args...);
    case 6: return keyswitch_emu_l<E, 6>(args...);
    case 7: return keyswitch_emu_l<E, 7>(args...);
    case 8: return keyswitch_emu_l<E, 8>(args...);
  }
  return 2;
}

ApiPlan view_of(u64 q) { return ApiPlan{4, q < ((u64)1 << 31) ? 4 : 8, false, false, q}; }

}  // namespace

extern "C" {

// The kernels' tile sizes, for the tests that choose shapes around them: which 0 rows of a workgroup's tile, 1 its columns, 2 the
// K step, 3 the slots per pass of the digit image, 4 the column tile, 5 the products per fold, 6 the bytes of the digit image.
uint32_t emu_lwe_mfma_geometry(int which) {
  const uint32_t g[] = {LWE_MFMA_ROWS, LWE_MFMA_COLS, LWE_MFMA_K_STEP, LWE_MFMA_CHUNK, LWE_MFMA_COL_TILE, LWE_MFMA_FLUSH_PRODUCTS, LWE_MFMA_IMAGE};
  return which >= 0 && which < 7 ? g[which] : 0;
}
uint32_t emu_lwe_mfma_limbs(uint64_t q) { return lwe_mfma_limbs(q); }
// byte offset of a lane's A fragment of (step of the chunk, row tile) in the digit image (tests/test_lwe_mfma_emu.py: banks)
uint32_t emu_lwe_mfma_a_frag_offset(uint32_t step, uint32_t rt, uint32_t lane) { return lwe_mfma_img_offset(rt * 16 + (lane & 15), step * 64 + 16 * (lane >> 4)); }

// One matrix step by the header's host loop: a, b 64 lanes x 16 bytes, c 64 lanes x 4 sums, in place.
void emu_lwe_mfma_step(const void* a, const void* b, int32_t* c) {
  LweFrag fa[LWE_MFMA_LANES], fb[LWE_MFMA_LANES];
  LweTile fc[LWE_MFMA_LANES];
  std::memcpy(fa, a, sizeof fa); std::memcpy(fb, b, sizeof fb); std::memcpy(fc, c, sizeof fc);
  lwe_mfma_step_wave(fa, fb, fc);
  std::memcpy(c, fc, sizeof fc);
}

// tn_lwe_ksk_prepared_bytes / tn_lwe_ksk_prepare_dev: ksk [n_in][terms][n_out + 1] words (as uint64) -> kprep.  0 ok, 2 a modulus
// the library has not, 4 what the entry points refuse, 5 a kprep off its alignment.
int emu_lwe_ksk_prepared_bytes(uint64_t q, size_t n_in, size_t n_out, size_t terms, size_t* bytes) {
  if (!modulus_ok(q)) return 2;
  ApiCheck k{view_of(q), "emu"};
  if (!check_lwe_ksk_bytes(k, n_in, n_out, terms, bytes)) return 4;
  *bytes = lwe_mfma_prepared_bytes(q, n_in, n_out, terms);
  return 0;
}
int emu_lwe_ksk_prepare(uint64_t q, const uint64_t* ksk, void* kprep, size_t n_in, size_t n_out, size_t terms) {
  if (!modulus_ok(q)) return 2;
  ApiCheck k{view_of(q), "emu"};
  if (!check_lwe_ksk_shape(k, n_in, n_out, terms)) return 4;
  if (!k.aligned16(kprep)) return 5;
  return with_lane(q, [&](auto e) { return prepare_emu<decltype(e)>(q, ksk, (signed char*)kprep, n_in, n_out, terms); });
}

// tn_lwe_keyswitch_prepared_dev: lwe [batch][n_in + 1] words (as uint64), kprep of emu_lwe_ksk_prepare, out [batch][n_out + 1].
// flags: bit 0 = balanced digits.
int emu_lwe_keyswitch_prepared(uint64_t q, const uint64_t* lwe, const void* kprep, uint64_t* out, size_t batch, size_t n_in, size_t n_out,
                               size_t terms, uint32_t base_log, uint32_t flags) {
  if (!modulus_ok(q)) return 2;
  ApiCheck k{view_of(q), "emu"};
  if (!(k.lwe_dim(n_in, "n_in") && k.lwe_dim(n_out, "n_out") && k.gadget(n_in, terms, base_log, flags, "n_in * terms", "key rows") &&
        k.lwe_byte_digits(base_log, flags) && k.lwe_sum(n_in, terms) && k.rows(batch, n_in + 1, "", "") && k.rows(batch, n_out + 1, "", "")))
    return 4;
  if (!k.aligned16(kprep)) return 5;
  return with_lane(q, [&](auto e) {
    return keyswitch_emu<decltype(e)>(lwe_mfma_limbs(q), q, lwe, (const signed char*)kprep, out, batch, n_in, n_out, terms, base_log, (flags & 1u) != 0);
  });
}

// The argument checks of the three entry points (api_checks.h, the lists capi.cpp runs) on a plan view made of (n, elem_bytes,
// has_fused, omega_only, q); n == 0 is a NULL plan.  No pointer is read.  Returns the status; *launch = 1 when the call would go
// on; msg receives the text tn_last_error would give.
int emu_lwe_ksk_prepared_bytes_api_check(uint32_t n, int elem_bytes, int has_fused, int omega_only, uint64_t q, size_t n_in, size_t n_out, size_t terms,
                                         const void* bytes, int* launch, char* msg, size_t msg_len) {
  ApiCheck k{ApiPlan{n, elem_bytes, has_fused != 0, omega_only != 0, q}, "tn_lwe_ksk_prepared_bytes"};
  return api_answer(k, check_lwe_ksk_bytes(k, n_in, n_out, terms, (const size_t*)bytes), launch, msg, msg_len);
}
int emu_lwe_ksk_prepare_api_check(uint32_t n, int elem_bytes, int has_fused, int omega_only, uint64_t q, const void* ksk, const void* kprep, size_t n_in,
                                  size_t n_out, size_t terms, int* launch, char* msg, size_t msg_len) {
  ApiCheck k{ApiPlan{n, elem_bytes, has_fused != 0, omega_only != 0, q}, "tn_lwe_ksk_prepare_dev"};
  return api_answer(k, check_lwe_ksk_prepare(k, ksk, kprep, n_in, n_out, terms), launch, msg, msg_len);
}
int emu_lwe_keyswitch_prepared_api_check(uint32_t n, int elem_bytes, int has_fused, int omega_only, uint64_t q, const void* lwe, const void* kprep,
                                         const void* out, size_t batch, size_t n_in, size_t n_out, size_t terms, uint32_t base_log, uint32_t flags,
                                         int* launch, char* msg, size_t msg_len) {
  ApiCheck k{ApiPlan{n, elem_bytes, has_fused != 0, omega_only != 0, q}, "tn_lwe_keyswitch_prepared_dev"};
  return api_answer(k, check_lwe_keyswitch_prepared(k, lwe, kprep, out, batch, n_in, n_out, terms, base_log, flags), launch, msg, msg_len);
}

}  // extern "C"

#ifdef EMU_SANITIZE_CASES
#include "../emu/sanitize_cases.h"
#include <cstdlib>
// The cases sanitize_lwe_mfma.cpp runs (lwe_mfma_cases): the limb rule, the prepared key through the layout rule and the stepped
// key switch against 128-bit host arithmetic written here, at either lane width, on exactly sized buffers (the sanitizer sees every
// access past one), shapes with ragged tiles; the fold on saturated sums; then the argument lists on made-up addresses.
void lwe_mfma_cases();
namespace {

typedef unsigned __int128 u128;

// an exactly sized, 16-byte aligned heap block: an access one byte past it is the sanitizer's to see
struct Exact {
  void* p; size_t bytes;
  explicit Exact(size_t n) : p(std::aligned_alloc(16, (n + 15) / 16 * 16)), bytes(n) {}
  ~Exact() { std::free(p); }
};

void stepping_cases(uint64_t q, uint32_t w_unsigned, uint32_t w_balanced) {
  uint64_t lcg = 88172645463325252ull ^ q;
  auto rnd = [&]() { lcg = lcg * 6364136223846793005ull + 1442695040888963407ull; return lcg; };
  auto word = [&]() { return q < ((uint64_t)1 << 31) ? (rnd() >> 32) : rnd(); };       // any word of the lane
  const uint32_t limbs = emu_lwe_mfma_limbs(q), terms = 3;
  // the limb rule, from the prepared key of a one-column key through the layout rule
  const size_t shapes[][3] = {{1, 1, 1}, {LWE_MFMA_ROWS + 1, 43, LWE_MFMA_COLS}, {17, 2 * LWE_MFMA_CHUNK / terms + 7, LWE_MFMA_COL_TILE - 2}};
  for (const auto& sh : shapes) {
    const size_t batch = sh[0], n_in = sh[1], n_out = sh[2], pitch = n_out + 1, slots = n_in * terms;
    std::vector<uint64_t> lwe(batch * (n_in + 1)), ksk(slots * pitch), out(batch * pitch);
    for (auto& v : lwe) v = word();
    for (auto& v : ksk) v = word();
    ksk[0] = q / 2; ksk[ksk.size() - 1] = q / 2 + 1; lwe[0] = q - 1;
    size_t bytes = 0;
    expect(emu_lwe_ksk_prepared_bytes(q, n_in, n_out, terms, &bytes) == 0 && bytes % 1024 == 0, "prepared bytes");
    Exact kprep(bytes);
    std::memset(kprep.p, 0x55, bytes);
    expect(emu_lwe_ksk_prepare(q, ksk.data(), kprep.p, n_in, n_out, terms) == 0, "prepare runs");
    const size_t steps = lwe_mfma_steps(n_in, terms), cols = lwe_mfma_col_tiles(n_out) * LWE_MFMA_COL_TILE;
    bool same = true;
    for (size_t k = 0; k < steps * LWE_MFMA_K_STEP; ++k)
      for (size_t c = 0; c < cols; ++c) {
        __int128 v = 0, p = 1;
        for (uint32_t l = 0; l < limbs; ++l, p *= 256) v += p * ((const signed char*)kprep.p)[lwe_mfma_key_offset(k, c, l, steps, limbs)];
        const uint64_t x = k < slots && c < pitch ? ksk[k * pitch + c] % q : 0;
        same = same && v == (x > q / 2 ? (__int128)x - (__int128)q : (__int128)x);
      }
    expect(same, "the prepared key holds the centred residues, zero in the padding");
    for (uint32_t flags = 0; flags < 2; ++flags) {
      const uint32_t w = flags ? w_balanced : w_unsigned;
      expect(emu_lwe_keyswitch_prepared(q, lwe.data(), kprep.p, out.data(), batch, n_in, n_out, terms, w, flags) == 0, "keyswitch runs");
      same = true;
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
              const uint64_t kw = ksk[(i * terms + j) * pitch + c] % q;
              sum = (sum + (u128)(neg ? B - t : t) * (neg ? q - kw : kw)) % q;
            }
          }
          same = same && out[r * pitch + c] == (uint64_t)sum;
        }
      expect(same, "keyswitch equals the definition");
    }
  }
}

// the fold: 2^16 products of (-128) (-128) in every 32-bit sum, then as many again, 3 folds and a tail
void fold_case() {
  const uint64_t q = 4294962689ull;
  const size_t n_in = (2 * LWE_MFMA_FLUSH_PRODUCTS + LWE_MFMA_CHUNK + 4) / 4, terms = 4, n_out = 1, batch = 1;
  std::vector<uint64_t> lwe(batch * (n_in + 1), 0x7F7F7F80ull), ksk(n_in * terms * 2, q - 128 - 128 * 256), out(2);
  size_t bytes = 0;
  expect(emu_lwe_ksk_prepared_bytes(q, n_in, n_out, terms, &bytes) == 0, "fold: bytes");
  Exact kprep(bytes);
  expect(emu_lwe_ksk_prepare(q, ksk.data(), kprep.p, n_in, n_out, terms) == 0, "fold: prepare");
  expect(emu_lwe_keyswitch_prepared(q, lwe.data(), kprep.p, out.data(), batch, n_in, n_out, terms, 8, 1) == 0, "fold: keyswitch");
  // every digit of 0x7F7F7F80 is -128 (balanced, w = 8: 0x80 -> -128 carry 1; 0x7F + 1 = 0x80 -> -128 carry 1; ...)
  const u128 term = (u128)128 * (128 + 128 * 256) % q, sum = term * (u128)(n_in * terms) % q;
  expect(out[0] == (uint64_t)sum && out[1] == (uint64_t)((sum + 0x7F7F7F80ull) % q), "fold: sums past 2^31 stay exact");
}

void api_cases() {
  const uint32_t n = 4;
  const uint64_t q = 7681;
  const uintptr_t base = 1 << 20, far = (uintptr_t)1 << 40;
  auto at = [](uintptr_t x) { return reinterpret_cast<const void*>(x); };
  char msg[256];
  int launch = -1;
  auto by = [&](size_t n_in, size_t n_out, size_t terms, uintptr_t bytes = 64, uint32_t plan_n = 4) {
    const int st = emu_lwe_ksk_prepared_bytes_api_check(plan_n, 4, 0, 0, q, n_in, n_out, terms, at(bytes), &launch, msg, sizeof msg);
    return st == TN_OK ? (launch ? 0 : -1) : st;
  };
  auto pr = [&](uintptr_t ksk, uintptr_t kprep, size_t n_in, size_t n_out, size_t terms) {
    const int st = emu_lwe_ksk_prepare_api_check(n, 4, 0, 0, q, at(ksk), at(kprep), n_in, n_out, terms, &launch, msg, sizeof msg);
    return st == TN_OK ? (launch ? 0 : -1) : st;
  };
  auto ks = [&](uintptr_t lwe, uintptr_t kprep, uintptr_t out, size_t batch, size_t n_in, size_t n_out, size_t terms, uint32_t w = 4, uint32_t flags = 0,
                uint64_t q_ = 7681, int bytes = 4) {
    const int st = emu_lwe_keyswitch_prepared_api_check(n, bytes, 0, 0, q_, at(lwe), at(kprep), at(out), batch, n_in, n_out, terms, w, flags, &launch, msg,
                                                        sizeof msg);
    return st == TN_OK ? (launch ? 0 : -1) : st;
  };
  expect(by(8, 5, 2) == 0 && by(8, 5, 2, 64, 0) == TN_EINVAL, "bytes ok, NULL plan");
  expect(by(0, 5, 2) == TN_EINVAL && by(8, 65537, 2) == TN_EINVAL && by(8, 5, 0) == TN_EINVAL && by(8, 5, 65) == TN_EINVAL, "bytes: dims, terms");
  expect(by(65536, 5, 64) == 0 && by(8, 5, 2, 0) == TN_EINVAL, "bytes: 2^22 slots fit, NULL answer");
  expect(pr(base, far, 8, 5, 2) == 0 && pr(0, far, 8, 5, 2) == TN_EINVAL && pr(base, far + 8, 8, 5, 2) == TN_EINVAL, "prepare ok, NULL, alignment");
  // q = 7681: 2 limbs; 8 * 2 = 16 slots -> 1 step, 6 columns -> 1 tile: 2 KiB of kprep against 16 * 6 * 4 bytes of ksk
  for (long off = -2048 - 32; off <= 16 * 6 * 4 + 32; off += 16) {
    const uintptr_t kp = base + off;
    const bool want = kp < base + 16 * 6 * 4 && base < kp + 2048;
    expect(pr(base, kp, 8, 5, 2) == (want ? (int)TN_EINVAL : 0), "kprep against ksk: the intersection of the byte ranges");
  }
  expect(ks(base, far, 2 * far, 3, 8, 5, 2) == 0, "keyswitch ok");
  expect(ks(base, far, 2 * far, 3, 0, 5, 2) == TN_EINVAL && ks(base, far, 2 * far, 3, 8, 5, 2, 13) == TN_EINVAL, "dimensions, 2^base_log above q");
  expect(ks(base, far, 2 * far, 3, 8, 5, 2, 8, 0) == TN_EUNSUPPORTED && ks(base, far, 2 * far, 3, 8, 5, 2, 7, 0) == 0, "unsigned digits of 8 bits");
  expect(ks(base, far, 2 * far, 3, 8, 5, 2, 9, 1) == TN_EUNSUPPORTED && ks(base, far, 2 * far, 3, 8, 5, 2, 8, 1) == 0, "balanced digits of 9 bits");
  expect(ks(0, 0, 0, 0, 8, 5, 2) == -1 && ks(base, 0, 2 * far, 3, 8, 5, 2) == TN_EINVAL, "batch 0, NULL kprep");
  expect(ks(base, far + 4, 2 * far, 3, 8, 5, 2) == TN_EINVAL, "kprep off its alignment");
  for (long off = -80; off <= 2048 + 80; off += 4) {
    const uintptr_t out = base + off;
    const bool want_lwe = out < base + 3 * 9 * 4 && base < out + 3 * 6 * 4, want_key = out < base + 2048 && base < out + 3 * 6 * 4;
    expect(ks(base, far, out, 3, 8, 5, 2) == (want_lwe ? (int)TN_EINVAL : 0), "out against lwe: the intersection of the byte ranges");
    expect(ks(far, base, out, 3, 8, 5, 2) == (want_key ? (int)TN_EINVAL : 0), "out against kprep: the intersection of the byte ranges");
  }
}

void step_case() {
  // the host loop against the product written out: A one-hot at (row 3, k 37), B one-hot at (k 37, col 9), C = 5 everywhere
  LweFrag a[LWE_MFMA_LANES] = {}, b[LWE_MFMA_LANES] = {};
  int32_t c[LWE_MFMA_LANES * 4];
  for (auto& v : c) v = 5;
  a[3 + 16 * (37 / 16)].w[(37 % 16) / 4] = (uint32_t)(uint8_t)(-128) << (8 * (37 % 4));
  b[9 + 16 * (37 / 16)].w[(37 % 16) / 4] = (uint32_t)(uint8_t)127 << (8 * (37 % 4));
  emu_lwe_mfma_step(a, b, c);
  bool same = true;
  for (uint32_t l = 0; l < LWE_MFMA_LANES; ++l)
    for (uint32_t e = 0; e < 4; ++e) same = same && c[l * 4 + e] == ((4 * (l >> 4) + e == 3 && (l & 15) == 9) ? 5 - 128 * 127 : 5);
  expect(same, "one-hot step");
}

}  // namespace

void lwe_mfma_cases() {
  step_case();
  stepping_cases(7681, 4, 5);
  stepping_cases(8380417, 7, 8);
  stepping_cases(1152921504606830593ull, 7, 8);
  stepping_cases(4611686018427387904ull - 58, 5, 8);      // an even composite below 2^62: a general plan's modulus
  fold_case();
  api_cases();
}
#endif
