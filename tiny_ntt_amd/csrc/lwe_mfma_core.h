// lwe_mfma_core.h — the LWE-to-LWE key switch on the gfx950 matrix cores: the per-lane and per-tile code of the two kernels of
// kernels_lwe_mfma.hip (lwe_ksk_prepare_kernel, lwe_keyswitch_mfma_kernel), free of HIP, so tests/emu_lwe_mfma steps on the CPU
// exactly what the kernels run.  include/tinyntt.h has the definitions, DESIGN.md 3.2l the reasons, api_checks.h the bounds.
//
// out[r][c] = ( [c == n_out] b_r + sum_k d_k(r) key[k][c] ) mod q, k = i terms + j over K = n_in terms slots, is computed as an
// exact integer: d_k(r) is the library's digit as a signed byte (gadget_digit), key[k][c] the centred residue of the key word cut
// into L = lwe_mfma_limbs(q) balanced base-256 limbs, so sum_k d_k key[k][c] = sum_l 256^l sum_k d_k limb_l[k][c], and every
// inner sum is what v_mfma_i32_16x16x64_i8 computes.  It differs from lwe_keyswitch_kernel's sum (q - k for negative digits) by
// multiples of q only.
//
// The matrix step (lwe_mfma_step_lane / lwe_mfma_step_wave): D = A B + C on a wave of 64 lanes, A 16 x 64 and B 64 x 16 signed
// bytes, C and D 16 x 16 32-bit sums.  Lane l holds 16 bytes of A and of B and 4 words of C/D:
//   A: byte j of lane l is A[row l & 15][k = 16 (l >> 4) + j]        (rows of A: batch rows)
//   B: byte j of lane l is B[k = 16 (l >> 4) + j][col l & 15]        (columns of B: output columns)
//   C/D: word e of lane l is D[row 4 (l >> 4) + e][col l & 15]
// Byte j of a fragment is byte j & 3 of its 32-bit word j >> 2 (little endian).  tests/test_gpu_lwe_mfma.py checks this map on the
// hardware against lwe_mfma_step_wave before anything else.
//
// Tile: a workgroup of LWE_MFMA_WAVES = 4 waves owns LWE_MFMA_ROWS = 64 batch rows (LWE_MFMA_ROW_TILES = 4 A fragments) by
// LWE_MFMA_COLS = 64 columns; wave v owns column tile 4 slab + v and keeps 4 x L accumulator tiles: every B fragment it loads (16
// bytes per lane, one aligned global load, 1 KiB per wave at unit stride) serves 4 matrix steps.  The digits go chunk by chunk
// (LWE_MFMA_CHUNK = 512 slots) through an LDS image in A-fragment order, img[step][row tile][lane][16 bytes], cut once per
// workgroup (lwe_mfma_cut), read by every wave as one 16-byte word per lane at consecutive addresses (no bank conflict:
// tests/test_lwe_mfma_emu.py).  Rows past the batch and slots past K hold zero digits; the key's padding holds zero limbs.
#pragma once
#include "lwe_core.h"
#include "api_checks.h"       // LWE_MFMA_K_STEP, LWE_MFMA_COL_TILE, LWE_MFMA_FLUSH_PRODUCTS, lwe_mfma_limbs, lwe_mfma_prepared_bytes

namespace tn {

constexpr u32 LWE_MFMA_LANES = 64;
constexpr u32 LWE_MFMA_WAVES = LWE_THREADS / LWE_MFMA_LANES;                   // 4
constexpr u32 LWE_MFMA_ROW_TILES = 4;                                          // A fragments against one B fragment
constexpr u32 LWE_MFMA_ROWS = LWE_MFMA_ROW_TILES * 16;                         // 64 batch rows per workgroup
constexpr u32 LWE_MFMA_COLS = LWE_MFMA_WAVES * LWE_MFMA_COL_TILE;              // 64 columns per workgroup
constexpr u32 LWE_MFMA_CHUNK = 512;                                            // slots per pass of the digit image
constexpr u32 LWE_MFMA_CHUNK_STEPS = LWE_MFMA_CHUNK / LWE_MFMA_K_STEP;         // 8
constexpr u32 LWE_MFMA_IMAGE = LWE_MFMA_CHUNK * LWE_MFMA_ROWS;                 // 32 KiB of LDS
// a 32-bit sum is folded after at most LWE_MFMA_FLUSH_PRODUCTS = 2^16 products of magnitude <= 2^14 (api_checks.h): 128 chunks
constexpr u32 LWE_MFMA_FLUSH_CHUNKS = LWE_MFMA_FLUSH_PRODUCTS / LWE_MFMA_CHUNK;
constexpr u32 LWE_MFMA_MAX_LIMBS = 8;
constexpr u32 LWE_MFMA_PREP_IMAGE = LWE_MFMA_WAVES * LWE_MFMA_MAX_LIMBS * LWE_MFMA_FRAG_BYTES;      // 32 KiB: 4 column tiles x L limb planes of one K step
static_assert(LWE_MFMA_CHUNK % LWE_MFMA_K_STEP == 0 && LWE_MFMA_FLUSH_PRODUCTS % LWE_MFMA_CHUNK == 0, "whole steps per chunk, whole chunks per fold");

struct alignas(16) LweFrag { u32 w[4]; };        // a lane's 16 signed bytes of A or B
struct LweTile { int32_t v[4]; };                // a lane's 4 sums of C/D

// ---- one int8 matrix step ---------------------------------------------------------------------------------------
#if defined(__HIPCC__)
// this lane's fragments; the wave computes c += a b
__device__ __forceinline__ void lwe_mfma_step_lane(const LweFrag& a, const LweFrag& b, LweTile& c) {
#if defined(__HIP_DEVICE_COMPILE__)
  typedef int v4i __attribute__((ext_vector_type(4)));
  const v4i av = {(int)a.w[0], (int)a.w[1], (int)a.w[2], (int)a.w[3]}, bv = {(int)b.w[0], (int)b.w[1], (int)b.w[2], (int)b.w[3]};
  v4i cv = {c.v[0], c.v[1], c.v[2], c.v[3]};
  cv = __builtin_amdgcn_mfma_i32_16x16x64_i8(av, bv, cv, 0, 0, 0);
  c.v[0] = cv[0]; c.v[1] = cv[1]; c.v[2] = cv[2]; c.v[3] = cv[3];
#else
  (void)a; (void)b; (void)c;
#endif
}
#endif
inline int lwe_frag_byte(const LweFrag& f, u32 j) { return (int)(signed char)(unsigned char)(f.w[j >> 2] >> (8 * (j & 3))); }
// the same step on the host: the 64 lanes' fragments, by the lane -> element map at the top of this file
inline void lwe_mfma_step_wave(const LweFrag* a, const LweFrag* b, LweTile* c) {
  for (u32 l = 0; l < LWE_MFMA_LANES; ++l)
    for (u32 e = 0; e < 4; ++e) {
      const u32 row = 4 * (l >> 4) + e, col = l & 15;
      int64_t sum = c[l].v[e];
      for (u32 k = 0; k < LWE_MFMA_K_STEP; ++k) sum += lwe_frag_byte(a[row + 16 * (k >> 4)], k & 15) * lwe_frag_byte(b[col + 16 * (k >> 4)], k & 15);
      c[l].v[e] = (int32_t)sum;                  // (the kernels' bounds keep it in 32 bits: api_checks.h)
    }
}

// ---- the limb rule ----------------------------------------------------------------------------------------------
// limb l of the key word x: canonical, centred into (-q/2, q/2], cut from the low end into balanced base-256 limbs.  The signed
// low byte of a two's-complement word IS its balanced residue mod 256.
template <typename E> TN_HD void lwe_mfma_cut_limbs(E x, u32 limbs, signed char* s, const Arith<E>& ar) {
  const E xc = lwe_canon(x, ar);
  int64_t c = xc > (E)(ar.q >> 1) ? (int64_t)xc - (int64_t)ar.q : (int64_t)xc;       // q < 2^62
  for (u32 l = 0; l < limbs; ++l) {
    const signed char b = (signed char)(unsigned char)((u64)c & 0xffu);
    s[l] = b;
    c = (c - b) >> 8;                              // exact: c - b is a multiple of 256
  }
}

// ---- the prepared key -------------------------------------------------------------------------------------------
// byte offset of limb l of key[k][col]: [column tile][K step][limb][lane][16 bytes], lane = (col & 15) + 16 ((k & 63) >> 4)
TN_HD size_t lwe_mfma_key_offset(size_t k, size_t col, u32 l, size_t steps, u32 limbs) {
  const size_t frag = ((col / LWE_MFMA_COL_TILE) * steps + k / LWE_MFMA_K_STEP) * limbs + l;
  return (frag * LWE_MFMA_LANES + (col & 15) + 16 * ((k & 63) >> 4)) * 16 + (k & 15);
}
// The prepare kernel's tile: K step `step` by the 4 column tiles from ct0 on.  lwe_mfma_prep_stage reads 64 key rows of 64
// consecutive words (a wave per row: unit stride), cuts the limbs and puts them as bytes into the image [column tile][limb][lane][16];
// behind the barrier lwe_mfma_prep_store copies the image out as 16-byte words at unit stride (a column tile's limb planes of a
// step are one run of limbs KiB).  Key rows past K and columns past n_out give zero limbs; column tiles past the last are not stored.
struct LwePrepTile { u32 step, ct0; };
TN_HD u32 lwe_mfma_prep_tiles(u32 steps, u32 cts) { return steps * ((cts + LWE_MFMA_WAVES - 1) / LWE_MFMA_WAVES); }
TN_HD LwePrepTile lwe_mfma_prep_tile(u32 tile, u32 steps) { return {tile % steps, (tile / steps) * LWE_MFMA_WAVES}; }
template <typename E>
TN_HD void lwe_mfma_prep_stage(const E* __restrict__ ksk, signed char* img, const LwePrepTile& t, u32 slots, u32 n_out, u32 limbs, u32 tid,
                               const Arith<E>& ar) {
  const u32 c = tid & 63, col = t.ct0 * LWE_MFMA_COL_TILE + c;
  for (u32 kk = tid >> 6; kk < LWE_MFMA_K_STEP; kk += LWE_THREADS / 64) {
    const u32 k = t.step * LWE_MFMA_K_STEP + kk;
    signed char s[LWE_MFMA_MAX_LIMBS];
    const bool inside = k < slots && col <= n_out;
    lwe_mfma_cut_limbs<E>(inside ? galois_ld(ksk + ((size_t)k * (n_out + 1) + col)) : (E)0, limbs, s, ar);
    for (u32 l = 0; l < limbs; ++l) img[((((c >> 4) * limbs + l) * LWE_MFMA_LANES) + (c & 15) + 16 * (kk >> 4)) * 16 + (kk & 15)] = s[l];
  }
}
TN_HD void lwe_mfma_prep_store(const signed char* img, signed char* __restrict__ kprep, const LwePrepTile& t, u32 steps, u32 cts, u32 limbs,
                                      u32 tid) {
  const u32 per_ct = limbs * LWE_MFMA_LANES;                                   // 16-byte words of one column tile
  for (u32 u = tid; u < LWE_MFMA_WAVES * per_ct; u += LWE_THREADS) {
    const u32 ct = t.ct0 + u / per_ct;
    if (ct >= cts) break;                                                      // (u grows with the column tile)
    const size_t dst = (((size_t)ct * steps + t.step) * per_ct + u % per_ct) * 16;
    *reinterpret_cast<LweFrag*>(kprep + dst) = *reinterpret_cast<const LweFrag*>(img + (size_t)u * 16);
  }
}

// ---- the key switch ---------------------------------------------------------------------------------------------
struct LweMfmaTile { u32 row0, rows, ct0; };       // ct0: the first of the workgroup's 4 column tiles
TN_HD u32 lwe_mfma_slabs(u32 n_out) { return (n_out + 1 + LWE_MFMA_COLS - 1) / LWE_MFMA_COLS; }
TN_HD u32 lwe_mfma_row_tiles(u32 batch) { return (batch + LWE_MFMA_ROWS - 1) / LWE_MFMA_ROWS; }
// batch * (n_out + 1) <= 2^31 - 1: the count is below 2^31 / 4096 + 2^31 / 64 + 1026.  Slab-major, as lwe_ks_tiles.
TN_HD u32 lwe_mfma_tiles(u32 batch, u32 n_out) { return lwe_mfma_row_tiles(batch) * lwe_mfma_slabs(n_out); }
TN_HD LweMfmaTile lwe_mfma_tile(u32 tile, u32 batch) {
  const u32 rt = lwe_mfma_row_tiles(batch), row0 = (tile % rt) * LWE_MFMA_ROWS;
  return {row0, batch - row0 < LWE_MFMA_ROWS ? batch - row0 : LWE_MFMA_ROWS, (tile / rt) * LWE_MFMA_WAVES};
}

// byte of (row r of the tile, slot kk of the chunk) in the digit image
TN_HD u32 lwe_mfma_img_offset(u32 r, u32 kk) {
  return ((((kk >> 6) * LWE_MFMA_ROW_TILES + (r >> 4)) * LWE_MFMA_LANES) + (r & 15) + 16 * ((kk & 63) >> 4)) * 16 + (kk & 15);
}
// Thread tid's share of a pass: slots [k0, k0 + LWE_MFMA_CHUNK) of the tile's 64 rows as signed bytes.  A thread takes whole
// input words (the balanced carry runs up a word's digits) of the words that reach into the chunk, consecutive threads
// consecutive words of a row, and writes the digits whose slot lies inside; slots from K = slots on are zeroed up to the end of
// their K step (no step beyond it is read).  Rows past the batch hold zeros.
template <typename E>
TN_HD void lwe_mfma_cut(const E* __restrict__ lwe, signed char* img, const LweMfmaTile& t, u32 n_in, u32 slots, u32 k0, u32 terms, u32 w, bool balanced,
                        u32 tid, const Arith<E>& ar) {
  const u32 kend = slots - k0 < LWE_MFMA_CHUNK ? slots : k0 + LWE_MFMA_CHUNK;           // k0 < slots
  const u32 i_lo = k0 / terms, words = (kend - 1) / terms - i_lo + 1;
  for (u32 idx = tid; idx < words * LWE_MFMA_ROWS; idx += LWE_THREADS) {
    const u32 r = idx / words, i = i_lo + idx % words;
    const E x = r < t.rows ? lwe_canon(lwe[(size_t)(t.row0 + r) * (n_in + 1) + i], ar) : (E)0;
    u32 carry = 0;
    for (u32 j = 0; j < terms; ++j) {
      const E g = gadget_digit<E>(x, j * w, w, balanced, carry, ar.q);          // carry: this digit is negative (or its -0)
      const int d = (carry && g) ? -(int)(u32)(E)(ar.q - g) : (int)(u32)g;       // in [-128, 128): lwe_byte_digits
      const u32 k = i * terms + j;
      if (k >= k0 && k < kend) img[lwe_mfma_img_offset(r, k - k0)] = (signed char)d;
    }
  }
  const u32 pad = ((kend + LWE_MFMA_K_STEP - 1) & ~(LWE_MFMA_K_STEP - 1)) - kend;       // below 64
  for (u32 idx = tid; idx < pad * LWE_MFMA_ROWS; idx += LWE_THREADS) img[lwe_mfma_img_offset(idx / pad, kend - k0 + idx % pad)] = 0;
}
// K steps of the chunk at k0
TN_HD u32 lwe_mfma_chunk_steps(u32 slots, u32 k0) {
  return slots - k0 < LWE_MFMA_CHUNK ? (slots - k0 + LWE_MFMA_K_STEP - 1) / LWE_MFMA_K_STEP : LWE_MFMA_CHUNK_STEPS;
}
// a lane's A fragment of (step of the chunk, row tile) and its B fragment of (column tile, step of the key, limb)
TN_HD LweFrag lwe_mfma_a_frag(const signed char* img, u32 step, u32 rt, u32 lane) {
  return *reinterpret_cast<const LweFrag*>(img + (((size_t)step * LWE_MFMA_ROW_TILES + rt) * LWE_MFMA_LANES + lane) * 16);
}
TN_HD LweFrag lwe_mfma_b_frag(const signed char* __restrict__ kprep, size_t ct, size_t step, u32 l, size_t steps, u32 limbs, u32 lane) {
  return *reinterpret_cast<const LweFrag*>(kprep + (((ct * steps + step) * limbs + l) * LWE_MFMA_LANES + lane) * 16);
}

// sum += v 2^sh as two's-complement 128-bit integers, sh in {0, 8, .., 56}
TN_HD void lwe_wide_add(LweAcc& sum, int32_t v, u32 sh) {
  const int64_t x = v;
  const u64 lo = (u64)x << sh, hi = sh ? (u64)(x >> (64 - sh)) : (u64)(x >> 63);
  sum.lo += lo;
  sum.hi += hi + (sum.lo < lo ? 1u : 0u);
}
// The fold of one row tile's L accumulator tiles into its 4 wide sums: wide[e] += sum_l acc[l].v[e] 2^(8 l), magnitude below
// 2^30 (2^64 - 1) / 255 < 2^87 per fold; the accumulators start again from zero.
template <u32 L> TN_HD void lwe_mfma_fold(LweTile* acc, LweAcc* wide) {
#pragma unroll
  for (u32 l = 0; l < L; ++l)
#pragma unroll
    for (u32 e = 0; e < 4; ++e) {
      lwe_wide_add(wide[e], acc[l].v[e], 8 * l);
      acc[l].v[e] = 0;
    }
}
// A multiple of q that makes every total non-negative, chosen on the host and passed by value: 64-bit lanes, the smallest
// multiple from 2^94 on (|total| < 2^94, so 0 <= total + offset < 2^95 + 2^62: lwe_ks_reduce's hi limb is a word); 32-bit lanes
// (L <= 4: |total| < 2^6 2^30 (2^32 - 1) / 255 < 2^61), the smallest from 2^62 on: 0 <= total + offset < 2^64, hi is 0.
inline LweAcc h_lwe_mfma_offset(u64 q, int elem_bytes) {
  typedef unsigned __int128 u128;
  const u128 bound = (u128)1 << (elem_bytes == 8 ? 94 : 62), m = (bound + q - 1) / q * q;
  return {(u64)m, (u64)(m >> 64)};
}
// The store of a lane's 4 sums of one row tile: rows 4 (lane >> 4) + e of the row tile, column col; lwe_ks_reduce as it
// stands, the body b_r added in column n_out as lwe_ks_finish does.  Rows past the batch and columns past n_out are not stored.
template <typename E>
TN_HD void lwe_mfma_finish(const E* __restrict__ lwe, E* __restrict__ out, const LweMfmaTile& t, u32 rt, u32 lane, u32 col, u32 n_in, u32 n_out,
                           const LweAcc* wide, const LweAcc& offset, const LweRed<E>& red, const Arith<E>& ar) {
  if (col > n_out) return;
#pragma unroll
  for (u32 e = 0; e < 4; ++e) {
    const u32 r = rt * 16 + 4 * (lane >> 4) + e;
    if (r < t.rows) {
      LweAcc s = wide[e];
      s.lo += offset.lo;
      s.hi += offset.hi + (s.lo < offset.lo ? 1u : 0u);
      E v = lwe_ks_reduce<E>(s, red, ar);
      if (col == n_out) v = csub((E)(v + lwe_canon(lwe[(size_t)(t.row0 + r) * (n_in + 1) + n_in], ar)), ar.q);
      out[(size_t)(t.row0 + r) * (n_out + 1) + col] = v;
    }
  }
}

}  // namespace tn
