// lwe_core.h — the LWE ends of a programmable bootstrap: the modulus switch to 2n, the sample extraction and the LWE-to-LWE
// key switch: the per-word and per-tile code of the three kernels of kernels_lwe.hip, free of HIP, so tests/emu_lwe steps on
// the CPU exactly what the gfx950 kernels run.  include/tinyntt.h has the definitions; DESIGN.md 3.2k the reasons.
//
// Conventions (include/tinyntt.h): an LWE ciphertext of dimension d is a dense row of d + 1 words a_0 .. a_{d-1}, b with phase
// b + sum a_i s_i; an RLWE ciphertext is [2][n] with phase c0 + c1 s.  Every input word is taken mod q with the canonical
// policy's mul_tw(x, one, q), exact for any word on every plan (gadget_decompose_kernel's); outputs are canonical residues.
// The three kernels need q, the plan's `one` record and (the first two) log2 n: no table of the plan is read.
#pragma once
#include "fused_core.h"
#include "galois_core.h"      // galois_ld / galois_st (rows streamed once), galois_neg, the tile of rows of an LDS image

namespace tn {

constexpr u32 LWE_THREADS = 256;         // one workgroup, all three kernels

template <typename E> TN_HD E lwe_canon(E x, const Arith<E>& ar) { return mul_tw(x, ar.one, ar.q); }

// ---- modulus switch ---------------------------------------------------------------------------------------------
// floor((2n x + floor(q / 2)) / q) mod 2n for x = the word mod q.  2n x does not fit the lane, so: long division, one bit of
// the quotient per step (r < q < 2^(W-2) doubles without leaving the lane), log2(2n) steps leave 2n x = Q q + r; the rounding
// adds 1 where r + floor(q / 2) >= q (the sum is below 2q).  Q + 1 may reach 2n: the mask takes it to 0.
template <typename E> TN_HD u32 lwe_modswitch_word(E x, const Arith<E>& ar, u32 logn) {
  const E q = ar.q;
  E r = lwe_canon(x, ar);
  u32 e = 0;
  for (u32 b = 0; b <= logn; ++b) {
    r = (E)(r << 1);
    const bool ge = r >= q;
    r = ge ? (E)(r - q) : r;
    e = (e << 1) | (ge ? 1u : 0u);
  }
  e += (E)(r + (E)(q >> 1)) >= q ? 1u : 0u;
  return e & ((2u << logn) - 1u);
}

// lwe [batch][dim + 1] -> exps [dim + 1][batch]: a transpose.  A workgroup takes tiles of LWE_MS_TILE x LWE_MS_TILE words
// through an LDS image of exponents, rows padded by one word: a wave reads 64 consecutive words of a row of lwe and, behind
// the barrier, writes 64 consecutive words of a row of exps, reading the image at a stride of 65 words (conflict free).
constexpr u32 LWE_MS_TILE = 64;
constexpr u32 LWE_MS_PITCH = LWE_MS_TILE + 1;
constexpr u32 LWE_MS_IMAGE = LWE_MS_TILE * LWE_MS_PITCH;        // 32-bit words of LDS
struct LweMsTile { u32 row0, rows, col0, cols; };
TN_HD u32 lwe_ms_col_tiles(u32 dim) { return (dim + 1 + LWE_MS_TILE - 1) / LWE_MS_TILE; }
// batch * (dim + 1) <= 2^31 - 1 (check_lwe_modswitch): the count is below 2^31 / 4096 + 2^31 / 64 + 1026
TN_HD u32 lwe_ms_tiles(u32 batch, u32 dim) { return ((batch + LWE_MS_TILE - 1) / LWE_MS_TILE) * lwe_ms_col_tiles(dim); }
TN_HD LweMsTile lwe_ms_tile(u32 tile, u32 batch, u32 dim) {
  const u32 ct = lwe_ms_col_tiles(dim), row0 = (tile / ct) * LWE_MS_TILE, col0 = (tile % ct) * LWE_MS_TILE;
  return {row0, batch - row0 < LWE_MS_TILE ? batch - row0 : LWE_MS_TILE, col0, dim + 1 - col0 < LWE_MS_TILE ? dim + 1 - col0 : LWE_MS_TILE};
}
template <typename E>
TN_HD void lwe_ms_stage(const E* __restrict__ lwe, u32* img, const LweMsTile& t, u32 dim, u32 tid, const Arith<E>& ar, u32 logn) {
  const u32 c = tid & (LWE_MS_TILE - 1);
  if (c >= t.cols) return;
  for (u32 r = tid / LWE_MS_TILE; r < t.rows; r += LWE_THREADS / LWE_MS_TILE)
    img[r * LWE_MS_PITCH + c] = lwe_modswitch_word<E>(galois_ld(lwe + ((size_t)(t.row0 + r) * (dim + 1) + t.col0 + c)), ar, logn);
}
TN_HD void lwe_ms_store(const u32* img, u32* __restrict__ exps, const LweMsTile& t, u32 batch, u32 tid) {
  const u32 r = tid & (LWE_MS_TILE - 1);
  if (r >= t.rows) return;
  for (u32 c = tid / LWE_MS_TILE; c < t.cols; c += LWE_THREADS / LWE_MS_TILE)
    galois_st(exps + ((size_t)(t.col0 + c) * batch + t.row0 + r), img[r * LWE_MS_PITCH + c]);
}

// ---- sample extraction ------------------------------------------------------------------------------------------
// a [batch][2][n] -> lwe [batch][n + 1]: coefficient `index` of c0 + c1 s as an LWE phase: lwe[i] = c1[index - i] for
// i <= index, -c1[n + index - i] above it, lwe[n] = c0[index].  A reversed, partly negated copy: the c1 rows of a tile
// (galois_tile: 1024 / n rows, one from n = 1024 on) go into an LDS image at unit stride, canonical; behind the barrier
// every thread stores at unit stride, in one flat loop over the tile's rows * (n + 1) output words, what it reads from the image
// backwards (conflict free).  The image index is MASKED to the row, as galois_dst's is: no index addresses a word outside it.
// c0[index] is one word per row, read where it is stored.
template <typename E>
TN_HD void lwe_extract_stage(const E* __restrict__ a, E* img, u32 row0, u32 words, u32 logn, u32 tid, const Arith<E>& ar) {
  const u32 n1 = (1u << logn) - 1u;
  for (u32 i = tid; i < words; i += LWE_THREADS)
    img[i] = lwe_canon(galois_ld(a + ((((size_t)(row0 + (i >> logn)) * 2 + 1) << logn) + (i & n1))), ar);
}
template <typename E>
TN_HD void lwe_extract_gather(const E* __restrict__ a, const E* img, E* __restrict__ lwe, u32 row0, u32 words, u32 logn, u32 index, u32 tid,
                              const Arith<E>& ar) {
  const u32 n = 1u << logn, n1 = n - 1u, total = (words >> logn) * (n + 1);
  index &= n1;
  E* out = lwe + (size_t)row0 * (n + 1);                 // the tile's rows are one run of rows * (n + 1) words
  for (u32 j = tid; j < total; j += LWE_THREADS) {
    const u32 r = j / (n + 1), i = j - r * (n + 1);
    E v;
    if (i == n) {
      v = lwe_canon(a[(((size_t)(row0 + r) * 2) << logn) + index], ar);
    } else {
      const E x = img[(r << logn) + ((index - i) & n1)];
      v = i > index ? galois_neg(x, ar.q) : x;
    }
    galois_st(out + j, v);
  }
}

// ---- embedding --------------------------------------------------------------------------------------------------
// lwe [batch][n + 1] -> a [batch][2][n], the inverse of the extraction at `index`: a[1][k] = lwe[index - k] for k <= index,
// -lwe[n + index - k] above it; a[0][index] = lwe[n], 0 elsewhere.  Element-wise: thread `first` of `stride` takes output
// words first, first + stride, ... below batch * 2n (below 2^32: check_lwe_embed) and stores them at unit stride; a wave's
// loads run backwards over consecutive words (the same cache lines).  The index into the row is MASKED, as the extraction's.
template <typename E>
TN_HD void lwe_embed_words(const E* __restrict__ lwe, E* __restrict__ a, u32 batch, u32 logn, u32 index, size_t first, size_t stride, const Arith<E>& ar) {
  const u32 n = 1u << logn, n1 = n - 1u;
  index &= n1;
  const size_t total = ((size_t)batch * 2) << logn;
  for (size_t j = first; j < total; j += stride) {
    const size_t r = j >> (logn + 1);
    const u32 k = (u32)j & n1;
    const E* row = lwe + r * ((size_t)n + 1);
    E v;
    if (((j >> logn) & 1u) == 0) {
      v = k == index ? lwe_canon(row[n], ar) : (E)0;
    } else {
      const E x = lwe_canon(galois_ld(row + ((index - k) & n1)), ar);
      v = k > index ? galois_neg(x, ar.q) : x;
    }
    galois_st(a + j, v);
  }
}

// ---- key switch -------------------------------------------------------------------------------------------------
// out[r][k] = ( [k == n_out] b_r + sum_{i < n_in} sum_{j < terms} d_j(a_r[i]) ksk[i][j][k] ) mod q: a product
// [batch][n_in terms] x [n_in terms][n_out + 1] with small left factors.  A workgroup owns a tile of LWE_KS_ROWS batch rows by
// a slab of LWE_KS_COLS columns, a thread per column: key rows are read at unit stride and every key word serves
// LWE_KS_ROWS rows.  The input words go chunk by chunk (LWE_KS_SLOTS / terms of them) through an LDS slab of digits
// dig[slot][row], slot = (i - i0) terms + j, which is key row i0 terms + slot: lwe_ks_cut fills it (canonical word, the
// library's own gadget_digit, back to a signed integer), a barrier, lwe_ks_accumulate walks it (every lane reads the same
// LWE_KS_ROWS words: a broadcast), a barrier.
// Digits in the slab: unsigned mode, the digit itself, below 2^32; balanced mode, the signed digit in [-2^31, 2^31) as a
// two's-complement word (w <= 32: check_lwe_keyswitch).  A negative digit multiplies q - k in place of the key word k.
// Sums are not reduced: an accumulator is 128 bits, and one term is below 2^32 2^64 (unsigned mode: the key word is taken as it
// is, any word) or 2^31 2^62 (balanced mode: the key word is made canonical first, for q - k), so n_in terms <= 2^22 terms stay
// below 2^118 (api_checks.h: LWE_KS_MAX_SLOTS, LWE_KS_MAX_BASE_LOG; the checker refuses more).  One reduction per output word
// at the end (lwe_ks_reduce).
constexpr u32 LWE_KS_ROWS = 8;
constexpr u32 LWE_KS_COLS = LWE_THREADS;
constexpr u32 LWE_KS_SLOTS = 1024;                      // digit slots per row of the slab: 32 KiB of LDS
constexpr u32 LWE_KS_UNROLL = 4;                        // key words in flight per thread

struct LweAcc { u64 lo, hi; };

// 2^32 and 2^64 mod q as records of the canonical policy's product: what folds an accumulator's limbs (lwe_ks_reduce)
template <typename E> struct LweRed { typename TwOf<E>::type r32, r64; };
inline Tw64 h_lwe_tw(u64 w, u64 q, u64) { return h_make_tw64(w, q); }
inline Tw32 h_lwe_tw(u64 w, u64 q, u32) { return h_make_tw32(w, q); }
template <typename E> inline LweRed<E> h_lwe_red(u64 q) {
  LweRed<E> r;
  r.r32 = h_lwe_tw((u64)((((unsigned __int128)1) << 32) % q), q, (E)0);
  r.r64 = h_lwe_tw((u64)((((unsigned __int128)1) << 64) % q), q, (E)0);
  return r;
}

struct LweKsTile { u32 row0, rows, col0; };
TN_HD u32 lwe_ks_slabs(u32 n_out) { return (n_out + 1 + LWE_KS_COLS - 1) / LWE_KS_COLS; }
TN_HD u32 lwe_ks_row_tiles(u32 batch) { return (batch + LWE_KS_ROWS - 1) / LWE_KS_ROWS; }
// batch * (n_out + 1) <= 2^31 - 1 (check_lwe_keyswitch): the count is below 2^31 / 2048 + 2^31 / 8 + 258.  Slab-major: the
// workgroups in flight together walk the same columns of the key.
TN_HD u32 lwe_ks_tiles(u32 batch, u32 n_out) { return lwe_ks_row_tiles(batch) * lwe_ks_slabs(n_out); }
TN_HD LweKsTile lwe_ks_tile(u32 tile, u32 batch) {
  const u32 rt = lwe_ks_row_tiles(batch), row0 = (tile % rt) * LWE_KS_ROWS;
  return {row0, batch - row0 < LWE_KS_ROWS ? batch - row0 : LWE_KS_ROWS, (tile / rt) * LWE_KS_COLS};
}
TN_HD u32 lwe_ks_chunk(u32 terms) { return LWE_KS_SLOTS / terms; }      // input words per pass of the slab (terms <= 64: 16 at least)

// acc += mag * k
template <typename E> TN_HD void lwe_mac(LweAcc& acc, u32 mag, E k) {
  u64 add_lo, add_hi;
  if (sizeof(E) == 8) {
    const u64 p0 = (u64)mag * (u32)k;
    const u64 m = (u64)mag * (u32)((u64)k >> 32) + (p0 >> 32);        // the product is m 2^32 + lo32(p0)
    add_lo = (m << 32) | (u32)p0;
    add_hi = m >> 32;
  } else {
    add_lo = (u64)mag * (u32)k;
    add_hi = 0;
  }
  acc.lo += add_lo;
  acc.hi += add_hi + (acc.lo < add_lo ? 1u : 0u);
}

// Thread tid's share of a pass: words [i0, i0 + len) of the tile's rows into digits.  Rows past the batch hold zeros.
template <typename E>
TN_HD void lwe_ks_cut(const E* __restrict__ lwe, u32* dig, const LweKsTile& t, u32 n_in, u32 i0, u32 len, u32 terms, u32 w, bool balanced, u32 tid,
                      const Arith<E>& ar) {
  for (u32 r = 0; r < LWE_KS_ROWS; ++r)
    for (u32 ii = tid; ii < len; ii += LWE_THREADS) {
      u32* d = dig + (size_t)ii * terms * LWE_KS_ROWS + r;
      const E x = r < t.rows ? lwe_canon(lwe[(size_t)(t.row0 + r) * (n_in + 1) + i0 + ii], ar) : (E)0;
      u32 carry = 0;
      for (u32 j = 0; j < terms; ++j) {
        const E g = gadget_digit<E>(x, j * w, w, balanced, carry, ar.q);          // carry: this digit is negative (or its -0)
        const u32 mag = (u32)((carry && g) ? (E)(ar.q - g) : g);
        d[j * LWE_KS_ROWS] = carry ? 0u - mag : mag;
      }
    }
}

// One thread's column (kcol = ksk + the column) over the slab's `slots` key rows from key row krow0 on, LWE_KS_UNROLL key words
// requested before the first is used (galois_stage's way).
template <typename E, bool BAL>
TN_HD void lwe_ks_accumulate(const E* __restrict__ kcol, size_t pitch, size_t krow0, const u32* dig, u32 slots, LweAcc* acc, const Arith<E>& ar) {
  for (u32 s0 = 0; s0 < slots; s0 += LWE_KS_UNROLL) {
    E kk[LWE_KS_UNROLL];
#pragma unroll
    for (u32 u = 0; u < LWE_KS_UNROLL; ++u) kk[u] = s0 + u < slots ? kcol[(krow0 + s0 + u) * pitch] : (E)0;
#pragma unroll
    for (u32 u = 0; u < LWE_KS_UNROLL; ++u) {
      if (s0 + u >= slots) break;
      E k = kk[u], kn = 0;
      if (BAL) {
        k = lwe_canon(k, ar);
        kn = (E)(ar.q - k);
      }
      const u32* d = dig + (size_t)(s0 + u) * LWE_KS_ROWS;
#pragma unroll
      for (u32 r = 0; r < LWE_KS_ROWS; ++r) {
        const u32 raw = d[r];
        if (BAL) {
          const bool neg = (raw >> 31) != 0;
          lwe_mac<E>(acc[r], neg ? 0u - raw : raw, neg ? kn : k);
        } else {
          lwe_mac<E>(acc[r], raw, k);
        }
      }
    }
  }
}

// hi 2^64 + lo mod q, limb by limb.  32-bit lanes: a term is below 2^32 2^32, so hi stays below 2^22.
template <typename E> TN_HD E lwe_ks_reduce(const LweAcc& acc, const LweRed<E>& red, const Arith<E>& ar) {
  const E q = ar.q;
  if (sizeof(E) == 8) return csub((E)(mul_tw((E)acc.hi, red.r64, q) + lwe_canon((E)acc.lo, ar)), q);
  E v = lwe_canon((E)(u32)acc.lo, ar);
  v = csub((E)(v + mul_tw((E)(u32)(acc.lo >> 32), red.r32, q)), q);
  return csub((E)(v + mul_tw((E)(u32)acc.hi, red.r64, q)), q);
}

// The store of a thread's column: the reduced sums, the body b_r added in column n_out.
template <typename E>
TN_HD void lwe_ks_finish(const E* __restrict__ lwe, E* __restrict__ out, const LweKsTile& t, u32 n_in, u32 n_out, u32 col, const LweAcc* acc,
                         const LweRed<E>& red, const Arith<E>& ar) {
#pragma unroll
  for (u32 r = 0; r < LWE_KS_ROWS; ++r) {        // (a constant trip count: the sums stay in registers)
    if (r < t.rows) {
      E v = lwe_ks_reduce<E>(acc[r], red, ar);
      if (col == n_out) v = csub((E)(v + lwe_canon(lwe[(size_t)(t.row0 + r) * (n_in + 1) + n_in], ar)), ar.q);
      out[(size_t)(t.row0 + r) * (n_out + 1) + col] = v;
    }
  }
}

}  // namespace tn
