// galois_core.h — the ring automorphism sigma_g : a(x) -> a(x^g) mod (x^n + 1), g odd, on coefficient rows and on prepared
// rows: the index maps and the per-thread code of the two kernels of kernels_galois.hip, free of HIP, so tests/emu
// steps on the CPU exactly what the gfx950 kernels run.  include/tinyntt.h has the definition; DESIGN.md 3.2f the derivation.
// Also the per-word code of the automorphism key switch (kernels_galoisks.hip): galois_dst, galois_scatter_word,
// galois_add_in.
//
// Both kernels take a tile of rows through an LDS image: every thread stages words at unit stride (galois_stage), one barrier,
// then for each of the call's elements every thread reads the sources of its destination words from the image and stores them
// at unit stride (galois_gather / galois_gather_hat).  Both sides of HBM see unit-stride streams; the permutation happens in LDS.
#pragma once
#include "fused_core.h"

namespace tn {

constexpr u32 GALOIS_THREADS = 256;      // one workgroup
constexpr u32 GALOIS_TILE = 1024;        // words a workgroup takes per pass at least: 1024 / n rows for n < 1024, one row otherwise
constexpr u32 GALOIS_MAX = 16;           // TN_GALOIS_MAX: the elements travel by value in the kernel arguments
constexpr u32 GALOIS_UNROLL = 4;         // global loads in flight per thread while staging

// what a launch passes by value.  Coefficient kernel: v[m] = g_m^-1 mod 2n; prepared kernel: v[m] = g_m.
struct GaloisList { u32 count; u32 v[GALOIS_MAX]; };

TN_HD u32 galois_tile_rows(u32 logn) { return (1u << logn) >= GALOIS_TILE ? 1u : GALOIS_TILE >> logn; }
TN_HD u32 galois_tile_words(u32 logn) { return (1u << logn) >= GALOIS_TILE ? (1u << logn) : GALOIS_TILE; }

// The tile loop both kernels run: workgroup `first` of `stride` takes tiles first, first + stride, ... below galois_tiles();
// tile t holds rows [row0, row0 + rows) of the call, `words` words, and writes its images from out_offset on (count images
// per row).  The kernels and the CPU stepping take every bound from here.  rows_total <= 2^31 - 1 (check_automorphism).
struct GaloisTile { u32 row0, words; size_t in_offset, out_offset; };
TN_HD u32 galois_tiles(u32 rows_total, u32 logn) { const u32 rpp = galois_tile_rows(logn); return rows_total / rpp + (rows_total % rpp ? 1u : 0u); }
TN_HD GaloisTile galois_tile(u32 tile, u32 rows_total, u32 logn, u32 count) {
  const u32 rpp = galois_tile_rows(logn), row0 = tile * rpp, rows = rows_total - row0 < rpp ? rows_total - row0 : rpp;
  return {row0, rows << logn, (size_t)row0 << logn, ((size_t)row0 * count) << logn};
}

// g^-1 mod 2n for odd g (Newton: g is its own inverse mod 8, every step doubles the correct bits)
TN_HD u32 galois_inverse(u32 g, u32 logn) {
  u32 x = g;
  for (int i = 0; i < 4; ++i) x *= 2u - g * x;
  return x & ((2u << logn) - 1u);
}

// Coefficients, gather form: destination d takes a[u mod n], negated where u >= n, u = d g^-1 mod 2n (d g^-1 < 2^27).
TN_HD u32 galois_src(u32 d, u32 ginv, u32 logn, bool& negate) {
  const u32 u = (d * ginv) & ((2u << logn) - 1u);
  negate = (u >> logn) != 0;
  return u & ((1u << logn) - 1u);
}

// Prepared rows.  Word prep_idx(tau, r) = (r << (logn - lpt)) | tau of a row holds slot j = (tau << lpt) | r of the transform
// (FusedCfg::prep_idx, fused_core.h); slot j of a complete transform holds a(psi^(2 brv(j) + 1)).
TN_HD u32 galois_hat_slot(u32 word, u32 logn, u32 lpt) { return ((word & ((1u << (logn - lpt)) - 1u)) << lpt) | (word >> (logn - lpt)); }
TN_HD u32 galois_hat_word(u32 slot, u32 logn, u32 lpt) { return ((slot & ((1u << lpt) - 1u)) << (logn - lpt)) | (slot >> lpt); }

// The source word of destination word `word` under sigma_g.
//   complete transform: sigma_g(a)(psi^e) = a(psi^(e g)): slot j takes slot brv((e g mod 2n - 1) / 2), e = 2 brv(j) + 1.
//   BC (the forward stopped one stage early): slots (2i, 2i + 1) hold (a0, a1) = a mod (x^2 - zeta_i), zeta_i = psi^(2 e_i),
//     e_i = 2 brv_{logn-1}(i) + 1.  x^g = x (x^2)^((g-1)/2), so pair i takes pair i' = brv_{logn-1}((e_i g mod n - 1) / 2) as
//     (a0', a1' zeta_i^((g-1)/2)); fexp = e_i (g - 1) mod 2n is the exponent of psi of that factor (odd words; 0 for even ones).
template <bool BC> TN_HD u32 galois_hat_src(u32 word, u32 g, u32 logn, u32 lpt, u32& fexp) {
  const u32 j = galois_hat_slot(word, logn, lpt);
  fexp = 0;
  if constexpr (BC) {
    const u32 e = 2u * bitrev(j >> 1, (int)logn - 1) + 1u;
    const u32 e2 = (e * g) & ((1u << logn) - 1u);
    if (j & 1u) fexp = (e * (g - 1u)) & ((2u << logn) - 1u);
    return galois_hat_word((bitrev((e2 - 1u) >> 1, (int)logn - 1) << 1) | (j & 1u), logn, lpt);
  } else {
    const u32 e = 2u * bitrev(j, (int)logn) + 1u;
    const u32 e2 = (e * g) & ((2u << logn) - 1u);
    return galois_hat_word(bitrev((e2 - 1u) >> 1, (int)logn), logn, lpt);
  }
}

// rows streamed once: non-temporal on the device
template <typename E> TN_HD E galois_ld(const E* p) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_nontemporal_load(p);
#else
  return *p;
#endif
}
template <typename E> TN_HD void galois_st(E* p, E v) {
#if defined(__HIP_DEVICE_COMPILE__)
  __builtin_nontemporal_store(v, p);
#else
  *p = v;
#endif
}

template <typename E> TN_HD E galois_neg(E x, E q) { return x ? (E)(q - x) : (E)0; }      // -x mod q for canonical x; 0 stays 0

// Coefficients, scatter form (polydot_galoisks_kernel, kernels_galoisks.hip: the holder of a source word puts it where sigma_g
// takes it): source word s goes to word (s g) mod n, negated where bit log2 n of s g mod 2n is set (s g < 2^27).  The index
// is MASKED to the row: no g addresses a word outside it.  The same map as galois_src, read from the other side.
TN_HD u32 galois_dst(u32 s, u32 g, u32 logn, bool& negate) {
  const u32 t = s * g;
  negate = ((t >> logn) & 1u) != 0;
  return t & ((1u << logn) - 1u);
}
// one word of sigma_g on its way to the image: any word -> its canonical residue under the plan's policy, with the wrap's sign
template <typename E, typename Pol> TN_HD E galois_scatter_word(E x, bool negate, const Arith<E>& ar) {
  const E v = gadget_canon<E, Pol>(x, ar);
  return negate ? galois_neg(v, ar.q) : v;
}
// the add-in at the store: (x + s) mod q for canonical x (an inverse transform's output) and canonical s (a word of sigma_g(a))
template <typename E> TN_HD E galois_add_in(E x, E s, E q) { return csub((E)(x + s), q); }

// Staging half, thread tid: `words` words of the tile's rows (in: the tile's first row) into the image, unit stride, GALOIS_UNROLL
// loads requested before the first is used.  CANON: any word -> [0, q) with the canonical policy (gadget_decompose_kernel's).
template <typename E, bool CANON>
TN_HD void galois_stage(const E* __restrict__ in, E* img, u32 words, u32 tid, E q, typename TwOf<E>::type one) {
  for (u32 i0 = tid; i0 < words; i0 += GALOIS_UNROLL * GALOIS_THREADS) {
    E v[GALOIS_UNROLL];
#pragma unroll
    for (u32 k = 0; k < GALOIS_UNROLL; ++k) {
      const u32 i = i0 + k * GALOIS_THREADS;
      v[k] = i < words ? galois_ld(in + i) : (E)0;
    }
#pragma unroll
    for (u32 k = 0; k < GALOIS_UNROLL; ++k) {
      const u32 i = i0 + k * GALOIS_THREADS;
      if (i < words) img[i] = CANON ? mul_tw(v[k], one, q) : v[k];
    }
  }
}

// Gather half of the coefficient kernel, thread tid.  out: image m of the tile's row r is at out[(r * count + m) << logn].
template <typename E>
TN_HD void galois_gather(const E* img, E* __restrict__ out, u32 words, u32 logn, const GaloisList& gl, E q, u32 tid) {
  const u32 n1 = (1u << logn) - 1u;
  for (u32 m = 0; m < gl.count; ++m) {
    const u32 ginv = gl.v[m];
#pragma unroll 4
    for (u32 i = tid; i < words; i += GALOIS_THREADS) {
      const u32 d = i & n1;
      bool negate;
      const u32 s = galois_src(d, ginv, logn, negate);
      const E x = img[(i - d) + s];
      galois_st(out + ((((size_t)(i >> logn) * gl.count + m) << logn) + d), negate ? galois_neg(x, q) : x);
    }
  }
}

// The base case's factors psi^t, t < n, as a product of two records kept in LDS beside the image: ftab[t & 63] = psi^(t mod 64)
// and ftab[64 + (t >> 6)] = psi^(64 (t >> 6)), copied once per workgroup from the plan's psi_pow (split records).  One record
// per odd word straight from psi_pow is a 16-byte load at a bit-reversed index for every lane: 1,521 against 733 us per launch
// at n = 4096 / 60-bit, 65,536 rows (profiles/galois_factor_ab.txt).
constexpr u32 GALOIS_FLO = 64;
TN_HD u32 galois_factor_records(u32 logn) { return GALOIS_FLO + ((1u << logn) / GALOIS_FLO); }
template <typename E>
TN_HD void galois_stage_factors(const typename TwOf<E>::type* __restrict__ psi_pow, typename TwOf<E>::type* ftab, u32 logn, u32 tid) {
  for (u32 i = tid; i < galois_factor_records(logn); i += GALOIS_THREADS) ftab[i] = psi_pow[i < GALOIS_FLO ? i : (i - GALOIS_FLO) * GALOIS_FLO];
}

// Gather half of the prepared kernel.  Complete transform: a permutation of words.  BC: odd words are multiplied by
// +-psi^(fexp mod n) (two split products out of ftab: the first lazy, of any word, the second canonical).
template <typename E, bool BC>
TN_HD void galois_gather_hat(const E* img, E* __restrict__ out, u32 words, u32 logn, u32 lpt, const GaloisList& gl, const Arith<E>& ar,
                             const typename TwOf<E>::type* ftab, u32 tid) {
  const u32 n1 = (1u << logn) - 1u;
  for (u32 m = 0; m < gl.count; ++m) {
    const u32 g = gl.v[m];
#pragma unroll 4
    for (u32 i = tid; i < words; i += GALOIS_THREADS) {
      const u32 d = i & n1;
      u32 fexp;
      const u32 s = galois_hat_src<BC>(d, g, logn, lpt, fexp);
      E x = img[(i - d) + s];
      if constexpr (BC) {
        if ((d >> (logn - lpt)) & 1u) {      // an odd slot: register index r = word >> (logn - lpt) is the slot's low bits
          const u32 t = fexp & n1;
          x = mul_sp(x, ftab[GALOIS_FLO + (t >> 6)], ar.sk);
          x = Policy<E, true>::mul_tw_canon(x, ftab[t & (GALOIS_FLO - 1u)], ar);
          if (fexp >> logn) x = galois_neg(x, ar.q);
        }
      }
      galois_st(out + ((((size_t)(i >> logn) * gl.count + m) << logn) + d), x);
    }
  }
}

}  // namespace tn
