// emu_pack.cpp — TEST INFRASTRUCTURE: steps the pack / trace step kernel (polydot_pack_kernel: tiny_ntt_amd/csrc/kernels_pack.hip)
// on the CPU, one emulated thread at a time, with the Stepper of tests/emu/emu_stepper.h and the headers the gfx950 kernel is
// compiled from (fused_core.h, pack_core.h, galois_core.h, cmux_core.h).  One emulated workgroup takes the rows in turn, as a
// persistent workgroup does.  Per row: the words of ev[row][1] and the rotated words of od[row][1] (monomial_index,
// monomial_negated) become d[1] (pack_rotated_word, pack_diff_word), which is scattered under sigma_g through the Stepper's own
// transpose image (galois_dst, pack_scatter_word) and read back at the thread's phase-0 indices; per term (gadget_term_step)
// gadget_digit, ONE forward transform, component 0's product through dot_product_into and component 1's in place; inverse 0; s[0]
// joins its output (pack_sum_word, pack_add_in) and d[0] takes the way through the image and is added in; inverse 1; s[1], formed
// from the words read again, joins its output.  Every loop over the threads ends where the kernel has a workgroup barrier (or,
// in a workgroup of one wave, where program order stands for it).  Every word of the image carries the permutation it was
// written for and the three hazards of the kernel's comment are tagged (code 9):
//   (1) a scatter comes only when a transform has run to its end since the last read-back (the image is free of its readers),
//   (2) a read-back sees words of its own scatter, and only when all n have been written,
//   (3) a transform begins only when all n words of the last scatter have been read back.
// What the tags do and do not show: the stepping runs every loop over the threads to its end before the next begins, so the tags
// hold wherever the ORDER of the kernel's steps is right (a scatter moved in front of an inverse, a transform begun between a
// scatter and its read-back, a row's second scatter running into the next row's first are caught).  They do not show that a
// barrier stands between two steps: the kernel's READBACK_BARRIER, which only some shapes need, could be removed without a tag
// changing.  That barrier is covered on the device alone (tests/test_gpu_pack.py runs every fused shape).
// The trace form (od == NULL) steps the kernel's TRACE instantiation: ev goes raw through the scatter (galois_scatter_word) and
// the sums are ev mod q (gadget_canon).
// Also the stepping of the LWE embedding (lwe_embed_kernel: kernels_lwe.hip, lwe_core.h's lwe_embed_words), the two entry points'
// argument lists (csrc/api_checks.h: check_pack_step, check_lwe_embed) for the CPU and the destination map by itself.  A library
// of its own, tests/emu_pack/_build/libemu_pack.so (tests/test_pack_emu.py, tests/test_lwe_embed.py, tests/test_gpu_pack.py);
// with -DEMU_SANITIZE_CASES its cases for sanitize_pack.cpp (make -C tests/emu_pack sanitize).
#include "../emu/emu_stepper.h"
#include "../../tiny_ntt_amd/csrc/pack_core.h"
#include "../../tiny_ntt_amd/csrc/lwe_core.h"
#include <string>

namespace {

// ev, od, c: [batch][2][n] (od may be NULL: the trace step); bhat: [sets][2][terms][n]
template <typename Sh, bool BC>
int polydot_pack_emu(const HostTables& t, const u64* ev, const u64* od, u32 rot, u32 galois, const u64* bhat, size_t bhat_sets, u64* c, size_t batch,
                     size_t terms, u32 base_log, bool balanced) {
  typedef typename Sh::E E;
  constexpr int LOGN = Sh::LOGN;
  typedef Policy<E, Sh::LAZY> Pol;
  typedef Stepper<E, LOGN, Sh::LPT, Pol, BC> S;
  typedef typename S::Cfg Cfg;
  constexpr u32 N = (u32)Cfg::N, EMASK = 2u * N - 1u;
  static_assert(Cfg::lds_elems() >= Cfg::N, "the transpose image holds a row");
  const FusedProductSetup<E> su = fused_product_setup(h_make_arith<E>(t), BC, false);
  S wg{su.ar};
  const typename S::Table fwd(t, su.fwd), inv(t, su.inv);
  std::vector<typename S::Regs> xw(S::T), xr(S::T), ad(S::T), acc0(S::T), acc1(S::T);
  std::vector<typename S::Regs>* const sums[2] = {&acc0, &acc1};
  std::vector<u32> carries(S::T);
  rot &= EMASK;
  // the tags
  std::vector<u32> written_for(N, 0);                        // the permutation each word of the image was scattered for
  u32 permutation = 0;                                       // 1, 2, ...: two per row
  size_t scattered = 0, read_back = N;                       // of the current permutation
  bool transform_since = true;                               // the barrier behind the staging of the twiddles
  int hazard = 0;
  auto own = [](u32 tau, int r) { return (u32)r * Cfg::THREADS + tau; };     // phase 0: the words thread tau owns
  auto transform_begins = [&]() {
    if (read_back != N) hazard = 9;                          // hazard (3)
    transform_since = true;
  };
  // every thread's words of row `arow` of ev, and the rotated words of that row of od (zeros in the trace step)
  auto request = [&](std::vector<typename S::Regs>& e, std::vector<typename S::Regs>& o, size_t arow) {
    for (u32 tau = 0; tau < S::T; ++tau) {
      const u32 t0 = (tau - rot) & EMASK;
      for (int r = 0; r < Cfg::R; ++r) {
        e[tau].x[r] = (E)ev[(arow << LOGN) + own(tau, r)];
        o[tau].x[r] = od ? (E)od[(arow << LOGN) + monomial_index(t0 + (u32)r * Cfg::THREADS, (u32)LOGN)] : (E)0;
      }
    }
  };
  auto t_word = [&](E x, u32 tau, int r) {
    return pack_rotated_word<E, Pol>(x, monomial_negated(((tau - rot) & EMASK) + (u32)r * Cfg::THREADS, (u32)LOGN), wg.ar);
  };
  // x: every thread's words of d (pack form: canonical; trace form: ev's own, any words) -> its words of sigma_g(d), through the image
  const bool trace = od == nullptr;
  auto permute = [&](std::vector<typename S::Regs>& x) {
    E* img = wg.lds.data();
    if (!transform_since || read_back != N) hazard = 9;      // hazard (1)
    ++permutation;
    scattered = 0;
    for (u32 tau = 0; tau < S::T; ++tau)
      for (int r = 0; r < Cfg::R; ++r) {
        bool neg;
        const u32 d = galois_dst(own(tau, r), galois, (u32)LOGN, neg);
        img[d] = trace ? galois_scatter_word<E, Pol>(x[tau].x[r], neg, wg.ar) : pack_scatter_word<E>(x[tau].x[r], neg, wg.ar.q);
        written_for[d] = permutation;
        ++scattered;
      }
    // ---- __syncthreads(): hazard (2) ----
    read_back = 0;
    transform_since = false;
    for (u32 tau = 0; tau < S::T; ++tau)
      for (int r = 0; r < Cfg::R; ++r) {
        if (scattered != N || written_for[own(tau, r)] != permutation) hazard = 9;
        x[tau].x[r] = img[own(tau, r)];
        ++read_back;
      }
  };
  for (size_t row = 0; row < batch; ++row) {
    request(xw, xr, row * 2 + 1);                            // requested behind the previous row's second store
    for (u32 tau = 0; tau < S::T; ++tau) {
      for (int r = 0; r < Cfg::R; ++r) {
        if (!trace) xw[tau].x[r] = pack_diff_word<E, Pol>(xw[tau].x[r], t_word(xr[tau].x[r], tau, r), wg.ar);
        acc0[tau].x[r] = 0;
        acc1[tau].x[r] = 0;
      }
      carries[tau] = 0;
    }
    permute(xw);                                             // the top of the row
    const size_t set = (bhat_sets == 1 ? 0 : row) * 2 * terms;
    for (size_t j = 0; j < terms; ++j) {
      const size_t boff[2] = {set + j, set + terms + j};
      transform_begins();
      gadget_term_step(wg, fwd, xw, carries, j, base_log, balanced, bhat, 2, boff, sums);      // (barriers inside)
    }
    transform_begins();
    wg.inverse(acc0, inv);                                   // (ends with a barrier: the image is free)
    request(ad, xr, row * 2);                                // ev[row][0] inside inverse 0, the rotated od[row][0] behind it
    for (u32 tau = 0; tau < S::T; ++tau)
      for (int r = 0; r < Cfg::R; ++r) {
        if (trace) {                                         // s[0] = ev[0] mod q; d[0] = ev[0] is made canonical in the scatter
          acc0[tau].x[r] = pack_add_in<E>(acc0[tau].x[r], gadget_canon<E, Pol>(ad[tau].x[r], wg.ar), wg.ar.q);
          continue;
        }
        const E tw = t_word(xr[tau].x[r], tau, r);
        acc0[tau].x[r] = pack_add_in<E>(acc0[tau].x[r], pack_sum_word<E, Pol>(ad[tau].x[r], tw, wg.ar), wg.ar.q);
        ad[tau].x[r] = pack_diff_word<E, Pol>(ad[tau].x[r], tw, wg.ar);
      }
    permute(ad);
    // ---- __syncthreads() where the second inverse's first exchange has none: hazard (3) ----
    for (u32 tau = 0; tau < S::T; ++tau)
      for (int r = 0; r < Cfg::R; ++r) c[((row * 2) << LOGN) + own(tau, r)] = pack_add_in<E>(acc0[tau].x[r], ad[tau].x[r], wg.ar.q);
    transform_begins();
    wg.inverse(acc1, inv);
    request(ad, xr, row * 2 + 1);                            // both again: the rotated words inside inverse 1, ev[row][1] behind it (c overlaps neither)
    for (u32 tau = 0; tau < S::T; ++tau)
      for (int r = 0; r < Cfg::R; ++r)
        c[((row * 2 + 1) << LOGN) + own(tau, r)] =
            pack_add_in<E>(acc1[tau].x[r], trace ? gadget_canon<E, Pol>(ad[tau].x[r], wg.ar) : pack_sum_word<E, Pol>(ad[tau].x[r], t_word(xr[tau].x[r], tau, r), wg.ar),
                           wg.ar.q);
  }
  return hazard;
}

template <typename E> int embed_emu(u32 n, u64 q, const u64* lwe64, u64* a64, size_t batch, u32 index) {
  Arith<E> ar = {};
  ar.q = (E)q;
  ar.one = h_lwe_tw(1 % q, q, (E)0);
  u32 logn = 0;
  while ((1u << logn) < n) ++logn;
  std::vector<E> lwe(batch * ((size_t)n + 1)), a(batch * 2 * (size_t)n);
  for (size_t i = 0; i < lwe.size(); ++i) lwe[i] = (E)lwe64[i];      // words travel as uint64; a 32-bit lane sees the low half
  const size_t threads = 3 * (size_t)LWE_THREADS;                     // a grid of three workgroups
  for (size_t tid = 0; tid < threads; ++tid) lwe_embed_words<E>(lwe.data(), a.data(), (u32)batch, logn, index, tid, threads, ar);
  for (size_t i = 0; i < a.size(); ++i) a64[i] = a[i];
  return 0;
}

}  // namespace

extern "C" {

// The kernel's flow on ev, od [batch][2][n] (od NULL: the trace step).  0 ok, 2 bad params, 3 bad bhat_sets / ev, 4 what the gadget
// calls refuse (terms, base_log, flags), 5 an element that is not odd and below 2n or a rotation the entry point refuses, 7
// unsupported n, 9 an access to the image out of its order.  Words travel as uint64 regardless of lane width.
// canonical: the canonical policy (TN_PLAN_FORCE_CANONICAL).  flags: bit 0 = balanced digits.
int emu_poly_pack_step_prepared(uint32_t n, uint64_t q, uint64_t psi, int canonical, const uint64_t* ev, const uint64_t* od, uint32_t rot, uint32_t galois,
                                const uint64_t* bhat, size_t bhat_sets, uint64_t* c, size_t batch, size_t terms, uint32_t base_log, uint32_t flags) {
  if (bhat_sets != 1 && bhat_sets != batch) return 3;
  if (!ev) return 3;
  if (!params_ok(n, q, psi)) return 2;
  const HostTables t = h_build_tables(n, q, psi, !(canonical & 1));
  if (!gadget_ok(t, terms, base_log, flags)) return 4;
  if (!(galois & 1u) || galois >= 2 * (uint64_t)n || rot >= 2 * (uint64_t)n || (!od && rot)) return 5;
  const bool bal = (flags & 1u) != 0;
  return emu_with_shape(t, [&](auto sh, auto bc) {
    return polydot_pack_emu<decltype(sh), decltype(bc)::value>(t, ev, od, rot, galois, bhat, bhat_sets, c, batch, terms, base_log, bal);
  });
}

// lwe [batch][n + 1] -> a [batch][2][n], the inverse of the extraction at `index`.  0 ok, 2 a plan the library has not, 4 index >= n.
int emu_lwe_embed(uint32_t n, uint64_t q, const uint64_t* lwe, uint64_t* a, size_t batch, uint32_t index) {
  if (!(n >= 4 && !(n & (n - 1)) && n <= 8192 && q >= 2 && q < ((u64)1 << 62))) return 2;
  if (index >= n) return 4;
  return q < ((u64)1 << 31) ? embed_emu<u32>(n, q, lwe, a, batch, index) : embed_emu<u64>(n, q, lwe, a, batch, index);
}

// The two maps of a row's loads and scatter: dst[s] = the image word that source word s goes to under sigma_g, bit 31 set where it is
// negated (galois_dst); src[i] = the word of od that X^rot brings to word i, bit 31 set where it is negated (monomial_index,
// monomial_negated, as the kernel forms them from a thread's first index and a register's offset).
void emu_pack_maps(uint32_t logn, uint32_t g, uint32_t rot, uint32_t threads, uint32_t* dst, uint32_t* src) {
  const u32 n = 1u << logn, emask = 2u * n - 1u;
  for (u32 s = 0; s < n; ++s) {
    bool neg;
    const u32 d = galois_dst(s, g, logn, neg);
    dst[s] = d | (neg ? 0x80000000u : 0u);
    const u32 tau = s % threads, v = ((tau - (rot & emask)) & emask) + (s - tau);
    src[s] = monomial_index(v, logn) | (monomial_negated(v, logn) ? 0x80000000u : 0u);
  }
}

// The argument checks of tn_poly_pack_step_prepared_dev and tn_lwe_embed_dev (api_checks.h, the lists capi.cpp runs) on a plan
// view made of (n, elem_bytes, has_fused, omega_only, q); n == 0 is a NULL plan.  No pointer is read.  Returns the status;
// *launch = 1 when the call would go on to its launch; msg receives the text tn_last_error would give.
int emu_pack_api_check(uint32_t n, int elem_bytes, int has_fused, int omega_only, uint64_t q, const void* ev, const void* od, uint32_t rot, uint32_t galois,
                       const void* bhat, const void* c, size_t sets, size_t batch, size_t terms, uint32_t base_log, uint32_t flags, int* launch, char* msg,
                       size_t msg_len) {
  ApiCheck k{ApiPlan{n, elem_bytes, has_fused != 0, omega_only != 0, q}, "tn_poly_pack_step_prepared_dev"};
  return api_answer(k, check_pack_step(k, ev, od, rot, galois, bhat, sets, c, batch, terms, base_log, flags), launch, msg, msg_len);
}
int emu_lwe_embed_api_check(uint32_t n, int elem_bytes, int has_fused, int omega_only, uint64_t q, const void* lwe, const void* a, size_t batch,
                            uint32_t index, int* launch, char* msg, size_t msg_len) {
  ApiCheck k{ApiPlan{n, elem_bytes, has_fused != 0, omega_only != 0, q}, "tn_lwe_embed_dev"};
  return api_answer(k, check_lwe_embed(k, lwe, a, batch, index), launch, msg, msg_len);
}

}  // extern "C"

#ifdef EMU_SANITIZE_CASES
#include "../emu/sanitize_cases.h"
// The cases sanitize_pack.cpp runs (pack_cases): the stepping at the smallest shape of either lane width and at the base-case
// shape, both policies, batch 2 x 2 terms, one shared set and one per row, both digit modes, (g, rot) pairs that cover the
// wrap's sign on both maps, and the trace step, each compared with the explicit route stepped: the monomial product's stepping
// on od, s and d in 128-bit host arithmetic, the automorphism key switch's stepping on d, the addition of s.  Then the
// embedding on exactly sized buffers against host arithmetic, and the argument lists on made-up addresses.
extern "C" int emu_monomial_mul(uint32_t n, uint64_t q, const uint64_t* a, const uint32_t* exps, uint64_t* out, size_t batch, size_t group, uint32_t flags);
extern "C" int emu_poly_galois_keyswitch_prepared(uint32_t n, uint64_t q, uint64_t psi, int canonical, const uint64_t* a, uint32_t galois, const uint64_t* bhat,
                                                  size_t bhat_sets, uint64_t* c, size_t batch, size_t terms, uint32_t base_log, uint32_t flags);
void pack_cases();
namespace {

void stepping_cases(uint32_t n, uint64_t q, uint64_t psi) {
  const size_t batch = 2, terms = 2, words = batch * 2 * n;
  uint64_t lcg = 88172645463325252ull ^ q;
  auto rnd = [&]() { lcg = lcg * 6364136223846793005ull + 1442695040888963407ull; return lcg; };
  std::vector<uint64_t> ev(words), od(words), bh(batch * 2 * terms * n), c(words), t(words), s(words), d(words), ks(words);
  for (auto& v : ev) v = q < ((uint64_t)1 << 31) ? (rnd() >> 32) : rnd();      // any word of the lane
  for (auto& v : od) v = q < ((uint64_t)1 << 31) ? (rnd() >> 32) : rnd();
  for (auto& v : bh) v = rnd() % q;                                          // prepared rows hold canonical words
  ev[0] = q - 1; ev[1] = q; ev[2] = 0; od[0] = q - 1; od[1] = 0; od[2] = q; od[n] = q - 1; ev[n] = 0; ev[n + 1] = q - 1; od[n + 1] = q - 1;
  const uint32_t w = (uint32_t)((64 - __builtin_clzll(q)) + 1) / 2;
  const uint32_t pairs[][2] = {{3, 0}, {5, 1}, {n + 1, n / 2}, {2 * n - 1, n}, {3, 2 * n - 1}, {5, n - 1}};
  for (int form = 0; form < 7; ++form) {                                     // 6: the trace step
    const bool trace = form == 6;
    const uint32_t g = trace ? 2 * n - 1 : pairs[form][0], rot = trace ? 0 : pairs[form][1];
    for (int canonical = 0; canonical < 2; ++canonical)
      for (size_t sets : {(size_t)1, batch})
        for (uint32_t flags = 0; flags < 2; ++flags) {
          expect(emu_poly_pack_step_prepared(n, q, psi, canonical, ev.data(), trace ? nullptr : od.data(), rot, g, bh.data(), sets, c.data(), batch, terms, w,
                                             flags) == 0, "runs, no hazard tag");
          if (trace) {
            std::fill(t.begin(), t.end(), 0);
          } else {
            const std::vector<uint32_t> exps(batch, rot);
            expect(emu_monomial_mul(n, q, od.data(), exps.data(), t.data(), batch, 2, 0) == 0, "monomial product runs");
          }
          for (size_t i = 0; i < words; ++i) {
            const uint64_t e = (q < ((uint64_t)1 << 31) ? (uint32_t)ev[i] : ev[i]) % q;
            s[i] = (uint64_t)(((unsigned __int128)e + t[i]) % q);
            d[i] = (uint64_t)(((unsigned __int128)e + q - t[i]) % q);
          }
          expect(emu_poly_galois_keyswitch_prepared(n, q, psi, canonical, d.data(), g, bh.data(), sets, ks.data(), batch, terms, w, flags) == 0, "key switch runs");
          bool same = true;
          for (size_t i = 0; i < words; ++i) same = same && c[i] == (uint64_t)(((unsigned __int128)ks[i] + s[i]) % q);
          expect(same, "equals the explicit route stepped");
        }
  }
}

void embed_cases(uint32_t n, uint64_t q) {
  const size_t batch = 3;
  uint64_t lcg = 2463534242ull ^ q;
  auto rnd = [&]() { lcg = lcg * 6364136223846793005ull + 1442695040888963407ull; return lcg; };
  std::vector<uint64_t> lwe(batch * (n + 1)), a(batch * 2 * n);
  for (auto& v : lwe) v = q < ((uint64_t)1 << 31) ? (rnd() >> 32) : rnd();
  lwe[0] = q; lwe[1] = 0; lwe[2] = q - 1;
  for (uint32_t index : {0u, 1u, n / 2, n - 1}) {
    expect(emu_lwe_embed(n, q, lwe.data(), a.data(), batch, index) == 0, "embedding runs");
    bool same = true;
    for (size_t r = 0; r < batch; ++r)
      for (uint32_t k = 0; k < n; ++k) {
        const uint64_t x = lwe[r * (n + 1) + (k <= index ? index - k : n + index - k)] % q;
        same = same && a[(r * 2 + 1) * n + k] == (k <= index ? x : (q - x) % q);
        same = same && a[(r * 2) * n + k] == (k == index ? lwe[r * (n + 1) + n] % q : 0);
      }
    expect(same, "embedding is the definition");
  }
  expect(emu_lwe_embed(n, q, lwe.data(), a.data(), batch, n) == 4, "index n refused");
}

void api_cases() {
  const uint32_t n = 4;
  const uint64_t q = 7681;
  const uintptr_t row = n * 4, base = 1 << 20, far = (uintptr_t)1 << 40, mid = (uintptr_t)1 << 30;
  auto at = [](uintptr_t x) { return reinterpret_cast<const void*>(x); };
  auto run = [&](uintptr_t ev, uintptr_t od, uint32_t rot, uint32_t g, uintptr_t b, uintptr_t c, size_t sets, size_t batch, size_t terms, uint32_t w = 4,
                 uint32_t flags = 0, int fused = 1) {
    int launch = -1;
    char msg[256];
    const int st = emu_pack_api_check(n, 4, fused, 0, q, at(ev), at(od), rot, g, at(b), at(c), sets, batch, terms, w, flags, &launch, msg, sizeof msg);
    return st == TN_OK ? (launch ? 0 : -1) : st;
  };
  expect(run(base, mid, 3, 3, far, 2 * far, 1, 3, 2) == 0, "ok");
  expect(run(base, mid, 7, 1, far, 2 * far, 3, 3, 2) == 0, "a key per row, rot = 2n - 1 ok");
  expect(run(base, 0, 0, 7, far, 2 * far, 1, 3, 2) == 0, "the trace step ok");
  expect(run(base, 0, 1, 7, far, 2 * far, 1, 3, 2) == TN_EINVAL, "the trace step with a rotation");
  expect(run(base, mid, 8, 3, far, 2 * far, 1, 3, 2) == TN_EINVAL, "rot = 2n");
  expect(run(base, mid, 3, 4, far, 2 * far, 1, 3, 2) == TN_EINVAL, "even element");
  expect(run(base, mid, 3, 9, far, 2 * far, 1, 3, 2) == TN_EINVAL, "element above 2n");
  expect(run(base, mid, 3, 3, far, 2 * far, 1, 3, 2, 4, 0, 0) == TN_EUNSUPPORTED, "no fused kernels");
  expect(run(base, mid, 8, 3, far, 2 * far, 1, 3, 2, 4, 0, 0) == TN_EUNSUPPORTED, "no fused kernels before the rotation");
  expect(run(base, mid, 3, 3, far, 2 * far, 1, 3, 0) == TN_EINVAL, "terms 0");
  expect(run(base, mid, 3, 3, far, 2 * far, 1, 3, 2, 4, 2) == TN_EINVAL, "flag 2");
  expect(run(base, mid, 3, 3, far, 2 * far, 1, 0, 2) == -1, "batch 0 launches nothing");
  expect(run(0, mid, 3, 3, far, 2 * far, 1, 3, 2) == TN_EINVAL, "NULL ev");
  expect(run(base, mid, 3, 3, far, 2 * far, 2, 3, 2) == TN_EINVAL, "sets 2");
  // byte by byte: c's batch * 2 rows against ev's and od's batch * 2 rows and against the set's 2 * terms rows
  for (size_t batch = 1; batch <= 2; ++batch)
    for (size_t terms = 1; terms <= 2; ++terms)
      for (int which = 0; which < 3; ++which)
        for (long off = -5 * (long)row; off <= 9 * (long)row; off += (long)row / 2) {
          const size_t in_rows = which < 2 ? batch * 2 : 2 * terms;
          const uintptr_t out = base + off;
          const bool want = out < base + in_rows * row && base < out + batch * 2 * row;
          const int st = which == 0 ? run(base, mid, 3, 3, far, out, 1, batch, terms)
                       : which == 1 ? run(mid, base, 3, 3, far, out, 1, batch, terms) : run(far, mid, 3, 3, base, out, 1, batch, terms);
          expect(st == (want ? (int)TN_EINVAL : 0), "overlap is the intersection of the byte ranges");
        }
}

}  // namespace

void pack_cases() {
  const uint64_t q60 = 1152921504606830593ull, psi4096 = 431606828070683274ull;
  stepping_cases(256, 8380417, 1239911);
  stepping_cases(256, q60, h_powmod(psi4096, 16, q60));
  stepping_cases(4096, q60, psi4096);
  embed_cases(256, 8380417);
  embed_cases(1024, q60);
  api_cases();
}
#endif
