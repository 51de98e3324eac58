// emu_galoisks.cpp — TEST INFRASTRUCTURE: steps the automorphism key-switch kernel (polydot_galoisks_kernel:
// tiny_ntt_amd/csrc/kernels_galoisks.hip) on the CPU, one emulated thread at a time, with the Stepper of tests/emu/emu_stepper.h and the
// headers the gfx950 kernel is compiled from (fused_core.h, galois_core.h).  One emulated workgroup takes the rows in turn, as a
// persistent workgroup does, and the two permutations of a row go through the Stepper's own transpose image, which every
// exchange of a transform overwrites: the words of a[row][1] are scattered under sigma_g (galois_dst, galois_scatter_word) and
// read back at the thread's phase-0 indices, then per term (gadget_term_step) gadget_digit, ONE forward transform, component 0's
// product through dot_product_into and component 1's in place; two inverses; behind the first the words of a[row][0] take the
// same way through the image and are added in (galois_add_in).  Every loop over the threads below ends where the kernel has a
// workgroup barrier (or, in a workgroup of one wave, where program order stands for it).  On top of that every word of the
// image carries the permutation it was written for and the three hazards of the kernel's comment are tagged (code 9):
//   (1) a scatter comes only when a transform has run to its end since the last read-back (the image is free of its readers),
//   (2) a read-back sees words of its own scatter, and only when all n have been written,
//   (3) a transform begins only when all n words of the last scatter have been read back.
// Also the entry point's argument list (csrc/api_checks.h: check_galois_keyswitch) for the CPU and the image indices by
// themselves.  A library of its own, tests/emu_galoisks/_build/libemu_galoisks.so (tests/test_galoisks_emu.py,
// tests/test_gpu_galoisks.py); with -DEMU_SANITIZE_CASES its cases for sanitize_galoisks.cpp (make -C tests/emu_galoisks sanitize).
#include "../emu/emu_stepper.h"
#include "../../tiny_ntt_amd/csrc/galois_core.h"
#include <string>

namespace {

// a, c: [batch][2][n]; bhat: [sets][2][terms][n]
template <typename Sh, bool BC>
int polydot_galoisks_emu(const HostTables& t, const u64* a, u32 galois, const u64* bhat, size_t bhat_sets, u64* c, size_t batch, size_t terms,
                         u32 base_log, bool balanced) {
  typedef typename Sh::E E;
  constexpr int LOGN = Sh::LOGN;
  typedef Policy<E, Sh::LAZY> Pol;
  typedef Stepper<E, LOGN, Sh::LPT, Pol, BC> S;
  typedef typename S::Cfg Cfg;
  constexpr u32 N = (u32)Cfg::N;
  static_assert(Cfg::lds_elems() >= Cfg::N, "the transpose image holds a row");
  const FusedProductSetup<E> su = fused_product_setup(h_make_arith<E>(t), BC, false);
  S wg{su.ar};
  const typename S::Table fwd(t, su.fwd), inv(t, su.inv);
  std::vector<typename S::Regs> xw(S::T), ad(S::T), acc0(S::T), acc1(S::T);
  std::vector<typename S::Regs>* const sums[2] = {&acc0, &acc1};
  std::vector<u32> carries(S::T);
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
  // x: every thread's raw words of a row of a -> its words of sigma_g of that row, through the image
  auto permute = [&](std::vector<typename S::Regs>& x) {
    E* img = wg.lds.data();
    if (!transform_since || read_back != N) hazard = 9;      // hazard (1)
    ++permutation;
    scattered = 0;
    for (u32 tau = 0; tau < S::T; ++tau)
      for (int r = 0; r < Cfg::R; ++r) {
        bool neg;
        const u32 d = galois_dst(own(tau, r), galois, (u32)LOGN, neg);
        img[d] = galois_scatter_word<E, Pol>(x[tau].x[r], neg, wg.ar);
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
    for (u32 tau = 0; tau < S::T; ++tau) {
      for (int r = 0; r < Cfg::R; ++r) {
        xw[tau].x[r] = (E)a[((row * 2 + 1) << LOGN) + own(tau, r)];      // requested inside the previous row's second inverse
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
    for (u32 tau = 0; tau < S::T; ++tau)
      for (int r = 0; r < Cfg::R; ++r) ad[tau].x[r] = (E)a[((row * 2) << LOGN) + own(tau, r)];      // requested inside inverse 0
    permute(ad);
    // ---- __syncthreads() where the second inverse's first exchange has none: hazard (3) ----
    for (u32 tau = 0; tau < S::T; ++tau)
      for (int r = 0; r < Cfg::R; ++r) c[((row * 2) << LOGN) + own(tau, r)] = galois_add_in<E>(acc0[tau].x[r], ad[tau].x[r], wg.ar.q);
    transform_begins();
    wg.inverse(acc1, inv);
    for (u32 tau = 0; tau < S::T; ++tau)
      for (int r = 0; r < Cfg::R; ++r) c[((row * 2 + 1) << LOGN) + own(tau, r)] = acc1[tau].x[r];
  }
  return hazard;
}

}  // namespace

extern "C" {

// c[r][0] = sigma_g(a[r][0]) + sum_j digit_j(sigma_g(a[r][1])) * b[bhat_sets == 1 ? 0 : r][0][j],
// c[r][1] =                    sum_j digit_j(sigma_g(a[r][1])) * b[bhat_sets == 1 ? 0 : r][1][j]: the kernel's flow.  0 ok, 2 bad
// params, 3 bad bhat_sets / a, 4 what the gadget calls refuse (terms, base_log, flags), 5 an element that is not odd and below
// 2n, 7 unsupported n, 9 an access to the image out of its order.  Words travel as uint64 regardless of lane width.
// canonical: the canonical policy (TN_PLAN_FORCE_CANONICAL).  flags: bit 0 = balanced digits.
int emu_poly_galois_keyswitch_prepared(uint32_t n, uint64_t q, uint64_t psi, int canonical, const uint64_t* a, uint32_t galois, const uint64_t* bhat,
                                       size_t bhat_sets, uint64_t* c, size_t batch, size_t terms, uint32_t base_log, uint32_t flags) {
  if (bhat_sets != 1 && bhat_sets != batch) return 3;
  if (!a) return 3;
  if (!params_ok(n, q, psi)) return 2;
  const HostTables t = h_build_tables(n, q, psi, !(canonical & 1));
  if (!gadget_ok(t, terms, base_log, flags)) return 4;
  if (!(galois & 1u) || galois >= 2 * (uint64_t)n) return 5;
  const bool bal = (flags & 1u) != 0;
  return emu_with_shape(t, [&](auto sh, auto bc) {
    return polydot_galoisks_emu<decltype(sh), decltype(bc)::value>(t, a, galois, bhat, bhat_sets, c, batch, terms, base_log, bal);
  });
}

// The scatter's map alone (galois_core.h: galois_dst): dst[s] = the image word that source word s of a row goes to under
// sigma_g, bit 31 set where it is negated.
void emu_galoisks_dst_row(uint32_t logn, uint32_t g, uint32_t* dst) {
  for (u32 s = 0; s < (1u << logn); ++s) {
    bool neg;
    const u32 d = galois_dst(s, g, logn, neg);
    dst[s] = d | (neg ? 0x80000000u : 0u);
  }
}

// The argument checks of tn_poly_galois_keyswitch_prepared_dev (api_checks.h: check_galois_keyswitch, the list capi.cpp runs) on
// a plan view made of (n, elem_bytes, has_fused, omega_only, q); n == 0 is a NULL plan.  No pointer is read.  Returns the
// status; *launch = 1 when the call would go on to its launch; msg receives the text tn_last_error would give.
int emu_galoisks_api_check(uint32_t n, int elem_bytes, int has_fused, int omega_only, uint64_t q, const void* a, uint32_t galois, const void* bhat,
                           const void* c, size_t sets, size_t batch, size_t terms, uint32_t base_log, uint32_t flags, int* launch, char* msg,
                           size_t msg_len) {
  ApiCheck k{ApiPlan{n, elem_bytes, has_fused != 0, omega_only != 0, q}, "tn_poly_galois_keyswitch_prepared_dev"};
  return api_answer(k, check_galois_keyswitch(k, a, galois, bhat, sets, c, batch, terms, base_log, flags), launch, msg, msg_len);
}

}  // extern "C"

#ifdef EMU_SANITIZE_CASES
#include "../emu/sanitize_cases.h"
// The cases sanitize_galoisks.cpp runs (galoisks_cases): the stepping at the smallest shape of either lane width and at the
// base-case shape, both policies, batch 2 x 2 terms, one shared set and one per row, both digit modes, g = 1, 3, n + 1 and
// 2n - 1, each compared with the explicit route stepped: the automorphism kernel's stepping on the batch * 2 rows, the
// two-component gadget kernel's stepping on the rotated second rows, the addition.  Then the argument list on made-up addresses.
extern "C" int emu_automorphism(uint32_t n, uint64_t q, const uint64_t* a, uint64_t* out, size_t batch, const uint32_t* galois, size_t count);
extern "C" int emu_poly_gadget_multidot_prepared(uint32_t n, uint64_t q, uint64_t psi, int canonical, const uint64_t* a, const uint64_t* bhat,
                                                 size_t bhat_sets, uint64_t* c, size_t batch, size_t outs, size_t terms, uint32_t base_log, uint32_t flags);
void galoisks_cases();
namespace {

void stepping_cases(uint32_t n, uint64_t q, uint64_t psi) {
  const size_t batch = 2, terms = 2;
  uint64_t lcg = 88172645463325252ull ^ q;
  auto rnd = [&]() { lcg = lcg * 6364136223846793005ull + 1442695040888963407ull; return lcg; };
  std::vector<uint64_t> a(batch * 2 * n), bh(batch * 2 * terms * n), c(batch * 2 * n), rot(batch * 2 * n), a1(batch * n), ks(batch * 2 * n);
  for (auto& v : a) v = q < ((uint64_t)1 << 31) ? (rnd() >> 32) : rnd();       // any word of the lane
  for (auto& v : bh) v = rnd() % q;                                          // prepared rows hold canonical words
  a[0] = q - 1; a[1] = q; a[2] = 0; a[n] = q - 1; a[n + 1] = q; a[n + 2] = 0;
  const uint32_t w = (uint32_t)((64 - __builtin_clzll(q)) + 1) / 2;
  for (uint32_t g : {1u, 3u, n + 1, 2 * n - 1})
    for (int canonical = 0; canonical < 2; ++canonical)
      for (size_t sets : {(size_t)1, batch})
        for (uint32_t flags = 0; flags < 2; ++flags) {
          expect(emu_poly_galois_keyswitch_prepared(n, q, psi, canonical, a.data(), g, bh.data(), sets, c.data(), batch, terms, w, flags) == 0,
                 "runs, no hazard tag");
          expect(emu_automorphism(n, q, a.data(), rot.data(), batch * 2, &g, 1) == 0, "automorphism runs");
          for (size_t r = 0; r < batch; ++r)
            for (size_t i = 0; i < n; ++i) a1[r * n + i] = rot[(r * 2 + 1) * n + i];
          expect(emu_poly_gadget_multidot_prepared(n, q, psi, canonical, a1.data(), bh.data(), sets, ks.data(), batch, 2, terms, w, flags) == 0, "pair runs");
          bool same = true;
          for (size_t r = 0; r < batch; ++r)
            for (size_t i = 0; i < n; ++i) {
              const uint64_t want0 = (uint64_t)(((unsigned __int128)ks[(r * 2) * n + i] + rot[(r * 2) * n + i]) % q);
              same = same && c[(r * 2) * n + i] == want0 && c[(r * 2 + 1) * n + i] == ks[(r * 2 + 1) * n + i];
            }
          expect(same, "equals the explicit route stepped");
        }
}

void api_cases() {
  const uint32_t n = 4;
  const uint64_t q = 7681;
  const uintptr_t row = n * 4, base = 1 << 20, far = (uintptr_t)1 << 40;
  auto at = [](uintptr_t x) { return reinterpret_cast<const void*>(x); };
  auto run = [&](uintptr_t a, uint32_t g, uintptr_t b, uintptr_t c, size_t sets, size_t batch, size_t terms, uint32_t w = 4, uint32_t flags = 0, int fused = 1) {
    int launch = -1;
    char msg[256];
    const int st = emu_galoisks_api_check(n, 4, fused, 0, q, at(a), g, at(b), at(c), sets, batch, terms, w, flags, &launch, msg, sizeof msg);
    return st == TN_OK ? (launch ? 0 : -1) : st;
  };
  expect(run(base, 3, far, 2 * far, 1, 3, 2) == 0, "ok");
  expect(run(base, 1, far, 2 * far, 3, 3, 2) == 0, "a key per row, g = 1 ok");
  expect(run(base, 7, far, 2 * far, 1, 3, 2) == 0, "g = 2n - 1 ok");
  expect(run(base, 4, far, 2 * far, 1, 3, 2) == TN_EINVAL, "even element");
  expect(run(base, 9, far, 2 * far, 1, 3, 2) == TN_EINVAL, "element above 2n");
  expect(run(base, 3, far, 2 * far, 1, 3, 2, 4, 0, 0) == TN_EUNSUPPORTED, "no fused kernels");
  expect(run(base, 4, far, 2 * far, 1, 3, 2, 4, 0, 0) == TN_EUNSUPPORTED, "no fused kernels before the element");
  expect(run(base, 3, far, 2 * far, 1, 3, 0) == TN_EINVAL, "terms 0");
  expect(run(base, 3, far, 2 * far, 1, 3, 2, 4, 2) == TN_EINVAL, "flag 2");
  expect(run(base, 3, far, 2 * far, 1, 0, 2) == -1, "batch 0 launches nothing");
  expect(run(0, 3, far, 2 * far, 1, 3, 2) == TN_EINVAL, "NULL a");
  expect(run(base, 3, far, 2 * far, 2, 3, 2) == TN_EINVAL, "sets 2");
  expect(run(4096, 3, 4096, 4096, 1, (size_t)1 << 29, 2, 1) == TN_EINVAL, "2^31 rows");
  expect(run(4096, 3, 4096, 4096, 1, ~(size_t)0 / 2 + 1, 1, 1) == TN_EINVAL, "a batch whose double wraps");
  // byte by byte: c's batch * 2 rows against a's batch * 2 rows and against the set's 2 * terms rows
  for (size_t batch = 1; batch <= 2; ++batch)
    for (size_t terms = 1; terms <= 2; ++terms)
      for (int which = 0; which < 2; ++which)
        for (long off = -5 * (long)row; off <= 9 * (long)row; off += (long)row / 2) {
          const size_t in_rows = which == 0 ? batch * 2 : 2 * terms;
          const uintptr_t out = base + off;
          const bool want = out < base + in_rows * row && base < out + batch * 2 * row;
          const int st = which == 0 ? run(base, 3, far, out, 1, batch, terms) : run(far, 3, base, out, 1, batch, terms);
          expect(st == (want ? (int)TN_EINVAL : 0), "overlap is the intersection of the byte ranges");
        }
}

}  // namespace

void galoisks_cases() {
  const uint64_t q60 = 1152921504606830593ull, psi4096 = 431606828070683274ull;
  stepping_cases(256, 8380417, 1239911);
  stepping_cases(256, q60, h_powmod(psi4096, 16, q60));
  stepping_cases(4096, q60, psi4096);
  api_cases();
}
#endif
