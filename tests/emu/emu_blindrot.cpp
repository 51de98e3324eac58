// emu_blindrot.cpp — TEST INFRASTRUCTURE: steps the blind-rotation kernel (polydot_blindrot_kernel:
// tiny_ntt_amd/csrc/kernels_blindrot.hip) on the CPU, one emulated thread at a time, with the Stepper of emu_stepper.h and
// the headers the gfx950 kernel is compiled from (fused_core.h, cmux_core.h, launch_plan.h).  One emulated workgroup takes the
// rows in turn, as a persistent workgroup does, with the accumulator in an LDS image of two rows that lives across steps AND
// rows: the first row is loaded before the loop, a later row where the last step of the row before it would write its result
// back.  Every loop over the threads below ends where the kernel has a workgroup barrier (or, in a workgroup of one wave, where
// program order stands for it); between two barriers the threads run one after the other, so a write-back placed in front of
// another thread's rotated read of the same step changes the result.  On top of that every word of the image carries the step
// it was written for, and each read and write checks it (code 9): a rotated or own read of step k must see a word written for
// step k, a write-back of step k comes only when all 2 n rotated reads of step k have happened.
// Also the entry point's argument list (csrc/api_checks.h: check_blind_rotate) and the LDS rule (launch_plan.h) for the CPU.
// Part of tests/emu/_build/libemu.so (tests/test_blindrot_emu.py, tests/test_gpu_blindrot.py); with -DEMU_SANITIZE_CASES its
// cases for tests/emu/sanitize_driver.cpp (make sanitize).
#include "emu_stepper.h"
#include "../../tiny_ntt_amd/csrc/cmux_core.h"
#include <string>

namespace {

// a, c: [batch][2][n]; exps: [steps][batch]; bhat: [steps][2][2][terms][n]
template <typename Sh, bool BC>
int polydot_blindrot_emu(const HostTables& t, const u64* a, const u32* exps, const u64* bhat, u64* c, size_t batch, size_t steps, size_t terms,
                         u32 base_log, bool balanced) {
  typedef typename Sh::E E;
  constexpr int LOGN = Sh::LOGN;
  typedef Policy<E, Sh::LAZY> Pol;
  typedef Stepper<E, LOGN, Sh::LPT, Pol, BC> S;
  typedef typename S::Cfg Cfg;
  if (!blindrot_lds_fits<Sh>()) return 8;
  constexpr u32 EMASK = 2u * (u32)Cfg::N - 1u, NMASK = (u32)Cfg::N - 1u, N = (u32)Cfg::N;
  const FusedProductSetup<E> su = fused_product_setup(h_make_arith<E>(t), BC, false);
  S wg{su.ar};
  const typename S::Table fwd(t, su.fwd), inv(t, su.inv);
  std::vector<typename S::Regs> xw(S::T), acc0(S::T), acc1(S::T);
  std::vector<typename S::Regs>* const sums[2] = {&acc0, &acc1};
  std::vector<u32> carries(S::T);
  std::vector<E> lds_acc(2 * (size_t)N);                       // the accumulator: component o at [o * N]
  std::vector<u32> written_for(2 * (size_t)N);                 // the step each word was written for (a row's load: step 0)
  size_t rotated_reads[2] = {0, 0};                            // of the current step, per component
  int hazard = 0;
  const size_t comp = 2 * terms;                               // prepared rows of one component of a key
  auto own = [](u32 tau, int r) { return (u32)r * Cfg::THREADS + tau; };     // phase 0: the words thread tau owns
  auto load_row = [&](size_t row, u32 o, u32 tau) {            // raw words of a[row][o] into the words the thread owns
    for (int r = 0; r < Cfg::R; ++r) {
      lds_acc[o * N + own(tau, r)] = (E)a[((row * 2 + o) << LOGN) + own(tau, r)];
      written_for[o * N + own(tau, r)] = 0;
    }
  };
  if (batch)
    for (u32 o = 0; o < 2; ++o)
      for (u32 tau = 0; tau < S::T; ++tau) load_row(0, o, tau);
  for (size_t row = 0; row < batch; ++row) {
    const size_t next = row + 1 < batch ? row + 1 : row;       // after the last row this row's words are read again and dropped
    for (size_t k = 0; k < steps; ++k) {
      // ---- __syncthreads(): the top of a step ----
      const bool last = k + 1 == steps;
      const u32 e = exps[k * batch + row] & EMASK;             // the kernel's scalar
      const size_t key = k * 2 * comp;
      rotated_reads[0] = rotated_reads[1] = 0;
      for (u32 tau = 0; tau < S::T; ++tau)
        for (int r = 0; r < Cfg::R; ++r) { acc0[tau].x[r] = 0; acc1[tau].x[r] = 0; }      // once per step
      size_t term = 0;                                         // i * terms + j
      for (u32 i = 0; i < 2; ++i) {
        for (u32 tau = 0; tau < S::T; ++tau) {                 // put_away
          const u32 t0 = (tau - e) & EMASK;
          for (int r = 0; r < Cfg::R; ++r) {
            const u32 v = t0 + (u32)r * Cfg::THREADS;
            const u32 at_own = i * N + own(tau, r), at_rot = i * N + (v & NMASK);
            if (written_for[at_own] != (u32)k || written_for[at_rot] != (u32)k) hazard = 9;
            ++rotated_reads[i];
            xw[tau].x[r] = cmux_word<E, Pol>(lds_acc[at_own], lds_acc[at_rot], monomial_negated(v, LOGN), wg.ar);
          }
          carries[tau] = 0;                                    // carries never run from one polynomial into the next
        }
        for (size_t j = 0; j < terms; ++j, ++term) {
          const size_t boff[2] = {key + term, key + comp + term};
          gadget_term_step(wg, fwd, xw, carries, j, base_log, balanced, bhat, 2, boff, sums);      // (barriers inside)
        }
      }
      for (u32 o = 0; o < 2; ++o) {
        std::vector<typename S::Regs>& acc = *sums[o];
        wg.inverse(acc, inv);                                  // (barriers inside: every rotated read of the step lies before them)
        for (u32 tau = 0; tau < S::T; ++tau) {
          if (rotated_reads[0] != N || rotated_reads[1] != N) hazard = 9;      // hazard (1)
          for (int r = 0; r < Cfg::R; ++r) {                   // the add-in from the thread's own words
            if (written_for[o * N + own(tau, r)] != (u32)k) hazard = 9;
            acc[tau].x[r] = cmux_add_in<E, Pol>(acc[tau].x[r], lds_acc[o * N + own(tau, r)], wg.ar);
          }
          if (last) {                                          // to c; the next row's words take the place of the write-back
            for (int r = 0; r < Cfg::R; ++r) c[((row * 2 + o) << LOGN) + own(tau, r)] = acc[tau].x[r];
            load_row(next, o, tau);
          } else {
            for (int r = 0; r < Cfg::R; ++r) {
              lds_acc[o * N + own(tau, r)] = acc[tau].x[r];
              written_for[o * N + own(tau, r)] = (u32)k + 1;
            }
          }
        }
      }
    }
  }
  return hazard;
}

}  // namespace

extern "C" {

// acc = a[r]; for k < steps: acc[o] = acc[o] + sum_{i < 2} sum_{j < terms} digit_j((X^e - 1) acc[i]) * b[k][o][i][j], e = exps[k][r];
// c[r] = acc: the kernel's flow.  0 ok, 2 bad params, 3 a NULL a / exps or steps == 0, 4 what the gadget calls refuse (terms,
// base_log, flags), 7 unsupported n, 8 a shape whose LDS request does not fit (blindrot_lds_fits), 9 an access to the
// accumulator image out of its order.  Words travel as uint64 regardless of lane width.  canonical: the canonical policy
// (TN_PLAN_FORCE_CANONICAL).  flags: bit 0 = balanced digits.  c may be a.
int emu_poly_blind_rotate_prepared(uint32_t n, uint64_t q, uint64_t psi, int canonical, const uint64_t* a, const uint32_t* exps, const uint64_t* bhat,
                                   uint64_t* c, size_t batch, size_t steps, size_t terms, uint32_t base_log, uint32_t flags) {
  if (!a || !exps || steps == 0) return 3;
  if (!params_ok(n, q, psi)) return 2;
  const HostTables t = h_build_tables(n, q, psi, !(canonical & 1));
  if (!gadget_ok(t, terms, base_log, flags)) return 4;
  const bool bal = (flags & 1u) != 0;
  return emu_with_shape(t, [&](auto sh, auto bc) {
    return polydot_blindrot_emu<decltype(sh), decltype(bc)::value>(t, a, exps, bhat, c, batch, steps, terms, base_log, bal);
  });
}

// The LDS rule of launch_plan.h for a plan's (n, elem_bytes, lazy): *bytes receives the workgroup's request and *words the
// input words per thread put away (0 and 0 where no fused kernel is built for n).  Returns 1 when the shape is supported.
int emu_blindrot_lds_fits(uint32_t n, int elem_bytes, int lazy, size_t* bytes, int* words) {
  u32 logn = 0;
  while ((1ull << logn) < n) ++logn;
  if (bytes) *bytes = 0;
  if (words) *words = 0;
  if (((u64)1 << logn) != n) return 0;
  with_fused_shape(elem_bytes, lazy != 0, logn, 0, [&](auto sh) {
    typedef decltype(sh) Sh;
    if (words) *words = blindrot_lds_words<Sh>();
    if (bytes) *bytes = blindrot_lds_bytes<Sh>(blindrot_lds_words<Sh>());
    return 0;
  });
  return blindrot_supported(elem_bytes, lazy != 0, logn) ? 1 : 0;
}

// The argument checks of the entry point (api_checks.h: check_blind_rotate, the list capi.cpp runs) on a plan view made of
// (n, elem_bytes, has_fused, omega_only, q, lazy); n == 0 is a NULL plan.  No pointer is read.  Returns the status; *launch = 1
// when the call would go on to its launch; msg receives the text tn_last_error would give.
int emu_blindrot_api_check(uint32_t n, int elem_bytes, int has_fused, int omega_only, uint64_t q, int lazy, const void* a, const void* exps,
                           const void* bhat, const void* c, size_t batch, size_t comps, size_t steps, size_t terms, uint32_t base_log, uint32_t flags,
                           int* launch, char* msg, size_t msg_len) {
  ApiCheck k{ApiPlan{n, elem_bytes, has_fused != 0, omega_only != 0, q, lazy != 0}, "tn_poly_blind_rotate_prepared_dev"};
  return api_answer(k, check_blind_rotate(k, a, exps, bhat, c, batch, comps, steps, terms, base_log, flags), launch, msg, msg_len);
}

}  // extern "C"

#ifdef EMU_SANITIZE_CASES
#include "sanitize_cases.h"
// The cases sanitize_driver.cpp runs (blindrot_cases): the stepping at the smallest shape of either lane width and at the base-case
// shape, both policies, batch 5 (one workgroup takes all five rows: four reloads of the accumulator), 3 steps x 2 terms, both
// digit modes, in place and out of place, with the exponents 0, 1, n, 2n - 1 and an unreduced one in step 0 and others behind.
// Properties that need no second implementation of the transforms: keys of zero rows return a mod q; exponents of 0 return a
// mod q whatever the keys; and three steps from one call equal three calls of one step each, where the accumulator goes
// through memory.  Then the LDS rule and the argument list on made-up addresses.
namespace {

void stepping_cases(uint32_t n, uint64_t q, uint64_t psi) {
  const size_t batch = 5, terms = 2, steps = 3;
  uint64_t lcg = 88172645463325252ull ^ q;
  auto rnd = [&]() { lcg = lcg * 6364136223846793005ull + 1442695040888963407ull; return lcg; };
  const uint32_t w = (uint32_t)((64 - __builtin_clzll(q)) + 1) / 2;
  std::vector<uint32_t> exps = {0u, 1u, n, 2 * n - 1, 0x80000000u + 2 * n + 3};
  for (size_t x = batch; x < steps * batch; ++x) exps.push_back((uint32_t)(rnd() >> 32));
  const std::vector<uint32_t> none(steps * batch, 2 * n);                       // 2n is 0
  const size_t key = 4 * terms * n;
  std::vector<uint64_t> a(batch * 2 * n), b(steps * key), zero(steps * key, 0);
  std::vector<uint64_t> c0(batch * 2 * n), c1(batch * 2 * n), c2(batch * 2 * n);
  for (auto& v : a) v = q < ((uint64_t)1 << 31) ? (rnd() >> 32) : rnd();        // any word of the lane
  for (auto& v : b) v = rnd() % q;
  a[0] = q - 1; a[1] = q; a[2] = 0;
  for (int canonical = 0; canonical < 2; ++canonical)
    for (uint32_t flags = 0; flags < 2; ++flags) {
      expect(emu_poly_blind_rotate_prepared(n, q, psi, canonical, a.data(), exps.data(), zero.data(), c0.data(), batch, steps, terms, w, flags) == 0, "runs");
      bool same = true;
      for (size_t x = 0; x < c0.size(); ++x) same = same && c0[x] == a[x] % q;
      expect(same, "keys of zero rows return a mod q");
      expect(emu_poly_blind_rotate_prepared(n, q, psi, canonical, a.data(), none.data(), b.data(), c0.data(), batch, steps, terms, w, flags) == 0, "runs");
      same = true;
      for (size_t x = 0; x < c0.size(); ++x) same = same && c0[x] == a[x] % q;
      expect(same, "exponents of 0 return a mod q");
      expect(emu_poly_blind_rotate_prepared(n, q, psi, canonical, a.data(), exps.data(), b.data(), c0.data(), batch, steps, terms, w, flags) == 0, "runs");
      // step by step through memory, two alternating buffers
      const uint64_t* src = a.data();
      for (size_t k = 0; k < steps; ++k) {
        uint64_t* dst = (k & 1) ? c2.data() : c1.data();
        expect(emu_poly_blind_rotate_prepared(n, q, psi, canonical, src, exps.data() + k * batch, b.data() + k * key, dst, batch, 1, terms, w, flags) == 0, "runs");
        src = dst;
      }
      same = true;
      for (size_t x = 0; x < c0.size(); ++x) same = same && c0[x] == src[x] && c0[x] < q;
      expect(same, "three steps from one call are three calls of one step");
      // in place
      c2 = a;
      expect(emu_poly_blind_rotate_prepared(n, q, psi, canonical, c2.data(), exps.data(), b.data(), c2.data(), batch, steps, terms, w, flags) == 0, "runs");
      expect(c2 == c0, "in place gives the bits of the out-of-place call");
    }
}

void lds_cases() {
  for (int elem_bytes : {4, 8})
    for (int lazy = 0; lazy < 2; ++lazy)
      for (uint32_t logn = 7; logn <= 14; ++logn) {
        size_t bytes = 1;
        int words = -1;
        const int fits = emu_blindrot_lds_fits(1u << logn, elem_bytes, lazy, &bytes, &words);
        const bool built = logn >= 8 && logn <= 13;
        expect((fits != 0) == (built && !(logn == 13 && elem_bytes == 8)), "only n = 8192 with 64-bit words is over the limit");
        expect(built ? (bytes > 2 * ((size_t)elem_bytes << logn) && (fits != 0) == (bytes <= 160 * 1024)) : bytes == 0, "the request holds two rows and is compared with 160 KiB");
        expect(built ? (words >= 0 && words <= 8) : words == 0, "words put away per thread");
      }
}

void api_cases() {
  constexpr uint32_t n = 256;
  constexpr uint64_t q = 8380417;
  const uintptr_t row = n * 4, base = 1 << 24, far = (uintptr_t)1 << 40, ex = (uintptr_t)1 << 44;
  auto at = [](uintptr_t x) { return reinterpret_cast<const void*>(x); };
  std::string text;
  auto run = [&](uintptr_t a, uintptr_t e, uintptr_t b, uintptr_t c, size_t batch, size_t comps, size_t steps, size_t terms, uint32_t w = 4, uint32_t flags = 0,
                 int fused = 1, uint32_t n_ = 256, int word = 4) {
    int launch = -1;
    char msg[256];
    const int st = emu_blindrot_api_check(n_, word, fused, 0, q, 1, at(a), at(e), at(b), at(c), batch, comps, steps, terms, w, flags, &launch, msg, sizeof msg);
    text = msg;
    return st == TN_OK ? (launch ? 0 : -1) : st;
  };
  expect(run(base, ex, far, 2 * far, 3, 2, 4, 2) == 0, "ok");
  expect(run(base, ex, far, base, 3, 2, 4, 2) == 0, "in place ok");
  expect(run(base, ex, far, 2 * far, 3, 0, 4, 2) == TN_EINVAL, "comps 0");
  expect(run(base, ex, far, 2 * far, 3, 1, 4, 2) == TN_EUNSUPPORTED, "comps 1");
  expect(run(base, ex, far, 2 * far, 3, 3, 4, 2) == TN_EUNSUPPORTED, "comps 3");
  expect(run(base, ex, far, 2 * far, 3, 2, 0, 2) == TN_EINVAL, "steps 0");
  expect(run(base, ex, far, 2 * far, 3, 2, 4, 0) == TN_EINVAL, "terms 0");
  expect(run(base, ex, far, 2 * far, 3, 2, 4, 2, 4, 0, 0) == TN_EUNSUPPORTED, "no fused kernels");
  expect(run(base, ex, far, 2 * far, 3, 2, 4, 2, 4, 0, 1, 8192, 8) == TN_EUNSUPPORTED && text.find("tn_poly_cmux_rotate_prepared_dev") != std::string::npos,
         "n = 8192 with 64-bit words names the loop");
  expect(run(base, ex, far, 2 * far, 3, 2, 4, 2, 4, 0, 1, 8192, 4) == 0, "n = 8192 with 32-bit words ok");
  expect(run(base, ex, far, 2 * far, 0, 2, 4, 2) == -1, "batch 0 launches nothing");
  expect(run(base, 0, far, 2 * far, 3, 2, 4, 2) == TN_EINVAL, "NULL exps");
  expect(run(4096, 4096, 4096, 4096, 1, 2, (size_t)1 << 29, 1, 1) == TN_EINVAL && text.find("steps * 4 * terms") != std::string::npos, "2^31 key rows");
  expect(run(4096, 4096, 4096, 4096, (size_t)1 << 30, 2, 1, 1, 1) == TN_EINVAL && text.find("batch * 2") != std::string::npos, "2^31 accumulator rows");
  expect(run(4096, 4096, 4096, 4096, (size_t)1 << 16, 2, (size_t)1 << 15, 1, 1) == TN_EINVAL && text.find("steps * batch") != std::string::npos, "2^31 exponents");
  expect(run(4096, 4096, 4096, 4096, ~(size_t)0 / 2 + 1, 2, 1, 1, 1) == TN_EINVAL, "a batch whose double wraps");
  // byte by byte: c's batch * 2 rows against a's batch * 2 rows (the same pointer excepted) and against the steps * 4 * terms key rows
  for (size_t batch = 1; batch <= 2; ++batch)
    for (int which = 0; which < 2; ++which)
      for (long off = -5 * (long)row; off <= 26 * (long)row; off += (long)row / 2) {
        const size_t terms = 2, steps = 3, in_rows = which == 1 ? steps * 4 * terms : batch * 2;
        const uintptr_t out = base + off;
        const bool want = out < base + in_rows * row && base < out + batch * 2 * row && !(which == 0 && off == 0);
        const int st = which == 0 ? run(base, ex, far, out, batch, 2, steps, terms) : run(far, ex, base, out, batch, 2, steps, terms);
        expect(st == (want ? (int)TN_EINVAL : 0), "overlap is the intersection of the byte ranges, c == a excepted");
      }
}

}  // namespace

void blindrot_cases() {
  const uint64_t q60 = 1152921504606830593ull, psi4096 = 431606828070683274ull;
  stepping_cases(256, 8380417, 1239911);
  stepping_cases(256, q60, h_powmod(psi4096, 16, q60));
  stepping_cases(4096, q60, psi4096);
  lds_cases();
  api_cases();
}
#endif
