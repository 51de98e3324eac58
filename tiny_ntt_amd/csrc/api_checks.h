// api_checks.h — the argument checks of the device entry points (capi.cpp), free of HIP: arithmetic on a small view of the
// plan and on the call's sizes and pointers, so tests/emu runs them on the CPU.  A step returns true when the call goes on;
// when it returns false, st and msg are the call's answer (st == TN_OK: nothing to do).  Each entry point is one ordered
// list of steps below; that order is behaviour of the C ABI: it decides which status and text a call with several faults gets.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string>
#include "../../include/tinyntt.h"
#include "launch_plan.h"

namespace tn {

// (lazy: the plan's policy, which names its fused shape together with n and elem_bytes; only check_blind_rotate asks)
struct ApiPlan { uint32_t n; int elem_bytes; bool has_fused, omega_only; uint64_t q; bool lazy = false; };     // a NULL plan: n == 0

// what the LWE key switch's kernel holds (lwe_core.h): digits as 32-bit words; 128-bit sums of n_in * terms terms below 2^32 2^64
constexpr size_t LWE_KS_MAX_SLOTS = (size_t)1 << 22;
constexpr uint32_t LWE_KS_MAX_BASE_LOG = 32;

// What the prepared key switch holds (lwe_mfma_core.h: signed bytes into the int8 matrix instruction, exact 32-bit sums).
//   Digits are signed bytes: unsigned digits of base_log <= 7, balanced ones of base_log <= 8.
//   A key word is L(q) balanced base-256 limbs in [-128, 128) of its centred residue in (-q/2, q/2]; L limbs hold the values
//   -128 (256^L - 1) / 255 .. 127 (256^L - 1) / 255, so L(q) is the smallest L with floor(q / 2) <= 127 (256^L - 1) / 255 (the
//   negative side has one value to spare): 3 for q = 8380417, 8 for q = 2^60 - 2^14 + 1, at most 4 below 2^31 and 8 below 2^62.
//   A product is at most 2^14 in magnitude, so a 32-bit sum takes LWE_MFMA_FLUSH_PRODUCTS = 2^16 of them (2^30) before it is
//   folded into a 128-bit partial sum_l acc_l 2^(8 l), below 2^88; n_in * terms <= LWE_KS_MAX_SLOTS = 2^22 is 2^6 folds: the
//   total is below 2^94 (2^61 on 32-bit lanes, L <= 4), and |total| <= 2^22 * 128 * q / 2 as a sum of digits times centred residues.
//   The prepared key: limb planes in the matrix instruction's B-fragment order, [column tile of 16][K step of 64][limb][lane of 64][16 bytes],
//   K = n_in * terms and the columns n_out + 1 padded to whole tiles with zero limbs.
constexpr uint32_t LWE_MFMA_K_STEP = 64, LWE_MFMA_COL_TILE = 16, LWE_MFMA_FRAG_BYTES = 64 * 16;
constexpr uint32_t LWE_MFMA_FLUSH_PRODUCTS = 1u << 16;
static inline uint32_t lwe_mfma_limbs(uint64_t q) {
  const unsigned __int128 half = q >> 1;
  unsigned __int128 span = 1;                                    // (256^L - 1) / 255
  uint32_t limbs = 1;
  while (half > 127 * span) { span = span * 256 + 1; ++limbs; }
  return limbs;
}
static constexpr size_t lwe_mfma_steps(size_t n_in, size_t terms) { return (n_in * terms + LWE_MFMA_K_STEP - 1) / LWE_MFMA_K_STEP; }
static constexpr size_t lwe_mfma_col_tiles(size_t n_out) { return (n_out + 1 + LWE_MFMA_COL_TILE - 1) / LWE_MFMA_COL_TILE; }
// at most 4097 * 65536 * 8 KiB: no step wraps size_t for arguments within check_lwe_ksk_prepare's limits
static inline size_t lwe_mfma_prepared_bytes(uint64_t q, size_t n_in, size_t n_out, size_t terms) {
  return lwe_mfma_col_tiles(n_out) * lwe_mfma_steps(n_in, terms) * lwe_mfma_limbs(q) * LWE_MFMA_FRAG_BYTES;
}

struct KernelPick { bool known, fused; int group, layout; };     // layout: CgLayout, cg_core.h (0 linear, 1 padded, 2 swizzled)
// The kernel a variant names; TN_VARIANT_AUTO is the fused kernel where the plan has it (and no trace is wanted), else CG.
static inline KernelPick pick_kernel(const ApiPlan& v, tn_variant variant, bool trace = false) {
  static const signed char cg[][2] = {{1, 0}, {8, 0}, {8, 1}, {1, 2}, {8, 2}, {2, 0}, {2, 1}, {2, 2}, {4, 0}, {4, 1}, {4, 2}};   // TN_VARIANT_CG ...
  if (variant == TN_VARIANT_AUTO) variant = (v.has_fused && !trace) ? TN_VARIANT_FUSED : TN_VARIANT_CG;
  if (variant == TN_VARIANT_FUSED) return {true, true, 0, 0};
  if (variant < TN_VARIANT_CG || variant > TN_VARIANT_CG4_SWIZZLED) return {false, false, 0, 0};
  return {true, false, cg[variant - TN_VARIANT_CG][0], cg[variant - TN_VARIANT_CG][1]};
}

struct __attribute__((visibility("hidden"))) ApiCheck {          // (hidden, static: the library exports the C ABI alone)
  ApiPlan v;
  const char* fn;
  tn_status st = TN_OK;
  std::string msg;
  ApiCheck(const ApiPlan& view, const char* name) : v(view), fn(name) {}
  bool fail(tn_status s, const char* what, bool named = true) {
    st = s; msg = named ? std::string(fn) + ": " + what : std::string(what);
    return false;
  }
  bool plan() { return v.n || fail(TN_EINVAL, "plan is NULL"); }
  bool arguments(bool present) { return present || fail(TN_EINVAL, "NULL argument"); }
  bool fused() { return v.has_fused || fail(TN_EUNSUPPORTED, "prepared operands need a plan with the fused kernels (tn_plan_has_fused)"); }
  bool psi(const char* why) { return !v.omega_only || fail(TN_EUNSUPPORTED, why); }
  bool terms(size_t terms) { return terms || fail(TN_EINVAL, "terms must be at least 1"); }
  // the kernels index rows with 32 bits; the division keeps batch * terms from wrapping size_t first
  bool rows(size_t batch, size_t terms, const char* count, const char* noun) {
    const size_t max = 0x7fffffffull;
    return !(batch > max || terms > max || (batch && terms > max / batch)) ||
           fail(TN_EINVAL, (std::string(count) + " too large for one call (max 2^31 - 1 " + noun + ")").c_str());
  }
  bool rows_wide(size_t batch) { return batch <= 0xffffffffull || fail(TN_EINVAL, "batch too large"); }      // grid-stride kernels
  bool work(size_t batch) { return batch != 0; }                                              // batch 0: TN_OK, nothing launched
  bool buffers(bool present) { return present || fail(TN_EINVAL, "NULL buffer"); }
  bool sets(size_t sets, size_t batch, const char* name, const char* one) {
    return sets == 1 || sets == batch || fail(TN_EINVAL, (std::string(name) + " must be 1 (" + one + ") or batch").c_str());
  }
  bool out_prepared(int flag) { return flag == 0 || flag == 1 || fail(TN_EINVAL, "out_prepared must be 0 (coefficients) or 1 (prepared rows)"); }
  // what both gadget calls ask: terms >= 1, known flags, 0 < base_log, 2^base_log < q, no shift reaches the word width
  bool gadget(size_t batch, size_t terms_, uint32_t base_log, uint32_t flags, const char* count = "batch * terms", const char* noun = "digit rows") {
    if (!terms(terms_)) return false;
    if (flags & ~(uint32_t)TN_GADGET_BALANCED) return fail(TN_EINVAL, "unknown flag bit");
    if (base_log == 0 || base_log >= 64 || (((uint64_t)1) << base_log) >= v.q) return fail(TN_EINVAL, "need 1 <= base_log and 2^base_log < q");
    if (terms_ - 1 > 63 / base_log) return fail(TN_EINVAL, "(terms - 1) * base_log must be below 64");
    return rows(batch, terms_, count, noun);
  }
  // output components of tn_poly_gadget_multidot_prepared_dev: one runs the gadget kernel, two the kernel built for them
  bool outs(size_t outs_) {
    if (!outs_) return fail(TN_EINVAL, "outs must be at least 1");
    return outs_ <= 2 || fail(TN_EUNSUPPORTED, "more than 2 output components are not supported");
  }
  // input polynomials of tn_poly_external_product_prepared_dev: one is the multidot call; two or more run the kernel built for
  // two output components
  bool ins(size_t ins_) { return ins_ || fail(TN_EINVAL, "ins must be at least 1"); }
  bool ins_outs(size_t ins_, size_t outs_) {
    return !(ins_ >= 2 && outs_ == 1) ||
           fail(TN_EUNSUPPORTED, "2 or more input polynomials into 1 output component are not supported (tn_gadget_decompose_dev, then tn_poly_dot_prepared_dev)");
  }
  // components of the accumulator of tn_poly_cmux_rotate_prepared_dev: the kernel has two output components
  bool comps(size_t comps_) {
    if (!comps_) return fail(TN_EINVAL, "comps must be 2");
    return comps_ == 2 || fail(TN_EUNSUPPORTED, "comps other than 2 is not supported (tn_monomial_mul_dev, tn_poly_external_product_prepared_dev, then an addition)");
  }
  // tn_poly_blind_rotate_prepared_dev: the steps; the shape, whose LDS request must fit a workgroup (launch_plan.h:
  // blindrot_supported); and c == a, the same pointer, as the one overlap of the two that is allowed
  bool steps(size_t steps_) { return steps_ || fail(TN_EINVAL, "steps must be at least 1"); }
  bool blindrot_shape() {
    uint32_t logn = 0;
    while ((1ull << logn) < v.n) ++logn;
    return blindrot_supported(v.elem_bytes, v.lazy, logn) ||
           fail(TN_EUNSUPPORTED, "the accumulator of this shape does not fit a workgroup's LDS (loop over tn_poly_cmux_rotate_prepared_dev)");
  }
  bool apart_or_same(const void* out, const void* in, size_t rows_) {
    const uintptr_t o = (uintptr_t)out, i = (uintptr_t)in, bytes = rows_ * (uintptr_t)v.n * (uintptr_t)v.elem_bytes;
    return o == i || !(o < i + bytes && i < o + bytes) || fail(TN_EINVAL, "c may be a itself (in place) but must not overlap it otherwise");
  }
  // rows per batch item and flags of tn_monomial_mul_dev
  bool group(size_t group_) { return group_ || fail(TN_EINVAL, "group must be at least 1"); }
  bool monomial_flags(uint32_t flags) { return !(flags & ~(uint32_t)TN_MONOMIAL_MINUS_ONE) || fail(TN_EINVAL, "unknown flag bit"); }
  // Galois elements of the automorphism calls: 1 .. TN_GALOIS_MAX of them, each odd and below 2n.  A NULL list is the
  // buffer check's to refuse (behind batch == 0).
  bool galois(const uint32_t* g, size_t count) {
    if (count < 1 || count > TN_GALOIS_MAX) return fail(TN_EINVAL, "count must be between 1 and TN_GALOIS_MAX (16)");
    for (size_t m = 0; g && m < count; ++m)
      if (!(g[m] & 1u) || g[m] >= 2 * (uint64_t)v.n)
        return fail(TN_EINVAL, ("galois[" + std::to_string(m) + "] = " + std::to_string(g[m]) + " is not an odd element below 2n").c_str());
    return true;
  }
  // The rotation of tn_poly_pack_step_prepared_dev: below 2n; the trace step (no od) has nothing to rotate
  bool pack_rot(uint32_t rot, bool has_od) {
    if (rot >= 2 * (uint64_t)v.n) return fail(TN_EINVAL, ("rot = " + std::to_string(rot) + " is not below 2n").c_str());
    return has_od || rot == 0 || fail(TN_EINVAL, "rot must be 0 when od is NULL (the trace step)");
  }
  // The byte ranges of out_rows rows at out and in_rows rows at in share no byte: the kernels prefetch the next row's input
  // while a row's result is being stored.  Compared as integers: a caller may pass any address, also one near 0.
  bool apart(const void* out, size_t out_rows, const void* in, size_t in_rows, const char* noun) {
    const uintptr_t o = (uintptr_t)out, i = (uintptr_t)in, row = (uintptr_t)v.n * (uintptr_t)v.elem_bytes;
    return !(o < i + in_rows * row && i < o + out_rows * row) || fail(TN_EINVAL, (std::string("output must not alias or overlap ") + noun).c_str());
  }
  // The LWE calls (tn_lwe_modswitch_dev, tn_sample_extract_dev, tn_lwe_keyswitch_dev): a dimension is 1 .. TN_LWE_MAX_DIM; the
  // extracted coefficient lies in the row; the key switch keeps digits as 32-bit words and sums of n_in * terms terms, each
  // below 2^32 2^64, in 128 bits: 2^22 of them stay below 2^118 (LWE_KS_MAX_SLOTS, LWE_KS_MAX_BASE_LOG above).  With
  // TN_LWE_MAX_DIM = 2^16 and the gadget rule's terms <= 64 no call reaches lwe_sum's bound today: it stands for the day either grows.
  bool lwe_dim(size_t d, const char* name) {
    return (d >= 1 && d <= TN_LWE_MAX_DIM) || fail(TN_EINVAL, (std::string(name) + " must be between 1 and TN_LWE_MAX_DIM (65536)").c_str());
  }
  bool lwe_index(uint32_t index) { return index < v.n || fail(TN_EINVAL, "index must be below n"); }
  bool lwe_digits(uint32_t base_log) {
    return base_log <= LWE_KS_MAX_BASE_LOG ||
           fail(TN_EUNSUPPORTED, "base_log above 32 is not supported: the kernel keeps digits as 32-bit words (LWE key switches use bases of 2^2 to 2^8)");
  }
  bool lwe_sum(size_t n_in, size_t terms_) {
    return n_in * terms_ <= LWE_KS_MAX_SLOTS ||
           fail(TN_EUNSUPPORTED, "n_in * terms above 2^22 is not supported: a 128-bit sum holds 2^22 terms below 2^32 * 2^64");
  }
  // The prepared key switch (tn_lwe_ksk_prepared_bytes, tn_lwe_ksk_prepare_dev, tn_lwe_keyswitch_prepared_dev) under the same
  // lwe_sum: its sum of signed digits (magnitude <= 128) times centred residues (magnitude <= q / 2) is |sum| <= 2^22 * 128 * q / 2,
  // held as 32-bit sums of at most LWE_MFMA_FLUSH_PRODUCTS byte products folded into 128 bits (the bounds stand at the top of this file).
  bool lwe_byte_digits(uint32_t base_log, uint32_t flags) {
    return base_log <= ((flags & TN_GADGET_BALANCED) ? 8u : 7u) ||
           fail(TN_EUNSUPPORTED, "digits wider than a signed byte are not supported (unsigned base_log <= 7, TN_GADGET_BALANCED base_log <= 8): "
                                 "tn_lwe_keyswitch_dev is the route");
  }
  bool lwe_key_terms(size_t n_in, size_t terms_) {           // what gadget() asks of terms, without a base: 1 .. 64, n_in * terms key rows
    if (!terms(terms_)) return false;
    if (terms_ > 64) return fail(TN_EINVAL, "terms must be at most 64");
    return rows(n_in, terms_, "n_in * terms", "key rows");
  }
  bool aligned16(const void* kprep) {                         // the kernel loads a lane's B fragment as one 16-byte word
    return ((uintptr_t)kprep & 15u) == 0 || fail(TN_EINVAL, "kprep must be aligned to 16 bytes");
  }
  // byte ranges of buffers that are not rows of n words
  bool apart_bytes(const void* out, size_t out_bytes, const void* in, size_t in_bytes, const char* noun) {
    const uintptr_t o = (uintptr_t)out, i = (uintptr_t)in;
    return !(o < i + in_bytes && i < o + out_bytes) || fail(TN_EINVAL, (std::string("output must not alias or overlap ") + noun).c_str());
  }
  // tn_poly_mult_dev words these two without its name (named = false)
  bool kernel(const KernelPick& k, bool trace, bool named = true) {
    if (!k.known) return fail(TN_EINVAL, "unknown variant", named);
    if (k.fused && !v.has_fused) return fail(TN_EUNSUPPORTED, "fused kernel not built for this n; use TN_VARIANT_CG", named);
    // register-tiled kernel: same results, no per-stage trace (its internal stages are not the CG stages)
    return !(k.fused && trace) || fail(TN_EUNSUPPORTED, "per-stage traces need a CG variant");
  }
};

// ---- one list per entry point (entry points with the same list share it) ----------------------
// c = f(a, b) row by row, or out = f(in) given as a == b: schoolbook, the *_host calls, and the head of the next three
static inline bool check_rows(ApiCheck& k, const void* a, const void* b, const void* c, size_t batch) {
  return k.plan() && k.rows(batch, 1, "batch", "rows") && k.buffers(!batch || (a && b && c)) &&
         k.apart(c, batch, a, batch, "an input") && k.apart(c, batch, b, batch, "an input");
}
static inline bool check_product(ApiCheck& k, const void* a, const void* b, const void* c, size_t batch, bool cyclic) {
  return check_rows(k, a, b, c, batch) &&
         k.psi(cyclic ? "not available on an omega-only plan" : "an omega-only plan has no psi (tn_plan_create_omega offers cg_ntt / cg_intt only)");
}
static inline bool check_transform(ApiCheck& k, const void* in, const void* out, size_t batch, bool twist) {
  return check_rows(k, in, in, out, batch) && (!twist || k.psi("an omega-only plan has no psi to twist with"));
}
static inline bool check_prepare(ApiCheck& k, const void* in, const void* out, size_t rows) {            // and tn_unprepare_dev
  return check_rows(k, in, in, out, rows) && k.fused();
}
static inline bool check_mult_prepared(ApiCheck& k, const void* a, const void* bhat, size_t bhat_rows, const void* c, size_t batch) {
  return k.plan() && k.fused() && k.rows(batch, 1, "batch", "rows") && k.work(batch) && k.buffers(a && bhat && c) &&
         k.sets(bhat_rows, batch, "bhat_rows", "shared operand") && k.apart(c, batch, a, batch, "an input") &&
         k.apart(c, batch, bhat, bhat_rows, "an input");
}
// tn_poly_dot_prepared_dev (out_prepared 0, "rows of a") and tn_poly_dot_hat_dev ("rows of ahat")
static inline bool check_dot(ApiCheck& k, const void* a, const void* bhat, size_t sets, const void* out, size_t batch, size_t terms,
                      int out_prepared, const char* noun) {
  return k.plan() && k.fused() && k.terms(terms) && k.out_prepared(out_prepared) && k.rows(batch, terms, "batch * terms", noun) &&
         k.work(batch) && k.buffers(a && bhat && out) && k.sets(sets, batch, "bhat_sets", "one set of operands for every row") &&
         k.apart(out, batch, a, batch * terms, "an input") && k.apart(out, batch, bhat, sets * terms, "an input");
}
static inline bool check_gadget_decompose(ApiCheck& k, const void* a, const void* digits, size_t batch, size_t terms, uint32_t base_log, uint32_t flags) {
  return k.plan() && k.gadget(batch, terms, base_log, flags) && k.work(batch) && k.buffers(a && digits) &&
         k.apart(digits, batch * terms, a, batch, "the input");
}
static inline bool check_gadget_dot(ApiCheck& k, const void* a, const void* bhat, size_t sets, const void* c, size_t batch, size_t terms,
                             uint32_t base_log, uint32_t flags) {
  return k.plan() && k.fused() && k.gadget(batch, terms, base_log, flags) && k.work(batch) && k.buffers(a && bhat && c) &&
         k.sets(sets, batch, "bhat_sets", "one set of operands for every row") && k.apart(c, batch, a, batch, "an input") &&
         k.apart(c, batch, bhat, sets * terms, "an input");
}
// batch * outs for a row limit; a factor that is above the limit by itself stands as it is (times the other it could wrap
// size_t), unless the other is 0
static inline size_t rows_times(size_t batch, size_t outs) {
  const size_t max = 0x7fffffffull;
  if (!batch || !outs) return 0;
  return batch > max ? batch : outs > max ? outs : batch * outs;
}
// check_gadget_dot's list with the component count behind the plan's: the row limit holds for batch * outs * terms, c has
// batch * outs rows and bhat sets * outs * terms
static inline bool check_gadget_multidot(ApiCheck& k, const void* a, const void* bhat, size_t sets, const void* c, size_t batch, size_t outs,
                                         size_t terms, uint32_t base_log, uint32_t flags) {
  return k.plan() && k.fused() && k.outs(outs) &&
         k.gadget(rows_times(batch, outs), terms, base_log, flags, "batch * outs * terms") && k.work(batch) &&
         k.buffers(a && bhat && c) && k.sets(sets, batch, "bhat_sets", "one set of operands for every row") &&
         k.apart(c, batch * outs, a, batch, "an input") && k.apart(c, batch * outs, bhat, sets * outs * terms, "an input");
}
// check_gadget_multidot's list with the count of input polynomials behind the plan's: the row limit holds for
// batch * outs * ins * terms (each factor of rows_times is below 2^31 or the product stands above it: no step wraps size_t), a
// has batch * ins rows, c batch * outs and bhat sets * outs * ins * terms
static inline bool check_external_product(ApiCheck& k, const void* a, const void* bhat, size_t sets, const void* c, size_t batch, size_t ins,
                                          size_t outs, size_t terms, uint32_t base_log, uint32_t flags) {
  return k.plan() && k.fused() && k.ins(ins) && k.outs(outs) && k.ins_outs(ins, outs) &&
         k.gadget(rows_times(rows_times(batch, outs), ins), terms, base_log, flags, "batch * outs * ins * terms") && k.work(batch) &&
         k.buffers(a && bhat && c) && k.sets(sets, batch, "bhat_sets", "one set of operands for every row") &&
         k.apart(c, batch * outs, a, batch * ins, "an input") && k.apart(c, batch * outs, bhat, sets * outs * ins * terms, "an input");
}
// tn_monomial_mul_dev: out has the batch * group rows of a; exps is a device array that the host never reads.  The kernel
// gathers, so nothing runs in place.
static inline bool check_monomial(ApiCheck& k, const void* a, const void* exps, const void* out, size_t batch, size_t group, uint32_t flags) {
  return k.plan() && k.group(group) && k.monomial_flags(flags) && k.rows(batch, group, "batch * group", "rows") && k.work(batch) &&
         k.buffers(a && exps && out) && k.apart(out, batch * group, a, batch * group, "the input");
}
// tn_poly_cmux_rotate_prepared_dev: check_external_product's list with ins = outs = comps and exps among the buffers: the row
// limit holds for batch * comps * comps * terms, a and c have batch * comps rows and bhat sets * comps * comps * terms
static inline bool check_cmux_rotate(ApiCheck& k, const void* a, const void* exps, const void* bhat, size_t sets, const void* c, size_t batch,
                                     size_t comps, size_t terms, uint32_t base_log, uint32_t flags) {
  return k.plan() && k.fused() && k.comps(comps) &&
         k.gadget(rows_times(rows_times(batch, comps), comps), terms, base_log, flags, "batch * comps * comps * terms") && k.work(batch) &&
         k.buffers(a && exps && bhat && c) && k.sets(sets, batch, "bhat_sets", "one set of operands for every row") &&
         k.apart(c, batch * comps, a, batch * comps, "an input") && k.apart(c, batch * comps, bhat, sets * comps * comps * terms, "an input");
}
// tn_poly_blind_rotate_prepared_dev: check_cmux_rotate's order with the steps behind the components.  One key per step, shared
// by every row: bhat has steps * 4 * terms rows, exps steps * batch words, a and c batch * 2 rows; c may be a itself.
static inline bool check_blind_rotate(ApiCheck& k, const void* a, const void* exps, const void* bhat, const void* c, size_t batch, size_t comps,
                                      size_t steps, size_t terms, uint32_t base_log, uint32_t flags) {
  return k.plan() && k.fused() && k.blindrot_shape() && k.comps(comps) && k.steps(steps) &&
         k.gadget(rows_times(steps, 4), terms, base_log, flags, "steps * 4 * terms", "key rows") &&
         k.rows(batch, 2, "batch * 2", "accumulator rows") && k.rows(steps, batch, "steps * batch", "exponents") && k.work(batch) &&
         k.buffers(a && exps && bhat && c) && k.apart_or_same(c, a, batch * 2) && k.apart(c, batch * 2, bhat, steps * 4 * terms, "the key");
}
// tn_automorphism_dev and, with the fused() step (prepared), tn_automorphism_prepared_dev: out has batch * count rows.  The
// kernels gather, so nothing runs in place.
static inline bool check_automorphism(ApiCheck& k, const void* in, const void* out, size_t batch, const uint32_t* galois, size_t count, bool prepared) {
  return k.plan() && (!prepared || k.fused()) && k.galois(galois, count) && k.rows(batch, count, "batch * count", "output rows") &&
         k.work(batch) && k.buffers(in && out && galois) && k.apart(out, batch * count, in, batch, "the input");
}
// tn_poly_galois_keyswitch_prepared_dev: check_gadget_multidot's list with two components and the Galois element (one, by
// value) behind the plan's steps: the row limit holds for batch * 2 * terms, a and c have batch * 2 rows and bhat
// sets * 2 * terms.  The kernel permutes within a row and prefetches the next one, so nothing runs in place.
static inline bool check_galois_keyswitch(ApiCheck& k, const void* a, uint32_t galois, const void* bhat, size_t sets, const void* c, size_t batch,
                                          size_t terms, uint32_t base_log, uint32_t flags) {
  return k.plan() && k.fused() && k.galois(&galois, 1) && k.gadget(rows_times(batch, 2), terms, base_log, flags, "batch * 2 * terms") &&
         k.work(batch) && k.buffers(a && bhat && c) && k.sets(sets, batch, "bhat_sets", "one set of operands for every row") &&
         k.apart(c, batch * 2, a, batch * 2, "an input") && k.apart(c, batch * 2, bhat, sets * 2 * terms, "an input");
}
// tn_poly_pack_step_prepared_dev: check_galois_keyswitch's list with the rotation behind the element (rot below 2n; the
// trace step, od == NULL, takes rot == 0 only) and two inputs of batch * 2 rows; od is not among the buffers that must be
// present.  The kernel reads a row's inputs again after its first component is stored, so nothing runs in place.
static inline bool check_pack_step(ApiCheck& k, const void* ev, const void* od, uint32_t rot, uint32_t galois, const void* bhat, size_t sets,
                                   const void* c, size_t batch, size_t terms, uint32_t base_log, uint32_t flags) {
  return k.plan() && k.fused() && k.galois(&galois, 1) && k.pack_rot(rot, od != nullptr) &&
         k.gadget(rows_times(batch, 2), terms, base_log, flags, "batch * 2 * terms") && k.work(batch) && k.buffers(ev && bhat && c) &&
         k.sets(sets, batch, "bhat_sets", "one set of operands for every row") && k.apart(c, batch * 2, ev, batch * 2, "an input") &&
         (!od || k.apart(c, batch * 2, od, batch * 2, "an input")) && k.apart(c, batch * 2, bhat, sets * 2 * terms, "an input");
}
// tn_lwe_embed_dev: check_sample_extract's list with the two buffers in each other's place.  Every plan.
static inline bool check_lwe_embed(ApiCheck& k, const void* lwe, const void* a, size_t batch, uint32_t index) {
  const size_t word = (size_t)k.v.elem_bytes;
  return k.plan() && k.lwe_index(index) && k.rows(batch, (size_t)k.v.n + 1, "batch * (n + 1)", "words") && k.work(batch) && k.buffers(a && lwe) &&
         k.apart_bytes(a, batch * 2 * (size_t)k.v.n * word, lwe, batch * ((size_t)k.v.n + 1) * word, "the input");
}
// tn_lwe_modswitch_dev: lwe has batch * (dim + 1) words of the plan's type, exps as many 32-bit words.  Every plan.
static inline bool check_lwe_modswitch(ApiCheck& k, const void* lwe, const void* exps, size_t batch, size_t dim) {
  return k.plan() && k.lwe_dim(dim, "dim") && k.rows(batch, dim + 1, "batch * (dim + 1)", "words") && k.work(batch) && k.buffers(lwe && exps) &&
         k.apart_bytes(exps, batch * (dim + 1) * 4, lwe, batch * (dim + 1) * (size_t)k.v.elem_bytes, "the input");
}
// tn_sample_extract_dev: a has batch * 2 rows, lwe batch * (n + 1) words; index by value, below n.  Every plan.
static inline bool check_sample_extract(ApiCheck& k, const void* a, const void* lwe, size_t batch, uint32_t index) {
  const size_t word = (size_t)k.v.elem_bytes;
  return k.plan() && k.lwe_index(index) && k.rows(batch, (size_t)k.v.n + 1, "batch * (n + 1)", "words") && k.work(batch) && k.buffers(a && lwe) &&
         k.apart_bytes(lwe, batch * ((size_t)k.v.n + 1) * word, a, batch * 2 * (size_t)k.v.n * word, "the input");
}
// tn_lwe_keyswitch_dev: the two dimensions, then what the gadget calls ask with n_in * terms key rows for the row limit, then
// what the kernel's digits and sums hold, then the word counts of lwe and out; ksk has n_in * terms * (n_out + 1) words.  Every plan.
static inline bool check_lwe_keyswitch(ApiCheck& k, const void* lwe, const void* ksk, const void* out, size_t batch, size_t n_in, size_t n_out,
                                       size_t terms, uint32_t base_log, uint32_t flags) {
  const size_t word = (size_t)k.v.elem_bytes;
  return k.plan() && k.lwe_dim(n_in, "n_in") && k.lwe_dim(n_out, "n_out") && k.gadget(n_in, terms, base_log, flags, "n_in * terms", "key rows") &&
         k.lwe_digits(base_log) && k.lwe_sum(n_in, terms) && k.rows(batch, n_in + 1, "batch * (n_in + 1)", "words") &&
         k.rows(batch, n_out + 1, "batch * (n_out + 1)", "words") && k.work(batch) && k.buffers(lwe && ksk && out) &&
         k.apart_bytes(out, batch * (n_out + 1) * word, lwe, batch * (n_in + 1) * word, "an input") &&
         k.apart_bytes(out, batch * (n_out + 1) * word, ksk, n_in * terms * (n_out + 1) * word, "an input");
}
// tn_lwe_ksk_prepared_bytes (host only: no buffer but the answer's) and tn_lwe_ksk_prepare_dev: the plan, the two dimensions,
// terms (1 .. 64, n_in * terms key rows), lwe_sum; then the answer's pointer, or the buffers, kprep's alignment and its byte
// range (lwe_mfma_prepared_bytes) against the plain key's.  Every plan.  No batch: there is always work.
static inline bool check_lwe_ksk_shape(ApiCheck& k, size_t n_in, size_t n_out, size_t terms) {
  return k.plan() && k.lwe_dim(n_in, "n_in") && k.lwe_dim(n_out, "n_out") && k.lwe_key_terms(n_in, terms) && k.lwe_sum(n_in, terms);
}
static inline bool check_lwe_ksk_bytes(ApiCheck& k, size_t n_in, size_t n_out, size_t terms, const size_t* bytes) {
  return check_lwe_ksk_shape(k, n_in, n_out, terms) && k.arguments(bytes != nullptr);
}
static inline bool check_lwe_ksk_prepare(ApiCheck& k, const void* ksk, const void* kprep, size_t n_in, size_t n_out, size_t terms) {
  return check_lwe_ksk_shape(k, n_in, n_out, terms) && k.buffers(ksk && kprep) && k.aligned16(kprep) &&
         k.apart_bytes(kprep, lwe_mfma_prepared_bytes(k.v.q, n_in, n_out, terms), ksk, n_in * terms * (n_out + 1) * (size_t)k.v.elem_bytes, "the input");
}
// tn_lwe_keyswitch_prepared_dev: check_lwe_keyswitch's list with the byte-wide digits behind lwe_digits' place, kprep's
// alignment behind the buffers and kprep's byte range in place of ksk's.  Every plan.
static inline bool check_lwe_keyswitch_prepared(ApiCheck& k, const void* lwe, const void* kprep, const void* out, size_t batch, size_t n_in,
                                                size_t n_out, size_t terms, uint32_t base_log, uint32_t flags) {
  const size_t word = (size_t)k.v.elem_bytes;
  return k.plan() && k.lwe_dim(n_in, "n_in") && k.lwe_dim(n_out, "n_out") && k.gadget(n_in, terms, base_log, flags, "n_in * terms", "key rows") &&
         k.lwe_byte_digits(base_log, flags) && k.lwe_sum(n_in, terms) && k.rows(batch, n_in + 1, "batch * (n_in + 1)", "words") &&
         k.rows(batch, n_out + 1, "batch * (n_out + 1)", "words") && k.work(batch) && k.buffers(lwe && kprep && out) && k.aligned16(kprep) &&
         k.apart_bytes(out, batch * (n_out + 1) * word, lwe, batch * (n_in + 1) * word, "an input") &&
         k.apart_bytes(out, batch * (n_out + 1) * word, kprep, lwe_mfma_prepared_bytes(k.v.q, n_in, n_out, terms), "an input");
}
static inline bool check_pointwise(ApiCheck& k, const void* a, const void* b, const void* c, size_t batch) {      // in place is allowed
  return k.plan() && k.rows_wide(batch) && k.buffers(!batch || (a && b && c));
}
static inline bool check_fill(ApiCheck& k, bool buffers, size_t batch) {                          // tn_fill_lcg_dev, tn_checksum_rows_dev
  return k.arguments(k.v.n && (!batch || buffers)) && k.rows_wide(batch);
}

}  // namespace tn
