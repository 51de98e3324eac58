/*
 * tinyntt.h — C ABI of libtinyntt.so: batched negacyclic polynomial
 * multiplication in Z_q[x]/(x^n+1) on AMD MI355X (gfx950), bit-exact against
 * orhosko/tiny-ntt's golden model.
 *
 * The reference has no FFI layer for this path: its boundary is the Python
 * signature `nwc_poly_mult(a, b, psi_2n) -> c` (new_reference/cg_ntt.py:78),
 * its 8-butterfly twin (new_reference/cg_ntt_8butterfly.py:107), the transforms
 * `cg_ntt` / `cg_intt` (cg_ntt.py:29,68) and the C++ benchmark entry
 * `negacyclic_mul_ntt(a, b, out)` (software_benchmark/benchmark_ntt_60bit.cpp:148,
 * benchmark_ntt.cpp:194).  Each entry point below names the reference interface
 * it replaces.  INTEGRATION.md shows the ctypes stub a maintainer would add.
 *
 * Conventions
 *   - Plain C: opaque plan handle, raw pointers, sizes; no C++/torch types.
 *   - Coefficients: row-major [batch][n], little-endian, uint32_t when q < 2^31,
 *     uint64_t otherwise (tn_plan_elem_bytes tells which).  Natural coefficient
 *     order in and out.  Outputs are canonical residues in [0, q)
 *     (cg_ntt.py:58-59 — Python's % is non-negative).
 *   - Inputs need not be reduced: any word value is taken mod q, as the
 *     reference's `%` does (cg_ntt.py:82-83).
 *   - *_dev entry points take DEVICE pointers (hipMalloc / torch tensors) and a
 *     hipStream_t passed as void* (NULL = the plan's own stream; TN_STREAM_LEGACY =
 *     the device's legacy default stream, hipStreamLegacy); they enqueue and return.  *_host entry points take host pointers, copy in, run, copy
 *     out and synchronise.
 *   - a, b are read-only; c must not alias or overlap a or b (byte ranges are checked: TN_EINVAL).
 *   - Every function returns a tn_status; nothing throws or aborts across the
 *     ABI.  tn_last_error() gives the message for the calling thread.
 *   - A plan's tables are immutable after creation.  *_dev calls on one plan serialise on the stream they are
 *     given and may be issued from several host threads (also on different streams: the fused kernels' row
 *     scheduler hands a counter slot to one launch at a time and falls back to a fixed stride when its ring is
 *     busy).  *_host calls and tn_time_poly_mult_dev use the plan's staging buffers and events and take a
 *     per-plan lock: concurrent callers are served one after the other.  Distinct plans/devices are independent.
 *   - Stream capture: *_dev launches may be captured into a hipGraph (hipStreamBeginCapture on the stream handed in) and
 *     replayed, also beside live launches of the same plan on other streams.  A captured launch never takes a slot of the
 *     row scheduler (it runs the fixed row stride), so no replay can share scheduler state with a live launch.  Plan
 *     creation, the *_host entry points and tn_time_poly_mult_dev synchronise and must not be captured.
 */
#ifndef TINYNTT_H
#define TINYNTT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TN_VERSION 100 /* 0.1.0 */
#define TN_STREAM_LEGACY ((void *)1) /* == hipStreamLegacy: the stream handle-0 callers (e.g. torch's default stream) mean */

typedef enum tn_status {
  TN_OK = 0,
  TN_EBADLEN = 1,   /* n not a supported power of two / wrong length  (ValueError at cg_ntt.py:36-37,:69-70,:79-80) */
  TN_EBADPARAM = 2, /* q even / out of range, psi^n != -1 mod q        (static_asserts at benchmark_ntt_60bit.cpp:58-59) */
  TN_ENODEVICE = 3, /* no usable HIP device: the library never falls back to a CPU path */
  TN_EHIP = 4,      /* a HIP runtime call failed */
  TN_ENOMEM = 5,
  TN_EINVAL = 6,    /* NULL pointer, aliasing, unknown variant */
  TN_EUNSUPPORTED = 7
} tn_status;

/* Kernel schedule selector.  All variants return identical bits. */
typedef enum tn_variant {
  TN_VARIANT_AUTO = 0,  /* fastest available: FUSED when the plan supports it, else CG */
  TN_VARIANT_FUSED = 1, /* register/LDS-tiled merged-twiddle kernel (the throughput path) */
  TN_VARIANT_CG = 2,    /* constant-geometry stage sweep in LDS: the dataflow of cg_ntt.py:49-64 */
  TN_VARIANT_CG8 = 3,   /* same, butterflies issued 8 per lane-step: cg_ntt_8butterfly.py:61-89 */
  TN_VARIANT_CG8_PADDED = 4, /* CG8 with 16 bytes of padding per lane-step in the LDS image; for the rocprof sweep */
  /* the rest of the lane-grouping x LDS-layout sweep (BASELINE config 5): GROUP butterflies per lane-step in {1, 2, 4, 8},
   * layout in {linear, padded, swizzled}; SWIZZLED = XOR-swizzled image, bank-conflict free for every access of the sweep */
  TN_VARIANT_CG_SWIZZLED = 5,
  TN_VARIANT_CG8_SWIZZLED = 6,
  TN_VARIANT_CG2 = 7,
  TN_VARIANT_CG2_PADDED = 8,
  TN_VARIANT_CG2_SWIZZLED = 9,
  TN_VARIANT_CG4 = 10,
  TN_VARIANT_CG4_PADDED = 11,
  TN_VARIANT_CG4_SWIZZLED = 12
} tn_variant;

typedef struct tn_plan tn_plan;

/* Plan flags */
#define TN_PLAN_DEFAULT 0u
#define TN_PLAN_FORCE_CANONICAL 1u /* disable lazy reduction in the FUSED kernel (debug / generic-modulus path) */
/* The caller PROMISES that every input coefficient of tn_poly_mult_* is already in [0, q) — the precondition of the reference's
 * C++ path (mod_add / mod_sub / mod_mul, benchmark_ntt_60bit.cpp:66-77, on make_poly's output :79-87); the Python path reduces
 * with % (cg_ntt.py:82-83) and needs no promise.  The fused product kernel at n = 4096 / 64-bit lanes then skips the input
 * folds (bound schedule started from q, replayed exactly at plan creation); every other kernel ignores the flag.  With the flag
 * set, inputs >= q give undefined results. */
#define TN_PLAN_CANONICAL_INPUTS 2u

/*
 * Create a plan for (n, q, psi) on HIP device `device`.
 * Replaces: module constants N, Q (cg_ntt.py:5-6) + the psi_2n argument of
 * nwc_poly_mult (:78); BENCH_N/BENCH_Q/BENCH_PSI (software_benchmark/CMakeLists.txt:5-7)
 * and the constexpr tables PsiPowers/OmegaPowers/... (benchmark_ntt_60bit.cpp:43-64).
 * Validates n = 2^m (4 <= n <= 8192; fused kernels for 256 <= n <= 8192), q odd prime < 2^62, psi^n == -1 (mod q):
 * the preconditions of the throughput kernels.  Parameters it rejects (TN_EBADPARAM) still have a defined result in the
 * reference: tn_plan_create_general computes it.
 */
tn_status tn_plan_create(tn_plan **out, uint32_t n, uint64_t q, uint64_t psi, int device, uint32_t flags);
/*
 * Plan for the UNTWISTED transforms with an arbitrary omega_n: cg_ntt(a_prime, omega_n, modulus) and
 * cg_intt(A, omega_n, modulus) (cg_ntt.py:29-75) evaluate their butterflies for ANY omega_n — it need not be a primitive
 * n-th root, nor have a square root psi mod q; the inverse uses modinv(omega_n) = omega_n^(q-2) (:72) and n^-1 (:74).
 * Such a plan offers tn_ntt_forward_* / tn_ntt_inverse_* / tn_ntt_forward_trace_host with the constant-geometry variants
 * (plus tn_pointwise_mul_dev, tn_fill_lcg_dev, tn_checksum_rows_dev); everything that needs psi returns TN_EUNSUPPORTED.
 * q: ANY modulus in [2, 2^62), prime or not, odd or even — "modinv" is pow(v, q-2, q) exactly as cg_ntt.py:9-10 computes it.
 */
tn_status tn_plan_create_omega(tn_plan **out, uint32_t n, uint64_t q, uint64_t omega, int device, uint32_t flags);
/*
 * Plan that validates NOTHING beyond the sizes: nwc_poly_mult(a, b, psi_2n) (cg_ntt.py:78-92) never checks psi_2n or the
 * modulus, so it returns a defined list for every psi_2n (roots of unity or not, zero included) and every modulus; this plan
 * computes that list: tables psi^i, omega = psi^2, pow(omega, q-2, q), pow(n, q-2, q), pow(psi, q-2, q)^i built literally,
 * constant-geometry kernels with canonical arithmetic (TN_VARIANT_AUTO = TN_VARIANT_CG; TN_VARIANT_FUSED is unsupported).
 * Offers every entry point except the merged tables of tn_plan_export_table (4, 5).  q in [2, 2^62); 4 <= n <= 8192.
 * The Python mirror falls back to it when tn_plan_create rejects (q, psi).
 */
tn_status tn_plan_create_general(tn_plan **out, uint32_t n, uint64_t q, uint64_t psi, int device, uint32_t flags);
tn_status tn_plan_destroy(tn_plan *plan);

uint32_t tn_plan_n(const tn_plan *plan);
uint64_t tn_plan_q(const tn_plan *plan);
uint64_t tn_plan_psi(const tn_plan *plan);
uint64_t tn_plan_omega(const tn_plan *plan);      /* psi^2: the omega_n that nwc_poly_mult passes to cg_ntt (cg_ntt.py:85) */
uint32_t tn_plan_elem_bytes(const tn_plan *plan); /* 4 or 8 */
int tn_plan_device(const tn_plan *plan);
int tn_plan_has_fused(const tn_plan *plan);       /* 1 if TN_VARIANT_FUSED is available for this (n, q) */
int tn_plan_is_lazy(const tn_plan *plan);         /* 1 if the fused kernel runs with lazy reduction */
int tn_plan_is_general(const tn_plan *plan);      /* 1 for a plan made by tn_plan_create_general */

/*
 * c[r] = a[r] * b[r] in Z_q[x]/(x^n+1) for r < batch.
 * Replaces: nwc_poly_mult(a, b, psi_2n) (cg_ntt.py:78-92), nwc_poly_mult_8butterfly
 * (cg_ntt_8butterfly.py:107-121; use TN_VARIANT_CG8), negacyclic_mul_ntt(a, b, out)
 * (benchmark_ntt_60bit.cpp:148-159).
 */
tn_status tn_poly_mult_dev(tn_plan *plan, const void *a, const void *b, void *c, size_t batch,
                           tn_variant variant, void *stream);
tn_status tn_poly_mult_host(tn_plan *plan, const void *a, const void *b, void *c, size_t batch,
                            tn_variant variant);

/*
 * Product with a PREPARED second operand: b is transformed once (tn_prepare_dev) and multiplied into any number of a's
 * (tn_poly_mult_prepared_dev), which then runs two transforms per row instead of three.  For a fixed b — one key polynomial
 * multiplied into a whole batch, or the same rows of b used by many calls.  Results are bit-identical to tn_poly_mult_dev.
 *
 * tn_prepare_dev: bhat[r] = prepared form of b[r] for r < rows: n words of tn_plan_elem_bytes each, the size of a row.  b may hold
 * any word values (taken mod q).  bhat must not overlap b (TN_EINVAL).
 * tn_poly_mult_prepared_dev: c[r] = a[r] * b[bhat_rows == 1 ? 0 : r] in Z_q[x]/(x^n+1) for r < batch.  bhat_rows must be 1 (one
 * operand shared by every row; the kernel keeps it in registers, so it costs no memory traffic per row) or batch; anything
 * else, and c overlapping a or bhat, is TN_EINVAL.
 *
 * The prepared form is OPAQUE: the negacyclic transform of b as the plan's fused product kernel holds it just before its
 * pointwise step, in that kernel's register order.  A prepared row is valid only for plans with the same (n, q, psi, flags)
 * and for the library build that made it (tn_build_id); do not store it across builds or interpret its words.  It serves the
 * negacyclic product only; there is no cyclic variant.
 * Both calls need a plan with the fused kernels (tn_plan_has_fused; TN_EUNSUPPORTED otherwise: general and omega-only plans,
 * n < 256), enqueue on the stream and return, and may be stream-captured like every *_dev launch.  rows == 0 / batch == 0 succeed
 * and launch nothing.  The reference has no counterpart: nwc_poly_mult transforms both operands on every call (cg_ntt.py:85-86).
 */
tn_status tn_prepare_dev(tn_plan *plan, const void *b, void *bhat, size_t rows, void *stream);
tn_status tn_poly_mult_prepared_dev(tn_plan *plan, const void *a, const void *bhat, size_t bhat_rows, void *c, size_t batch,
                                    void *stream);

/*
 * Dot product against PREPARED operands: c[r] = sum_{j < terms} a[r][j] * b[s][j] in Z_q[x]/(x^n+1), s = (bhat_sets == 1 ? 0 : r),
 * r < batch, with ONE inverse transform per output row: terms + 1 transforms instead of the 2 * terms of `terms` calls of
 * tn_poly_mult_prepared_dev, one result row stored, and no partial product in memory.  For sums of products against fixed
 * operands: the digits of a key switch against its key, a row of a module-lattice matrix against a vector.
 *
 * a is [batch][terms][n] words (the terms of one output row are contiguous; any word values, taken mod q); bhat is
 * [bhat_sets][terms][n], what tn_prepare_dev wrote for bhat_sets * terms rows of b (the prepared form is the same and stays
 * opaque); bhat_sets is 1 (one set of `terms` operands for every output row) or batch; c is [batch][n], canonical residues,
 * bit-identical to adding, mod q, the `terms` results of tn_poly_mult_dev.  terms == 1 is tn_poly_mult_prepared_dev.
 *
 * TN_EUNSUPPORTED: a plan without the fused kernels (as tn_poly_mult_prepared_dev).  TN_EINVAL: a NULL plan or buffer, terms == 0,
 * bhat_sets neither 1 nor batch, batch * terms > 2^31 - 1 (the kernel indexes rows of a with 32 bits), c overlapping a's
 * batch * terms rows or bhat's bhat_sets * terms rows.  batch == 0 succeeds and launches nothing.  Enqueues on the stream and
 * returns; may be stream-captured.  The negacyclic product only: there is no cyclic variant, no *_host form and no tn_multi_* form.
 */
tn_status tn_poly_dot_prepared_dev(tn_plan *plan, const void *a, const void *bhat, size_t bhat_sets, void *c, size_t batch,
                                   size_t terms, void *stream);

/*
 * Operands and results in the TRANSFORM DOMAIN: both operands of a sum of products prepared, the result as coefficients or
 * as a prepared row again, and the way back from a prepared row to coefficients.  For callers whose operands are fixed or
 * reused: c[i] = sum_j A[i][j] * s[j] for a prepared k x l matrix A over a batch of vectors s is one tn_prepare_dev of the
 * batch's l rows per vector and k calls of tn_poly_dot_hat_dev against a shared set (l + k transforms per vector instead of
 * the k (l + 1) of k calls of tn_poly_dot_prepared_dev); results kept prepared can be summed over several launches or fed
 * into the next product and are turned into coefficients once, by tn_unprepare_dev.
 *
 * tn_unprepare_dev: x[r] = the polynomial whose prepared form is xhat[r], r < rows: the inverse of tn_prepare_dev.  Natural
 * order, canonical residues: tn_unprepare_dev(tn_prepare_dev(x)) == x mod q, and tn_prepare_dev(tn_unprepare_dev(xhat)) ==
 * xhat word for word for rows the library wrote.  x must not overlap xhat (TN_EINVAL).
 *
 * tn_poly_dot_hat_dev: out[r] = sum_{j < terms} a[r][j] * b[s][j] in Z_q[x]/(x^n+1), s = (bhat_sets == 1 ? 0 : r), r < batch, with
 * BOTH operands prepared: ahat is [batch][terms][n], bhat is [bhat_sets][terms][n], both as tn_prepare_dev or this function
 * wrote them; bhat_sets is 1 (one set of `terms` rows for every output row) or batch.
 *   out_prepared == 0: out is [batch][n] coefficients, canonical residues; the one inverse transform runs in the same launch.
 *                      Bit-identical to tn_poly_dot_prepared_dev on the un-prepared a, i.e. to adding, mod q, the `terms`
 *                      results of tn_poly_mult_dev.
 *   out_prepared == 1: out is [batch][n] prepared words and no transform runs at all: word for word what tn_prepare_dev
 *                      writes for that coefficient result.
 *
 * The prepared form stays OPAQUE (see tn_prepare_dev), with one property callers may rely on: it is ADDITIVE.  The word-wise
 * sum mod q of two prepared rows of one plan is the prepared row of the sum of the two polynomials, for every plan: the
 * prepared form is a linear image of the polynomial over Z_q (its complete negacyclic transform, or, where the plan's product
 * kernel stops one stage early, its residues modulo the factors y^2 - zeta of x^n + 1), stored as canonical residues.
 * A prepared word the library did not write, in particular one >= q, gives an unspecified result (never an out-of-bounds
 * access: no address depends on data).  Sums must therefore be reduced below q before they are passed back.
 *
 * When to use which (MI355X, profiles/hat_domain_ab.txt; slowest repeat of the new call against the fastest of the old):
 *   - a already prepared (a fixed operand, or a result kept prepared): tn_poly_dot_hat_dev is faster than tn_poly_dot_prepared_dev at
 *     every measured point: x 0.59 - 0.66 of its time at n = 4096 / 60-bit, x 0.62 - 0.80 at n = 1024 / 24-bit (terms 2 - 4,
 *     coefficients out), x 0.42 - 0.71 with out_prepared = 1.
 *   - matrix times vector with the prepare of the vectors counted: faster at k = l = 4 (x 0.74 at n = 4096 / 60-bit, x 0.83 at
 *     n = 1024 / 24-bit) and at k = l = 2, n = 4096 / 60-bit (x 0.92); SLOWER at k = l = 2, n = 1024 / 24-bit (x 1.08: three short
 *     launches against two): there keep calling tn_poly_dot_prepared_dev.
 *   - tn_unprepare_dev costs what tn_ntt_inverse_dev does (x 0.99 / x 0.88); against tn_prepare_dev it is x 1.08 at n = 4096 / 60-bit
 *     (not faster) and x 0.94 at n = 1024 / 24-bit.
 *
 * TN_EUNSUPPORTED: a plan without the fused kernels (as tn_poly_dot_prepared_dev).  TN_EINVAL: a NULL plan or buffer, terms == 0,
 * bhat_sets neither 1 nor batch, batch * terms > 2^31 - 1 (rows are indexed with 32 bits), out_prepared neither 0 nor 1, out
 * overlapping ahat's batch * terms rows or bhat's bhat_sets * terms rows (byte ranges).  batch == 0 / rows == 0 succeed and
 * launch nothing.  Both calls enqueue on the stream and return, and may be stream-captured (a captured launch hands rows out
 * at the fixed stride).  The negacyclic product only: no cyclic variant, no *_host form and no tn_multi_* form.
 */
tn_status tn_unprepare_dev(tn_plan *plan, const void *xhat, void *x, size_t rows, void *stream);
tn_status tn_poly_dot_hat_dev(tn_plan *plan, const void *ahat, const void *bhat, size_t bhat_sets, void *out, size_t batch,
                              size_t terms, int out_prepared, void *stream);

/*
 * GADGET decomposition: the base-2^w digits of every coefficient of a, written out (tn_gadget_decompose_dev) or cut inside the
 * dot-product kernel (tn_poly_gadget_dot_prepared_dev), which is a key switch, a relinearisation or an external product
 * against a prepared key in ONE launch: a is read once per output row and the digits never exist in memory.
 *
 * Definition.  For a word x of a let x^ = x mod q (any word value is accepted), B = 2^w with w = base_log, and
 * u_j = (x^ >> (j w)) & (B - 1) for j < terms.
 *   flags == 0 (unsigned):        d_j = u_j.
 *   TN_GADGET_BALANCED:           carry_0 = 0, t = u_j + carry_j; t >= B/2: d_j = t - B, carry_{j+1} = 1; otherwise d_j = t,
 *                                 carry_{j+1} = 0.  d_j is in [-B/2, B/2); the last carry is dropped.
 * A digit is stored and used as its canonical residue d_j mod q (a negative digit as q + d_j).  Digit polynomial j of row r
 * holds digit j of every coefficient of a[r].  Digits above terms * w bits are not produced: the caller chooses terms.
 *
 * tn_gadget_decompose_dev: digits[r][j] = digit polynomial j of a[r]: a is [batch][n], digits is [batch][terms][n] canonical
 * residues, the layout tn_poly_dot_prepared_dev takes as its a.  An element-wise kernel; works on EVERY plan (general and
 * omega-only plans included).  digits must not overlap a (TN_EINVAL).
 *
 * tn_poly_gadget_dot_prepared_dev: c[r] = sum_{j < terms} digit_j(a[r]) * b[s][j] in Z_q[x]/(x^n+1), s = (bhat_sets == 1 ? 0 : r),
 * r < batch: a is [batch][n], bhat is [bhat_sets][terms][n] as tn_prepare_dev wrote it, bhat_sets is 1 or batch, c is
 * [batch][n] canonical residues, BIT-IDENTICAL to tn_poly_dot_prepared_dev on the output of tn_gadget_decompose_dev.
 * terms == 1 is one digit and the prepared product.
 *
 * When to use which (MI355X, profiles/gadget_dot_ab.txt; slowest repeat of the fused call against the fastest of
 * tn_gadget_decompose_dev followed by tn_poly_dot_prepared_dev on the same buffers, balanced digits, terms 2 - 4):
 *   - a given undecomposed: tn_poly_gadget_dot_prepared_dev is faster at every measured point, x 0.67 - 0.71 of the two launches at
 *     n = 4096 / 60-bit, 65,536 rows (4,795 against 6,998 us at four terms, shared set) and x 0.64 - 0.69 at n = 1024 / 24-bit,
 *     4,096 rows.  No measured point is slower.
 *   - digits that already exist in memory (decomposed once, used by several launches): tn_poly_dot_prepared_dev on them costs the
 *     same as the fused call on a (x 0.97 - 1.00 at n = 4096 / 60-bit, x 1.01 - 1.04 at n = 1024 / 24-bit: there the fused call is
 *     1 - 4 % SLOWER than the dot product alone), so nothing is gained by decomposing again.
 *   - n = 256 was not measured.
 *
 * TN_EINVAL, for both: a NULL plan or buffer, terms == 0, base_log == 0, 2^base_log >= q, (terms - 1) * base_log >= 64 (no
 * shift reaches the word width), a flag bit other than TN_GADGET_BALANCED, batch * terms > 2^31 - 1, an output overlapping an
 * input (byte ranges; c against a's batch rows and bhat's bhat_sets * terms rows); bhat_sets neither 1 nor batch.
 * TN_EUNSUPPORTED: tn_poly_gadget_dot_prepared_dev on a plan without the fused kernels (as tn_poly_dot_prepared_dev).
 * batch == 0 succeeds and launches nothing.  Both enqueue on the stream and return, and may be stream-captured (a captured
 * launch hands rows out at the fixed stride).  The negacyclic product only: no cyclic variant, no *_host form and no
 * tn_multi_* form.  The reference has no counterpart: it has neither a decomposition nor a transform-domain handle.
 */
#define TN_GADGET_BALANCED 1u
tn_status tn_gadget_decompose_dev(tn_plan *plan, const void *a, void *digits, size_t batch, size_t terms, uint32_t base_log,
                                  uint32_t flags, void *stream);
tn_status tn_poly_gadget_dot_prepared_dev(tn_plan *plan, const void *a, const void *bhat, size_t bhat_sets, void *c, size_t batch,
                                          size_t terms, uint32_t base_log, uint32_t flags, void *stream);

/*
 * GADGET product with several output components: both components of a key switch from ONE launch.  A key-switch key is `terms`
 * pairs (b_j, a_j) and the result is (sum_j d_j b_j, sum_j d_j a_j) for the same digits d_j of the same polynomial: a is read,
 * cut into digits and transformed ONCE per term for all components, instead of once per component.
 *
 * tn_poly_gadget_multidot_prepared_dev: c[r][o] = sum_{j < terms} digit_j(a[r]) * b[s][o][j] in Z_q[x]/(x^n+1),
 * s = (bhat_sets == 1 ? 0 : r), r < batch, o < outs.  a is [batch][n], any word values; bhat is [bhat_sets][outs][terms][n] as
 * tn_prepare_dev wrote it for bhat_sets * outs * terms rows (for a shared set, bhat + o * terms * n is a valid shared set of
 * tn_poly_gadget_dot_prepared_dev); c is [batch][outs][n], canonical residues.  Digits, flags and base_log are exactly those of
 * tn_poly_gadget_dot_prepared_dev, and the result is BIT-IDENTICAL to `outs` calls of it, one per component.
 * outs == 1 is that call and runs its kernel; outs == 2 runs a kernel of its own (`terms` forward transforms and two inverses
 * per output row instead of 2 * terms and two).  outs > 2 is NOT SUPPORTED: TN_EUNSUPPORTED.
 *
 * When to use which (MI355X, profiles/gadget_pair_ab.txt; slowest repeat of the one launch against the fastest repeat of two
 * tn_poly_gadget_dot_prepared_dev launches on the same buffers, balanced digits, terms 2 - 4):
 *   - both components wanted: one tn_poly_gadget_multidot_prepared_dev launch is faster at every measured point, x 0.70 - 0.76 of
 *     the two launches at n = 4096 / 60-bit, 65,536 rows and x 0.74 - 0.79 at n = 1024 / 24-bit, 4,096 rows, shared set or a set
 *     per row.  No measured point is slower.  The gain grows with terms.
 *   - one component wanted: outs = 1 is tn_poly_gadget_dot_prepared_dev, at its cost.
 *   - n = 256, n = 8192 and the canonical policy were not measured.
 *
 * TN_EINVAL: everything tn_poly_gadget_dot_prepared_dev refuses, in its order, with the row limit on batch * outs * terms
 * (<= 2^31 - 1) and the overlap check on c's batch * outs rows against a's batch rows and bhat's bhat_sets * outs * terms rows
 * (byte ranges); outs == 0.  TN_EUNSUPPORTED: a plan without the fused kernels; outs > 2 (looked at after the plan, before
 * terms, flags and base_log).  batch == 0 succeeds and launches nothing.  The call enqueues on the stream and returns, and may
 * be stream-captured (a captured launch hands rows out at the fixed stride).  No cyclic variant, no *_host form and no
 * tn_multi_* form.
 */
tn_status tn_poly_gadget_multidot_prepared_dev(tn_plan *plan, const void *a, const void *bhat, size_t bhat_sets, void *c, size_t batch,
                                               size_t outs, size_t terms, uint32_t base_log, uint32_t flags, void *stream);

/*
 * EXTERNAL PRODUCT RGSW x RLWE: both output components from the digits of ALL input polynomials of a ciphertext in ONE launch,
 * the inner loop of a CMux, a blind rotation (FHEW, TFHE, LMKCDEY) and a GSW-style multiplication.  The two calls above cut the
 * digits of one polynomial per output row; this one cuts the digits of every component of (a_0, ..., a_{ins-1}) and multiplies
 * all ins * terms digit rows into every output component.
 *
 * tn_poly_external_product_prepared_dev: c[r][o] = sum_{i < ins} sum_{j < terms} digit_j(a[r][i]) * b[s][o][i][j] in
 * Z_q[x]/(x^n+1), s = (bhat_sets == 1 ? 0 : r), r < batch, o < outs.  a is [batch][ins][n], any word values, taken mod q; bhat
 * is [bhat_sets][outs][ins][terms][n] as tn_prepare_dev wrote it for that many rows of b; c is [batch][outs][n], canonical
 * residues.  With this layout bhat + o * ins * terms * n of a shared set is a valid shared set of tn_poly_dot_prepared_dev with
 * ins * terms terms, and for ins == 1 the layout is exactly tn_poly_gadget_multidot_prepared_dev's.  Digits, flags and base_log
 * are those of tn_poly_gadget_dot_prepared_dev; balanced carries start at 0 for every input polynomial and never run from one
 * polynomial into the next.
 * The result is BIT-IDENTICAL, component by component, to tn_poly_dot_prepared_dev with ins * terms terms on the digits that
 * tn_gadget_decompose_dev writes for a viewed as batch * ins rows ([batch * ins][terms][n] = [batch][ins * terms][n]) and
 * component o's [sets][ins * terms][n] slice of bhat.
 *   ins == 1             is tn_poly_gadget_multidot_prepared_dev and runs its kernels.
 *   ins >= 2, outs == 2  runs a kernel of its own: ins * terms forward transforms and two inverses per output row, nothing but a
 *                        read and c written; ins is a run-time count (ins = 3, a rank-2 module, works like ins = 2).
 *   ins >= 2, outs == 1  is NOT SUPPORTED (TN_EUNSUPPORTED): tn_gadget_decompose_dev on the batch * ins rows followed by
 *                        tn_poly_dot_prepared_dev with ins * terms terms serves it.
 *
 * When to use which (MI355X, profiles/extprod_ab.txt; ins = outs = 2, balanced digits, terms 2 - 4, 9 interleaved repeats; the
 * slowest repeat of the one launch against the fastest repeat of the faster of two routes on the same buffers: route A, one
 * tn_poly_gadget_multidot_prepared_dev launch per input polynomial and a modular addition of the two results; route B,
 * tn_gadget_decompose_dev and one tn_poly_dot_prepared_dev launch per component):
 *   - ins >= 2, both components wanted: the one launch is faster at every measured point by disjoint ranges, x 0.55 - 0.61 of the
 *     faster route at n = 4096 / 60-bit, 65,536 rows (6,916 us against route B's 12,164 us at two terms, shared key; the key per
 *     row at four terms was measured at 32,768 rows) and x 0.59 - 0.60 at n = 1024 / 24-bit, 4,096 rows.  Route B is the faster
 *     route at two and three terms, route A at four terms of n = 4096.  No measured point is slower or within the spread.
 *   - route A's two launches WITHOUT their addition still cost more: the one launch is x 0.83 - 0.90 of them at n = 4096 and
 *     x 0.77 - 0.86 at n = 1024; the addition in torch costs about as much again as the launches at two terms.
 *   - one input polynomial: ins = 1 is tn_poly_gadget_multidot_prepared_dev, at its cost.
 *   - n = 256, n = 8192, the canonical policy and ins = 3 were not measured.
 *
 * Status, in this order: TN_EINVAL for a NULL plan; TN_EUNSUPPORTED for a plan without the fused kernels; TN_EINVAL for
 * ins == 0; TN_EINVAL for outs == 0 and TN_EUNSUPPORTED for outs > 2; TN_EUNSUPPORTED for ins >= 2 with outs == 1; TN_EINVAL
 * for everything the gadget calls refuse (terms == 0, a flag bit other than TN_GADGET_BALANCED, base_log == 0 or
 * 2^base_log >= q, (terms - 1) * base_log >= 64, batch * outs * ins * terms > 2^31 - 1); batch == 0 succeeds and launches
 * nothing; TN_EINVAL for a NULL buffer, for bhat_sets neither 1 nor batch, and for c's batch * outs rows overlapping a's
 * batch * ins rows or bhat's bhat_sets * outs * ins * terms rows (byte ranges).  The call enqueues on the stream and returns,
 * and may be stream-captured (a captured launch hands rows out at the fixed stride).  No cyclic variant, no *_host form and
 * no tn_multi_* form.
 */
tn_status tn_poly_external_product_prepared_dev(tn_plan *plan, const void *a, const void *bhat, size_t bhat_sets, void *c,
                                                size_t batch, size_t ins, size_t outs, size_t terms, uint32_t base_log,
                                                uint32_t flags, void *stream);

/*
 * CMUX ROTATION STEP: one step of a blind rotation (FHEW, TFHE, LMKCDEY) on an accumulator ciphertext acc = (acc_0, acc_1),
 *     acc  <-  acc + RGSW(s_i) [x] ((X^e - 1) * acc),        e = the step's LWE coefficient, another one for every ciphertext,
 * as the explicit pieces (tn_monomial_mul_dev, then tn_poly_external_product_prepared_dev, then an addition) or from ONE launch
 * (tn_poly_cmux_rotate_prepared_dev): the rotation is an address offset and a sign on the load the kernel performs anyway, and
 * the unrotated words that "- acc" needs are the ones the addition at the store needs.  No transform is added: 2 * terms + 2
 * per row, as in the external product.
 *
 * Definition.  exps is a DEVICE array of batch 32-bit words; any value is taken mod 2n: e = exps[r] & (2n - 1).  For a row x
 * (any word values, taken mod q) and t < n let s = (t - e) mod 2n; then
 *     rot_e(x)[t] = x[s] mod q                      if s < n,
 *                 = (q - x[s - n] mod q) mod q      otherwise      (a zero stays 0, never q).
 * rot_e(x) is X^e * x in Z_q[x]/(x^n + 1); rot_0 is canonicalisation, rot_n is negation.
 *
 * tn_monomial_mul_dev: a and out are [batch][group][n]; exponent exps[r] applies to all `group` rows of item r (group = 2 for
 * an RLWE ciphertext).  flags == 0: out = rot_e(a), that is X^e * a.  TN_MONOMIAL_MINUS_ONE: out = (rot_e(a) - a) mod q, that is
 * (X^e - 1) * a.  Outputs are canonical residues.  An element-wise kernel on EVERY plan (general and omega-only plans
 * included): it needs only n and q.  Stores are unit-stride, loads are unit-stride apart from the one wrap.  The index is
 * masked to the row: NO CONTENT OF exps CAN CAUSE AN OUT-OF-BOUNDS ACCESS (the same holds for the fused call).
 *
 * exps is read by the kernel, not by the host: a CAPTURED launch sees the exponents that are in the buffer at REPLAY time.  A
 * blind rotation replays one graph with new exponents written into the same buffer.
 *
 * tn_poly_cmux_rotate_prepared_dev:
 *     c[r][o] = ( a[r][o] mod q + sum_{i < comps} sum_{j < terms} digit_j( ((X^{e_r} - 1) * a[r][i]) ) * b[s][o][i][j] ) mod q,
 * o < comps, s = (bhat_sets == 1 ? 0 : r), r < batch.  a and c are [batch][comps][n]; bhat is [bhat_sets][comps][comps][terms][n],
 * exactly the layout of tn_poly_external_product_prepared_dev with ins = outs = comps; exps as above.  Digits, base_log and
 * flags (TN_GADGET_BALANCED) are the gadget calls'; carries start at 0 for every input polynomial.  comps must be 2 (the
 * kernel has two output components).
 * The result is BIT-IDENTICAL to the explicit route on the same buffers: tn_monomial_mul_dev(group = 2, TN_MONOMIAL_MINUS_ONE),
 * tn_poly_external_product_prepared_dev(ins = 2, outs = 2) on its output, then word-wise (a mod q + .) mod q.
 * c must not overlap a or bhat (byte ranges): the call does not run in place.  A blind rotation alternates two accumulator
 * buffers, acc -> acc' -> acc.
 *
 * When to use which (MI355X, profiles/cmux_ab.txt, tools/gpu_cmux.py; balanced digits, terms 2 - 4, random exponents, shared key
 * and key per row, 9 interleaved repeats; a point counts as faster only where the one launch's slowest repeat is below the
 * other's fastest; all outputs compared in full first):
 *   - a step of a blind rotation: tn_poly_cmux_rotate_prepared_dev is faster than the explicit route (tn_monomial_mul_dev,
 *     tn_poly_external_product_prepared_dev, the addition in torch) at all twelve measured points by disjoint ranges:
 *     x 0.48 - 0.62 at n = 4096 / 60-bit, 65,536 rows (7,642 against 15,969 us at two terms, shared key; the key per row at four
 *     terms ran on 32,768 rows) and x 0.54 - 0.66 at n = 1024 / 24-bit, 4,096 rows (72.1 against 134.1 us).  The gain shrinks
 *     with terms: the saving is a fixed amount per row.
 *   - against the route's two library launches WITHOUT the addition it is still faster at all twelve points by disjoint ranges,
 *     x 0.87 - 0.91 at n = 4096 and x 0.93 - 0.97 at n = 1024: a caller with a fused addition of their own gains that much.
 *   - against a plain tn_poly_external_product_prepared_dev launch on the same rows it is SLOWER at all twelve points, x 1.05 -
 *     1.14 at n = 4096 (700 - 1,000 us more for 65,536 rows, about the same at every term count) and x 1.08 - 1.14 at n = 1024: that is
 *     the price of the rotation and the add-in, two more reads of a by count.  How many of them hit in L2 was not isolated.
 *   - the rotation alone (an automorphism-like gather): tn_monomial_mul_dev; its time is inside the route's figures and was not
 *     measured by itself.
 *   - not measured: n = 256, n = 8192, the canonical policy, unsigned digits, a graph of many steps.
 *
 * Status of tn_monomial_mul_dev, in this order: TN_EINVAL for a NULL plan; for group == 0; for a flag bit other than
 * TN_MONOMIAL_MINUS_ONE; for batch * group > 2^31 - 1; batch == 0 succeeds and launches nothing; TN_EINVAL for a NULL buffer
 * (exps included) and for out's rows overlapping a's (byte ranges): the kernel gathers, nothing runs in place.
 * Status of tn_poly_cmux_rotate_prepared_dev, in this order: TN_EINVAL for a NULL plan; TN_EUNSUPPORTED for a plan without the
 * fused kernels; TN_EINVAL for comps == 0 and TN_EUNSUPPORTED for comps other than 2 (the text names the explicit route);
 * TN_EINVAL for everything the gadget calls refuse (terms == 0, a flag bit other than TN_GADGET_BALANCED, base_log == 0 or
 * 2^base_log >= q, (terms - 1) * base_log >= 64, batch * comps * comps * terms > 2^31 - 1); batch == 0 succeeds and launches
 * nothing; TN_EINVAL for a NULL buffer (exps included), for bhat_sets neither 1 nor batch, and for c's batch * comps rows
 * overlapping a's batch * comps rows or bhat's bhat_sets * comps * comps * terms rows.
 * Both calls enqueue on the stream and return, and may be stream-captured (a captured launch of the fused call hands rows out
 * at the fixed stride).  No cyclic variant, no *_host form and no tn_multi_* form.  The reference has no counterpart.
 */
#define TN_MONOMIAL_MINUS_ONE 1u
tn_status tn_monomial_mul_dev(tn_plan *plan, const void *a, const uint32_t *exps, void *out, size_t batch, size_t group,
                              uint32_t flags, void *stream);
tn_status tn_poly_cmux_rotate_prepared_dev(tn_plan *plan, const void *a, const uint32_t *exps, const void *bhat, size_t bhat_sets,
                                           void *c, size_t batch, size_t comps, size_t terms, uint32_t base_log, uint32_t flags,
                                           void *stream);

/*
 * BLIND ROTATION FROM ONE LAUNCH: `steps` CMux rotation steps per ciphertext with the accumulator kept in LDS across them
 * (tn_poly_blind_rotate_prepared_dev).  A row's blind rotation depends on no other row, so the workgroup that takes a row keeps
 * it for all steps: a is read once, c is written once, the rotated words and the add-in words of every step come from LDS, and
 * the only global traffic of a step is its key (shared by every row: L2) and one scalar load of the exponent.  One launch
 * instead of `steps`, no launch boundary between steps.
 *
 * a and c are [batch][2][n].  exps is a DEVICE array [steps][batch] (the layout of Plan.blind_rotate); any word is taken mod 2n
 * and the index is masked to the row, as above: no content of exps can cause an out-of-bounds access, and a captured launch sees
 * the exponents that are in the buffer at replay time.  bhat is [steps][2][2][terms][n] prepared rows: ONE KEY PER STEP, shared by
 * every row (a key per row and step is out of scope).  comps must be 2.  Digits, base_log and flags are the gadget calls'.
 * The result is BIT-IDENTICAL to `steps` calls of tn_poly_cmux_rotate_prepared_dev with bhat_sets = 1, step k on key k
 * (bhat + k * 4 * terms rows) and exps + k * batch.
 * c == a, the same pointer, is allowed (in place): a workgroup reads its row before it writes it and no other workgroup touches
 * that row.  Any other overlap of c with a, and any overlap of c with bhat, is refused.
 *
 * Shapes.  A fused plan is supported when the kernel's LDS request (the CMux step's layout plus two rows of n words) fits the
 * 160 KiB of one workgroup (csrc/launch_plan.h: blindrot_supported; tests/test_blindrot_emu.py walks every shape).  Supported:
 * n = 256 .. 4096 with 32-bit and with 64-bit words, n = 8192 with 32-bit words.  Over the limit: n = 8192 with 64-bit words
 * alone (two rows are 128 KiB beside a transpose image of 64 KiB and more): TN_EUNSUPPORTED, and the text names the loop over
 * tn_poly_cmux_rotate_prepared_dev.
 *
 * When to use which (MI355X, profiles/blindrot_ab.txt, tools/gpu_blindrot.py; balanced digits, random exponents, terms 2 and 3,
 * 9 interleaved repeats, the output compared in full with the loop's first; a point counts as faster only where the one launch's
 * slowest repeat is below the other's fastest):
 *   - a few hundred ciphertexts (batch 256: fewer rows than workgroups can be resident): the one launch is FASTER than the loop
 *     of tn_poly_cmux_rotate_prepared_dev launches at all six points by disjoint ranges, x 0.77 - 0.86 (n = 4096 / 60-bit, 16
 *     steps, two terms: 577 against 746 us; n = 1024 / 24-bit, 64 steps: 840 against 1,051 us), and as much faster than the same
 *     launches replayed from one captured graph (x 0.77 - 0.85): the graph does not remove the per-launch cost, the one launch does.
 *   - thousands of ciphertexts (batch 4,096): the one launch is SLOWER than the loop at all six points by disjoint ranges,
 *     x 1.04 - 1.08 at n = 1024 / 24-bit, x 1.06 - 1.10 at n = 2048 / 60-bit, x 1.13 - 1.16 at n = 4096 / 60-bit (9,073 against
 *     8,046 us at two terms), and slower than the graph (x 1.03 - 1.11).  The launch cost is small beside a step there, and the
 *     accumulator's LDS leaves fewer resident workgroups per CU than the step kernel has.  Use the loop (Plan.blind_rotate), or
 *     split the batch.
 *   - where the crossover lies between 256 and 4,096 rows was not measured; nor were n = 256, 512, 8192, the canonical policy,
 *     unsigned digits, step counts other than 64 (n = 1024) and 16, and in-place launches.
 *
 * Status, in this order: TN_EINVAL for a NULL plan; TN_EUNSUPPORTED for a plan without the fused kernels and for a shape over
 * the LDS limit; TN_EINVAL for comps == 0 and TN_EUNSUPPORTED for comps other than 2; TN_EINVAL for steps == 0; for everything
 * the gadget calls refuse (terms == 0, a flag bit other than TN_GADGET_BALANCED, base_log == 0 or 2^base_log >= q,
 * (terms - 1) * base_log >= 64); for steps * 4 * terms, batch * 2 or steps * batch above 2^31 - 1 (a text each); batch == 0
 * succeeds and launches nothing; TN_EINVAL for a NULL buffer (exps included), for c overlapping a without being a, and for c
 * overlapping bhat's steps * 4 * terms rows (byte ranges).
 * The call enqueues on the stream and returns, and may be stream-captured (a captured launch hands rows out at the fixed
 * stride).  No cyclic variant, no *_host form and no tn_multi_* form.  The reference has no counterpart.
 */
tn_status tn_poly_blind_rotate_prepared_dev(tn_plan *plan, const void *a, const uint32_t *exps, const void *bhat, void *c,
                                            size_t batch, size_t comps, size_t steps, size_t terms, uint32_t base_log,
                                            uint32_t flags, void *stream);

/*
 * GALOIS AUTOMORPHISMS: sigma_g : a(x) -> a(x^g) mod (x^n + 1) for odd g, on coefficient rows (tn_automorphism_dev) and on
 * prepared rows (tn_automorphism_prepared_dev).  Every rotation and conjugation of an RLWE scheme applies one before its key
 * switch (tn_poly_gadget_multidot_prepared_dev); traces, ring packing and hoisted rotations apply them to prepared rows.
 *
 * Definition.  A Galois element is an odd g with 1 <= g < 2n.  For a row a (any word values, taken mod q) sigma_g(a) is the
 * row out with, for every i < n and t = i g mod 2n:
 *     out[t]     = a[i] mod q             if t < n,
 *     out[t - n] = (q - a[i] mod q) mod q otherwise.
 * Outputs are canonical residues in [0, q); a zero coefficient stays 0 under the negation and never becomes q.  sigma_g is a
 * ring homomorphism, sigma_g(sigma_h(a)) = sigma_{g h mod 2n}(a), and sigma_1 is canonicalisation.
 *
 * tn_automorphism_dev: out[r][m] = sigma_{galois[m]}(a[r]), r < batch, m < count.  a is [batch][n]; out is [batch][count][n];
 * galois is a HOST array of count elements, read before the call returns.  Works on EVERY plan (general and omega-only plans
 * included): it needs only n and q.
 *
 * tn_automorphism_prepared_dev: the same on PREPARED rows: out[r][m] is the prepared form of sigma_{galois[m]}(the polynomial
 * whose prepared form is xhat[r]), word for word what tn_prepare_dev writes for sigma_g(tn_unprepare_dev(xhat[r])), for rows
 * the library wrote.  xhat is [rows][n], out is [rows][count][n].  In the transform domain the automorphism is a permutation of
 * words (and, where the plan's product runs the base case, one twiddle product on every second word): no transform runs.
 *
 * The elements travel by value in the kernel arguments, hence TN_GALOIS_MAX: no device table, no per-plan cache, no copy and no
 * synchronisation; nothing is set up per g.  count > 1 reads every input row once and writes count images of it (a hoisted
 * set of rotations, a trace step).  Both calls enqueue on the stream and return, and may be stream-captured.
 *
 * Status, in the order checked: TN_EINVAL a NULL plan; TN_EUNSUPPORTED tn_automorphism_prepared_dev on a plan without the
 * fused kernels (tn_plan_has_fused); TN_EINVAL count outside [1, TN_GALOIS_MAX]; TN_EINVAL an element that is even or >= 2n
 * (the text names its position); TN_EINVAL batch * count > 2^31 - 1; batch == 0 / rows == 0 succeed and launch nothing;
 * TN_EINVAL a NULL buffer or a NULL galois; TN_EINVAL out's batch * count rows overlapping the input's batch rows (byte
 * ranges): the kernels gather, so nothing runs in place.
 *
 * When to use which (MI355X, profiles/galois_ab.txt, tools/gpu_galois.py; 9 interleaved repeats, slowest repeat of the new call
 * against the fastest of the route it replaces; g in {3, 5, 2n - 1, one seeded}):
 *   - coefficients: tn_automorphism_dev is faster than the torch route (index_select, q - x, where) at every measured point:
 *     834 - 837 against 4,460 - 6,130 us at n = 4096 / 60-bit, 65,536 rows (x 0.14 - 0.19) and 7.3 - 7.9 against 39.6 - 40.4 us
 *     at n = 1024 / 24-bit, 4,096 rows (x 0.18 - 0.20).  At n = 4096 it runs at the rate of a device-to-device copy of the same
 *     rows (5.13 TB/s, x 0.98 of the copy's time); at n = 1024 / 4,096 rows, a launch of 8 us, it takes x 1.9 of the copy's 4.2 us.
 *   - prepared rows: tn_automorphism_prepared_dev is faster than tn_unprepare_dev + the torch route + tn_prepare_dev at every
 *     measured point: 729 - 734 against 6,100 - 7,710 us at n = 4096 / 60-bit (x 0.10 - 0.12; base-case format, x 0.86 of the
 *     copy's time) and 8.6 - 9.0 against 62.5 - 64.9 us at n = 1024 / 24-bit (x 0.13 - 0.14; x 2.1 of the copy's time).  A
 *     prepared row never needs to leave the transform domain to be rotated.
 *   - several elements of the same rows: one call with count = 4 against four calls with count = 1 is x 0.65 (coefficients) and
 *     x 0.79 (prepared) at n = 4096 / 60-bit, x 0.62 and x 0.57 at n = 1024 / 24-bit.  No measured point is slower.
 *   - beside a key switch: the coefficient automorphism takes x 0.21 (n = 4096 / 60-bit) and x 0.19 (n = 1024 / 24-bit) of one
 *     tn_poly_gadget_multidot_prepared_dev launch (outs 2, terms 2, shared key) on the same rows.
 *   - not measured: n = 256, n = 8192, the canonical policy, count above 4.  Not tested: a launch under stream capture; at
 *     n = 8192 with 64-bit words (an image above 48 KiB) the launcher sets the kernel's dynamic-LDS limit before every launch,
 *     as the launchers of the fused families do, and that path has never run inside a capture.
 *
 * No *_host form, no tn_multi_* form and no cyclic variant (the prepared form serves the negacyclic ring only).  The
 * reference has no counterpart.
 */
#define TN_GALOIS_MAX 16
tn_status tn_automorphism_dev(tn_plan *plan, const void *a, void *out, size_t batch, const uint32_t *galois, size_t count, void *stream);
tn_status tn_automorphism_prepared_dev(tn_plan *plan, const void *xhat, void *out, size_t rows, const uint32_t *galois, size_t count,
                                       void *stream);

/*
 * AUTOMORPHISM KEY SWITCH: the homomorphic automorphism of an RLWE ciphertext (c0, c1) under a key from sigma_g(s) to s,
 *     out0 = sigma_g(c0) + sum_j digit_j(sigma_g(c1)) * K[0][j]
 *     out1 =               sum_j digit_j(sigma_g(c1)) * K[1][j],
 * from ONE launch (tn_poly_galois_keyswitch_prepared_dev): the rotation of BFV / CKKS-style schemes, one step of a trace or of
 * LWE -> RLWE packing, the step between external products of an automorphism-based blind rotation (LMKCDEY).  sigma_g is a
 * signed index map on the load the gadget kernel performs anyway and sigma_g(c0) an add-in at its store; no transform is added:
 * terms + 2 per row, as in tn_poly_gadget_multidot_prepared_dev with outs = 2.
 *
 * tn_poly_galois_keyswitch_prepared_dev:
 *     c[r][o] = ( [o == 0] sigma_g(a[r][0]) + sum_{j < terms} digit_j( sigma_g(a[r][1]) ) * b[s][o][j] ) mod q,
 * o < 2, s = (bhat_sets == 1 ? 0 : r), r < batch.  a is [batch][2][n], any word values, taken mod q: a[r][0] is only rotated,
 * a[r][1] is rotated and switched.  bhat is [bhat_sets][2][terms][n] prepared rows, exactly the layout of
 * tn_poly_gadget_multidot_prepared_dev with outs = 2; bhat_sets is 1 (one key for every row) or batch.  c is [batch][2][n],
 * canonical residues.  sigma_g is the map defined above (GALOIS AUTOMORPHISMS); galois is ONE odd element below 2n, passed by
 * value: no table, nothing is set up per g, and a captured launch replays the g it was captured with.  Digits, base_log and
 * flags (TN_GADGET_BALANCED) are the gadget calls'.
 * The result is BIT-IDENTICAL to the explicit route on the same buffers: tn_automorphism_dev on a viewed as batch * 2 rows with
 * count = 1; tn_poly_gadget_multidot_prepared_dev with outs = 2 on the rotated a[r][1] rows; component 0 plus the rotated
 * a[r][0], word-wise mod q.  sigma_g is applied BEFORE the digits are cut, and that order is part of the contract: a balanced
 * digit of q - x is not minus the digit of x, so rotating the digits of a[r][1] instead is a different function of the inputs.
 * g = 1 is a plain key switch with its body added in, c = (a0 + <digits(a1), K[0]>, <digits(a1), K[1]>), useful by itself.
 * c must not overlap a or bhat (byte ranges): the kernel permutes within a row and prefetches the next one, so the call does
 * not run in place.  The index into the row is masked: no value of galois could cause an out-of-bounds access.
 *
 * When to use which (MI355X, profiles/galoisks_ab.txt, tools/gpu_galoisks.py; balanced digits, terms 2 - 4, g in {3, 5, 2n - 1,
 * one seeded} reported as a range, shared key and key per row, 9 interleaved repeats; a point counts as faster only where the
 * one launch's slowest repeat is below the other's fastest; all outputs compared in full first):
 *   - the homomorphic automorphism of a batch of ciphertexts: tn_poly_galois_keyswitch_prepared_dev is faster than the explicit
 *     route (tn_automorphism_dev, tn_poly_gadget_multidot_prepared_dev, the addition in torch) at all twelve measured points, for
 *     every g, by disjoint ranges: x 0.50 - 0.63 at n = 4096 / 60-bit, 65,536 rows (4,608 - 4,729 against 9,309 - 9,321 us at two
 *     terms, shared key) and x 0.51 - 0.63 at n = 1024 / 24-bit, 4,096 rows (44.5 - 44.6 against 87.9 - 88.0 us).  The gain shrinks
 *     with terms: the saving is a fixed amount per row.  The route was timed on the layout that suits it, [2][batch][n], where
 *     the rotated second components are contiguous rows; a caller who holds [batch][2][n] pays a copy on top of it.
 *   - against the route's two library launches WITHOUT the addition it is still faster at all twelve points by disjoint ranges,
 *     x 0.77 - 0.88 at n = 4096 and x 0.82 - 0.90 at n = 1024: a caller with a fused addition of their own gains that much.
 *   - against a plain tn_poly_gadget_multidot_prepared_dev launch (outs = 2) on the unrotated second components it is SLOWER at
 *     all twelve points, for every g, by disjoint ranges: x 1.06 - 1.14 at n = 4096 (390 - 810 us more for 65,536 rows) and
 *     x 1.06 - 1.11 at n = 1024 (3 - 6 us more for 4,096 rows): the price of the two permutations, their barriers and the second
 *     input row.  g = 3 is the slowest element at n = 4096 with a shared key (4,729 against 4,608 - 4,619 us at two terms, 7,295
 *     against 6,976 - 6,997 us at four) and at n = 1024 with a key per row (71.6 against 70.0 us at four terms); elsewhere the
 *     elements are within 1.3 % of one another.  Why was not isolated.
 *   - g = 1, a key switch with its body added in: not timed by itself; it runs the same code as every other g.
 *   - not measured: n = 256, n = 8192, the canonical policy, unsigned digits.
 *
 * Out of scope: a c = a + ... flag for trace steps; several g per call with one key each; a Galois element per row; rank above
 * 1; and the hoisted form (decompose once, rotate the transformed digits with tn_automorphism_prepared_dev), which is a
 * different function of its inputs and not bit-identical to this one.
 *
 * Status, in this order: TN_EINVAL for a NULL plan; TN_EUNSUPPORTED for a plan without the fused kernels; TN_EINVAL for a galois
 * that is even or >= 2n (the text names it); for everything the gadget calls refuse (terms == 0, a flag bit other than
 * TN_GADGET_BALANCED, base_log == 0 or 2^base_log >= q, (terms - 1) * base_log >= 64, batch * 2 * terms > 2^31 - 1); batch == 0
 * succeeds and launches nothing; TN_EINVAL for a NULL buffer, for bhat_sets neither 1 nor batch, and for c's batch * 2 rows
 * overlapping a's batch * 2 rows or bhat's bhat_sets * 2 * terms rows.
 * The call enqueues on the stream and returns, and may be stream-captured (a captured launch hands rows out at the fixed
 * stride).  Fused plans only; no cyclic variant, no *_host form and no tn_multi_* form.  The reference has no counterpart.
 */
tn_status tn_poly_galois_keyswitch_prepared_dev(tn_plan *plan, const void *a, uint32_t galois, const void *bhat, size_t bhat_sets,
                                                void *c, size_t batch, size_t terms, uint32_t base_log, uint32_t flags, void *stream);

/*
 * PACK STEP AND TRACE STEP: one level of LWE -> RLWE ring packing (PackLWEs and the field trace of Chen, Dai, Kim, Song,
 * "Efficient Homomorphic Conversion Between (Ring) LWE Ciphertexts"), from ONE launch:
 *     ct = (ev + X^rot od) + EvalAuto(ev - X^rot od, g),
 * EvalAuto the homomorphic automorphism above.  With t = X^rot * od on both components, s = ev + t and d = ev - t (every input
 * word taken mod q):
 *     c[r][0] = ( s0 + sigma_g(d0) + sum_{j < terms} digit_j( sigma_g(d1) ) * b[k][0][j] ) mod q
 *     c[r][1] = ( s1 +               sum_{j < terms} digit_j( sigma_g(d1) ) * b[k][1][j] ) mod q,
 * k = (bhat_sets == 1 ? 0 : r), r < batch.  ev, od and c are [batch][2][n]; bhat is [bhat_sets][2][terms][n] prepared rows, the
 * key from sigma_g(s) to s in the layout of tn_poly_galois_keyswitch_prepared_dev; rot (below 2n) and galois (odd, below 2n) are
 * passed by value: no table, and a captured launch replays the values it was captured with.  od == NULL is the TRACE STEP,
 * ct = ev + EvalAuto(ev, g) (s = d = ev); rot must then be 0.
 * The result is BIT-IDENTICAL to the explicit route: tn_monomial_mul_dev on od with the exponent rot; s and d by addition and
 * subtraction mod q of canonical words; tn_poly_galois_keyswitch_prepared_dev on d; the addition of s mod q.  The subtraction
 * comes before sigma_g and sigma_g before the digits are cut.  terms + 2 transforms per row, as in the automorphism key switch.
 * c must not overlap ev, od or bhat (byte ranges): the kernel reads a row's inputs again after its first component is stored.
 * Both indices into a row are masked: no value of rot or galois could cause an out-of-bounds access.
 *
 * The packing tree (Plan.pack_lwes in the Python package has it whole): embed ell = 2^m LWE ciphertexts with tn_lwe_embed_dev
 * at index 0, slot-major; at level t = 1 .. m pair the first half of the list with the second in one launch with
 * rot = n / 2^t, g = 2^t + 1; then trace steps for t = m + 1 .. log2 n with g = 2^t + 1.  The phase of the result is
 * n * sum_j mu_j X^(j n / ell) plus noise: THE FACTOR n IS NOT REMOVED.  The caller scales by n^-1 mod q beforehand, as the paper does.
 *
 * Status, in this order: TN_EINVAL for a NULL plan; TN_EUNSUPPORTED for a plan without the fused kernels; TN_EINVAL for a galois
 * that is even or >= 2n; for rot >= 2n, or rot != 0 with od == NULL; for everything the gadget calls refuse (as
 * tn_poly_galois_keyswitch_prepared_dev); batch == 0 succeeds and launches nothing; TN_EINVAL for a NULL ev, bhat or c, for
 * bhat_sets neither 1 nor batch, and for c's batch * 2 rows overlapping ev's or od's batch * 2 rows or bhat's bhat_sets * 2 * terms rows.
 * The call enqueues on the stream and returns, and may be stream-captured.  Fused plans only.  The reference has no counterpart.
 *
 * When to use which (MI355X, profiles/pack_ab.txt, tools/gpu_pack.py; one process per point, 9 interleaved repeats, one shared key,
 * balanced digits, terms 2 - 4, (g, rot) in {(3, n/2), (5, n/4), one seeded pair}, outputs compared in full first; n = 4096 / 60-bit,
 * 65,536 rows and n = 1024 / 24-bit, 4,096 rows; the README has the table):
 *   - a pack level: the one launch is faster than the explicit route, its three torch passes included, at all six points and for every g
 *     by disjoint ranges, x 0.21 - 0.27 at n = 4096 (5,667 - 5,684 against 26,868 - 26,903 us at two terms) and x 0.25 - 0.32 at
 *     n = 1024 (53.5 - 53.7 against 216.0 - 216.3 us), and faster than the route's two launches alone, x 0.90 - 0.94, at all six.
 *   - against a plain tn_poly_galois_keyswitch_prepared_dev on the same rows it is SLOWER at all six by disjoint ranges, x 1.18 - 1.26
 *     at n = 4096 and x 1.11 - 1.16 at n = 1024: the second input ciphertext, read twice, and the sums.
 *   - a trace step (od == NULL): x 0.41 - 0.56 of its route (the key switch and one torch addition) at all six by disjoint ranges;
 *     x 1.03 - 1.05 of the plain key switch at n = 4096 (disjoint), x 1.01 - 1.03 at n = 1024 (within the spread at three and four terms).
 *   - not measured: n = 256, n = 8192, a key per row, unsigned digits, the canonical policy.
 */
tn_status tn_poly_pack_step_prepared_dev(tn_plan *plan, const void *ev, const void *od, uint32_t rot, uint32_t galois, const void *bhat,
                                         size_t bhat_sets, void *c, size_t batch, size_t terms, uint32_t base_log, uint32_t flags,
                                         void *stream);

/*
 * THE LWE ENDS OF A PROGRAMMABLE BOOTSTRAP: the modulus switch that turns an LWE ciphertext into the exponents of a blind
 * rotation (tn_lwe_modswitch_dev), the sample extraction that takes an LWE ciphertext out of the rotated accumulator
 * (tn_sample_extract_dev) and the LWE-to-LWE key switch back to the small key (tn_lwe_keyswitch_dev).  With tn_monomial_mul_dev
 * and tn_poly_blind_rotate_prepared_dev (or a loop over tn_poly_cmux_rotate_prepared_dev) they make a TFHE-style bootstrap that
 * never leaves the library: LWE ciphertexts in, LWE ciphertexts under the same key out.
 *
 * Conventions.
 *   - An LWE ciphertext of dimension d is a row of d + 1 words of the plan's element type, a_0 .. a_{d-1}, b.  Rows are dense,
 *     [batch][d + 1].  Its phase is b + sum_i a_i s_i mod q.
 *   - An RLWE ciphertext is [2][n] with phase c0 + c1 s: the convention tn_poly_galois_keyswitch_prepared_dev implies.
 *   - With these the three calls and the blind rotation compose without a negation.  A caller with the b - <a, s> convention
 *     negates the key.
 *   - Every input word is taken mod q (any word value is accepted); outputs are canonical residues in [0, q).
 *   - All three calls work on EVERY plan (general and omega-only plans included): they need only n, q and the element width,
 *     as tn_gadget_decompose_dev and tn_automorphism_dev do.  LWE dimensions are independent of n and at most TN_LWE_MAX_DIM.
 *
 * tn_lwe_modswitch_dev: lwe is [batch][dim + 1]; exps is a device uint32_t array [dim + 1][batch], TRANSPOSED on purpose: rows
 * 0 .. dim - 1 are exactly the exps operand of tn_poly_blind_rotate_prepared_dev (steps = dim), row dim is the body's exponent,
 * for tn_monomial_mul_dev.  exps[i][r] = floor((2n x + floor(q / 2)) / q) mod 2n with x = lwe[r][i] mod q and n the plan's,
 * computed exactly (2n x does not fit a word: long division, one quotient bit per step).
 *
 * tn_sample_extract_dev: a is [batch][2][n], lwe is [batch][n + 1]; index is passed by value and must be below n.
 *     lwe[r][i] = a[r][1][index - i] mod q                      for i <= index,
 *     lwe[r][i] = (q - a[r][1][n + index - i] mod q) mod q      for index < i < n   (a zero stays 0),
 *     lwe[r][n] = a[r][0][index] mod q.
 * The phase of lwe[r] under the coefficients of s is coefficient `index` of a[r][0] + a[r][1] s.  The kernel's index into a row
 * is masked besides: no value of index could cause an out-of-bounds access.
 *
 * tn_lwe_keyswitch_dev: lwe is [batch][n_in + 1]; ksk is [n_in][terms][n_out + 1] words of the plan's type, a plain array (any
 * word values), not a prepared operand; out is [batch][n_out + 1]:
 *     out[r][k] = ( [k == n_out] b_r + sum_{i < n_in} sum_{j < terms} d_j(a_r[i]) * ksk[i][j][k] ) mod q,
 * a_r[i] = lwe[r][i] mod q, b_r = lwe[r][n_in] mod q.  d_j is the library's own digit (GADGET decomposition above: base 2^base_log,
 * unsigned or TN_GADGET_BALANCED with the carry running up the digits and the last carry dropped), used as a signed integer,
 * which equals its canonical residue mod q.  ksk[i][j] is an LWE encryption of s_i 2^(j base_log) under the output key.  n_in and
 * n_out are independent of the plan's n.  base_log above 32 is TN_EUNSUPPORTED (the kernel keeps digits as 32-bit words; LWE key
 * switches use bases of 2^2 to 2^8), and so is n_in * terms above 2^22 (the kernel's 128-bit sums are not reduced on the way).
 *
 * Status, in this order.  All three: TN_EINVAL a NULL plan.
 *   tn_lwe_modswitch_dev: TN_EINVAL dim outside [1, TN_LWE_MAX_DIM]; batch * (dim + 1) > 2^31 - 1; batch == 0 succeeds and
 *     launches nothing; TN_EINVAL a NULL buffer; exps overlapping lwe (byte ranges).
 *   tn_sample_extract_dev: TN_EINVAL index >= n; batch * (n + 1) > 2^31 - 1; batch == 0 succeeds; TN_EINVAL a NULL buffer; lwe
 *     overlapping a.
 *   tn_lwe_keyswitch_dev: TN_EINVAL n_in, then n_out, outside [1, TN_LWE_MAX_DIM]; everything the gadget calls refuse, in their
 *     order (terms == 0, a flag bit other than TN_GADGET_BALANCED, base_log == 0 or 2^base_log >= q, (terms - 1) * base_log >= 64,
 *     n_in * terms > 2^31 - 1); TN_EUNSUPPORTED base_log > 32; TN_EUNSUPPORTED n_in * terms > 2^22 (unreachable with today's
 *     limits, 2^16 and 64 terms: the bound stands for the day one of them grows); TN_EINVAL
 *     batch * (n_in + 1) or batch * (n_out + 1) > 2^31 - 1; batch == 0 succeeds; TN_EINVAL a NULL buffer; out overlapping lwe or ksk.
 * The calls enqueue on the stream and return; none allocates, copies or synchronises, and all may be stream-captured.
 *
 * When to use which (MI355X, profiles/lwe_ab.txt, tools/gpu_lwe.py; one process per point, 9 interleaved repeats, outputs compared
 * first; n = 1024 / 24-bit with n_out = 512 and n = 2048 / 60-bit with n_out = 768, batch 256 and 4,096; all by disjoint ranges):
 *   - the key switch at 60-bit: tn_lwe_keyswitch_dev is the only route (torch has no 128-bit sum): 2,157 us at batch 256 and 9,855 us
 *     at batch 4,096 for terms 4, w 15 (0.75 and 2.6 T multiply-adds / s), 4 - 8 % of the whole Plan.bootstrap on the same rows.
 *   - the key switch at 24-bit: a float64 torch.matmul on digits cut in torch (exact while the sums stay below 2^53) is FASTER at
 *     all four points, x 3.6 - 6.4 (98 against 633 us at batch 256, terms 3, w 8; 771 against 2,980 us at batch 4,096, terms 6, w 4):
 *     use it there.  It is also the figure a matrix-core formulation of this call starts from.
 *   - batch 256 runs at a seventh to a third of batch 4,096's multiply-add rate: 96 - 128 workgroups on 256 CUs; no split over i exists.
 *   - the two element-wise calls take 9 - 28 us per call, the enqueue through Python included, x 1.7 - 6.8 of a device-to-device copy
 *     of the same bytes (3 - 17 us).  The modulus switch takes the same 15 us at batch 256 and 4,096: most of that is not the kernel;
 *     the cause was not isolated.
 *   - not measured: n = 256, n = 8192, the canonical policy, other n_out, balanced key-switch digits.
 *
 * No *_host form, no tn_multi_* form, no key-switch key per row, no modulus switch to anything but the plan's 2n, no RLWE-to-LWE
 * packing.  The reference has no counterpart.
 */
#define TN_LWE_MAX_DIM 65536
tn_status tn_lwe_modswitch_dev(tn_plan *plan, const void *lwe, uint32_t *exps, size_t batch, size_t dim, void *stream);
tn_status tn_sample_extract_dev(tn_plan *plan, const void *a, void *lwe, size_t batch, uint32_t index, void *stream);
/*
 * tn_lwe_embed_dev: the exact inverse of tn_sample_extract_dev at `index` (below n): lwe is [batch][n + 1], a is [batch][2][n],
 *     a[r][1][k] = lwe[r][index - k] mod q                      for k <= index,
 *     a[r][1][k] = (q - lwe[r][n + index - k] mod q) mod q      for index < k < n   (a zero stays 0),
 *     a[r][0][index] = lwe[r][n] mod q, a[r][0][k] = 0 elsewhere.
 * Coefficient `index` of the phase of a[r] is the phase of lwe[r] under the coefficients of s (the other coefficients are not
 * zero: a trace removes them).  Every plan; status as tn_sample_extract_dev with the two buffers in each other's place; the
 * index into the row is masked besides.  Enqueues and returns, does not allocate, may be stream-captured.
 */
tn_status tn_lwe_embed_dev(tn_plan *plan, const void *lwe, void *a, size_t batch, uint32_t index, void *stream);
tn_status tn_lwe_keyswitch_dev(tn_plan *plan, const void *lwe, const void *ksk, void *out, size_t batch, size_t n_in, size_t n_out,
                               size_t terms, uint32_t base_log, uint32_t flags, void *stream);

/*
 * THE LWE KEY SWITCH ON THE MATRIX CORES: the key prepared once as signed bytes (tn_lwe_ksk_prepare_dev), then any number of key
 * switches with it (tn_lwe_keyswitch_prepared_dev) on the gfx950 int8 matrix instruction (v_mfma_i32_16x16x64_i8) with exact sums.
 *
 * Contract: out of tn_lwe_keyswitch_prepared_dev is word for word what tn_lwe_keyswitch_dev writes for the same lwe, the plain
 * ksk that kprep was prepared from and the same terms, base_log and flags, on every plan and for any input words.  Both compute
 * the same integer sum mod q; nothing is approximate.
 *
 * The prepared key is opaque and belongs to the plan (its q) and the build, as prepared operands do.  It is a pure function of
 * (q, ksk mod q, n_in, n_out, terms): every key word is made canonical, replaced by its centred residue in (-q/2, q/2] and cut,
 * from the low end, into L(q) balanced base-256 limbs in [-128, 128).  L limbs hold -128 (256^L - 1) / 255 .. 127 (256^L - 1) / 255,
 * so L(q) is the smallest L with floor(q / 2) <= 127 (256^L - 1) / 255: 3 for q = 8380417 (the canonical residue would not fit:
 * 127 (2^24 - 1) / 255 = 8355711 < q - 1), 8 for q = 2^60 - 2^14 + 1.  The limb planes lie in the matrix instruction's operand
 * order, [ceil((n_out + 1) / 16)][ceil(n_in * terms / 64)][L][64 lanes][16 bytes], the padding filled with zero limbs:
 * tn_lwe_ksk_prepared_bytes gives the size, padding included (host only; nothing is launched).  kprep must be aligned to 16 bytes.
 *
 * Digits are the library's own, as signed bytes: unsigned digits need base_log <= 7, TN_GADGET_BALANCED needs base_log <= 8;
 * wider digits are TN_EUNSUPPORTED (tn_lwe_keyswitch_dev is the route).  n_in, n_out, terms and n_in * terms keep the limits of
 * tn_lwe_keyswitch_dev (terms <= 64 for the two calls without a base_log).
 *
 * Status, in this order.  All three: TN_EINVAL a NULL plan; n_in, then n_out, outside [1, TN_LWE_MAX_DIM].
 *   tn_lwe_ksk_prepared_bytes, tn_lwe_ksk_prepare_dev: TN_EINVAL terms == 0, terms > 64, n_in * terms > 2^31 - 1; TN_EUNSUPPORTED
 *     n_in * terms > 2^22; then TN_EINVAL a NULL bytes, or a NULL buffer, kprep not aligned to 16 bytes, kprep (its
 *     tn_lwe_ksk_prepared_bytes) overlapping ksk.
 *   tn_lwe_keyswitch_prepared_dev: everything the gadget calls refuse, in their order, as tn_lwe_keyswitch_dev; TN_EUNSUPPORTED
 *     digits wider than a signed byte; TN_EUNSUPPORTED n_in * terms > 2^22; TN_EINVAL batch * (n_in + 1) or batch * (n_out + 1)
 *     > 2^31 - 1; batch == 0 succeeds and launches nothing; TN_EINVAL a NULL buffer; kprep not aligned to 16 bytes; out overlapping
 *     lwe or kprep.  The call cannot see how many bytes lie behind kprep: the caller vouches for tn_lwe_ksk_prepared_bytes of them.
 * The two device calls enqueue on the stream and return; neither allocates, copies or synchronises, and both may be stream-captured.
 * When to use which: README, "LWE ends of the bootstrap" (profiles/lwe_mfma_ab.txt, tools/gpu_lwe_mfma.py).
 */
tn_status tn_lwe_ksk_prepared_bytes(tn_plan *plan, size_t n_in, size_t n_out, size_t terms, size_t *bytes);
tn_status tn_lwe_ksk_prepare_dev(tn_plan *plan, const void *ksk, void *kprep, size_t n_in, size_t n_out, size_t terms, void *stream);
tn_status tn_lwe_keyswitch_prepared_dev(tn_plan *plan, const void *lwe, const void *kprep, void *out, size_t batch, size_t n_in, size_t n_out,
                                        size_t terms, uint32_t base_log, uint32_t flags, void *stream);

/*
 * The *_host entry points cut the batch into chunks that flow H2D -> kernel -> D2H on three
 * streams through a fixed set of device staging slots (copies overlap the kernels when the host
 * buffers are pinned; device staging stays bounded whatever the batch).  rows = rows per chunk,
 * 0 = automatic (32 MiB per operand).  No counterpart in the reference (its callers hand over
 * Python lists / std::vector, cg_ntt.py:78, benchmark_ntt_60bit.cpp:148).
 */
tn_status tn_plan_set_host_chunk_rows(tn_plan *plan, size_t rows);

/*
 * Untwisted cyclic transforms with omega = psi^2, natural order in and out.
 * tn_ntt_forward_*  replaces cg_ntt(a_prime, omega_n, modulus)  (cg_ntt.py:29-65),
 *                   cg_ntt_8butterfly (cg_ntt_8butterfly.py:41-97) with TN_VARIANT_CG8.
 * tn_ntt_inverse_*  replaces cg_intt(A, omega_n, modulus)       (cg_ntt.py:68-75).
 * TN_VARIANT_AUTO / FUSED: register-tiled kernel (merged transform + one extra LDS transpose for natural order);
 * CG variants: the reference's stage sweep.  Identical results.
 */
tn_status tn_ntt_forward_dev(tn_plan *plan, const void *in, void *out, size_t batch, tn_variant variant, void *stream);
tn_status tn_ntt_inverse_dev(tn_plan *plan, const void *in, void *out, size_t batch, tn_variant variant, void *stream);
tn_status tn_ntt_forward_host(tn_plan *plan, const void *in, void *out, size_t batch, tn_variant variant);
tn_status tn_ntt_inverse_host(tn_plan *plan, const void *in, void *out, size_t batch, tn_variant variant);

/*
 * Forward transform of ONE polynomial that also returns every stage's output:
 * trace is [log2 n][n] elements, row s-1 = the list `A` after stage s — the
 * data cg_ntt(..., verbose=True) prints 16-at-a-time (cg_ntt.py:60-62).  CG variants only (AUTO = CG here):
 * the stages observed are the reference's constant-geometry stages.
 */
tn_status tn_ntt_forward_trace_host(tn_plan *plan, const void *in, void *out, void *trace, tn_variant variant);

/*
 * twist + forward transform: the reference's second timed unit,
 * forward_ntt_bench(a, out) (benchmark_ntt_60bit.cpp:161-165).
 */
tn_status tn_twisted_ntt_forward_dev(tn_plan *plan, const void *in, void *out, size_t batch, tn_variant variant, void *stream);
tn_status tn_twisted_ntt_forward_host(tn_plan *plan, const void *in, void *out, size_t batch, tn_variant variant);

/*
 * Untwisted (CYCLIC) product: cg_ntt(a), cg_ntt(b), pointwise, cg_intt with omega = psi^2 —
 * python_poly_mult (test/cocotb_tests/test_ntt_poly_mult.py:38-43), i.e. what the reference's
 * RTL top level / RoCC accelerator computes.  TN_VARIANT_FUSED runs the fused
 * product kernel on the twiddle tables of the x^n - 1 factorisation tree (no twist anywhere).
 */
tn_status tn_cyclic_poly_mult_dev(tn_plan *plan, const void *a, const void *b, void *c, size_t batch,
                                  tn_variant variant, void *stream);

/* c[i] = a[i] * b[i] mod q over batch*n coefficients: pointwise_mul (benchmark_ntt_60bit.cpp:142-146; cg_ntt.py:88). */
tn_status tn_pointwise_mul_dev(tn_plan *plan, const void *a, const void *b, void *c, size_t batch, void *stream);

/*
 * O(n^2) direct negacyclic product on device — negacyclic_mul_reference (benchmark_ntt_60bit.cpp:167-180),
 * the benchmark_simple family, negacyclic_convolution (new_reference/test_cg_ntt.py:11-21).  An
 * independent on-device checker for the NTT path; not a throughput kernel.
 */
tn_status tn_schoolbook_dev(tn_plan *plan, const void *a, const void *b, void *c, size_t batch, void *stream);
tn_status tn_schoolbook_host(tn_plan *plan, const void *a, const void *b, void *c, size_t batch);

/*
 * Copy one of the plan's constant tables to the host as uint64_t values (the constants only,
 * without their Barrett factors).  which: 0 psi^i [n] (= rtl/twiddle_forward*.hex), 1 psi^-i * n^-1 [n],
 * 2 omega^j [n/2], 3 omega^-j [n/2], 4 psi^brv(i) [n], 5 psi^-brv(i) [n], 6 psi^-i [n] (= rtl/twiddle_inverse*.hex).
 */
tn_status tn_plan_export_table(tn_plan *plan, int which, void *host_out);

/*
 * Synthetic inputs and digests, on device, in the reference benchmark's own
 * conventions so runs can be diffed against its printed checksums:
 * tn_fill_lcg_dev: row r gets make_poly(seed0 + r * seed_stride)
 *                  (benchmark_ntt_60bit.cpp:79-87; benchmark_ntt.cpp:82-90 when q < 2^32).
 * tn_checksum_rows_dev: out[r] = checksum(row r)  (benchmark_ntt_60bit.cpp:182-188;
 *                  benchmark_ntt.cpp:228-233 when q < 2^32).  out is a DEVICE uint64_t[batch].
 */
tn_status tn_fill_lcg_dev(tn_plan *plan, void *dst, size_t batch, uint64_t seed0, uint64_t seed_stride, void *stream);
tn_status tn_checksum_rows_dev(tn_plan *plan, const void *src, uint64_t *out, size_t batch, void *stream);

/* Blocks until everything enqueued on the plan's own stream has finished. */
tn_status tn_plan_synchronize(tn_plan *plan);

/*
 * Times `iters` back-to-back launches of tn_poly_mult_dev on the plan's own
 * stream with HIP events recorded on that stream (hipEventRecord); returns the
 * mean milliseconds per launch.  (bench.py uses this so the timed region is
 * measured on the stream the kernel runs on.)
 */
tn_status tn_time_poly_mult_dev(tn_plan *plan, const void *a, const void *b, void *c, size_t batch,
                                tn_variant variant, int iters, float *ms_per_launch);

/* Name of the kernel a variant resolves to for this plan (for matching rocprof rows). */
const char *tn_kernel_name(const tn_plan *plan, tn_variant variant);

/*
 * One call sharded over several devices.  Polynomial pairs are independent: the batch is cut into contiguous
 * row blocks (tn_shard_rows: block sizes differ by at most one row), one block per entry; every entry has its OWN plan and stream
 * on its device; there is no collective and no exchange.  devices == NULL: every visible device once.  A device may be listed
 * several times (each entry still gets its own plan and stream).  The reference has no counterpart (single-threaded, one host).
 *   tn_multi_poly_mult_host  host buffers [batch][n]: one host thread per entry runs the H2D -> kernel -> D2H pipeline of its block.
 *   tn_multi_poly_mult_dev   operands already resident per device: a[i], b[i], c[i] hold rows[i] rows on entry i's device; the
 *                            launches are enqueued on the entries' own streams; tn_multi_synchronize waits for all of them.
 * Errors: the first failing entry's status; tn_multi_last_error() names the entry and carries its message.
 */
typedef struct tn_multi tn_multi;
tn_status tn_shard_rows(size_t batch, int parts, int index, size_t *first_row, size_t *rows);
tn_status tn_multi_create(tn_multi **out, uint32_t n, uint64_t q, uint64_t psi, const int *devices, int ndevices, uint32_t flags);
tn_status tn_multi_destroy(tn_multi *m);
int tn_multi_size(const tn_multi *m);
tn_plan *tn_multi_plan(tn_multi *m, int index);   /* entry index's plan (owned by m) */
int tn_multi_device(const tn_multi *m, int index);
tn_status tn_multi_poly_mult_host(tn_multi *m, const void *a, const void *b, void *c, size_t batch, tn_variant variant);
tn_status tn_multi_poly_mult_dev(tn_multi *m, const void *const *a, const void *const *b, void *const *c, const size_t *rows,
                                 tn_variant variant);
tn_status tn_multi_synchronize(tn_multi *m);
const char *tn_multi_last_error(void);

const char *tn_last_error(void);
const char *tn_status_string(tn_status s);
int tn_version(void);
/* First 16 hex digits of the sha256 of the sources this library was built from (csrc/Makefile); lets a stored
 * measurement (profiles/traffic_latest.json) say which build it was taken on.  No counterpart in the reference. */
const char *tn_build_id(void);

#ifdef __cplusplus
}
#endif
#endif /* TINYNTT_H */
