// plan.h — internal plan object behind the opaque tn_plan handle, the one launch path of the
// persistent kernels (launch_persistent) and the kernel launch entry points implemented in the kernels*.hip files.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <atomic>
#include <mutex>
#include "launch_plan.h"

struct tn_plan {
  tn::u32 n = 0, logn = 0;
  tn::u64 q = 0, psi = 0, omega = 0;
  int device = 0;
  int num_cus = 256;
  tn::u32 flags = 0;
  int elem_bytes = 8;
  bool has_fused = false, lazy = false, cg_lazy = false, cg_sched = false;
  bool bc_ok = false;              // the n = 4096 / 64-bit lazy product kernel runs the base case (HostTables::bc_ok)
  bool canonical_inputs = false;   // TN_PLAN_CANONICAL_INPUTS was given and the fused product kernel has a schedule for it (else the flag is ignored)
  bool omega_only = false;   // created by tn_plan_create_omega: no psi, only the constant-geometry transforms
  bool general = false;      // created by tn_plan_create_general: psi / q not validated, tables computed literally (cg_ntt.py:78-92 for ANY psi)
  int k = 0;            // bitlen(q)
  tn::Arith<tn::u64> ar64 = {};    // kernel-argument constants (h_make_arith); the one matching elem_bytes is used
  tn::Arith<tn::u32> ar32 = {};
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  // host-buffer entry points: chunks flow H2D (copy_in) -> kernel (stream) -> D2H (copy_out) through HOST_SLOTS
  // device staging slots; created on first use
  static constexpr int HOST_SLOTS = 3;
  hipStream_t copy_in = nullptr, copy_out = nullptr;
  hipEvent_t ev_in[HOST_SLOTS] = {}, ev_k[HOST_SLOTS] = {}, ev_out[HOST_SLOTS] = {};
  size_t host_chunk_rows = 0;      // rows per chunk; 0 = automatic (HOST_CHUNK_BYTES per operand)
  // device tables (Tw32[] or Tw64[] according to elem_bytes): split-constant records when the plan is lazy with 64-bit
  // lanes (h_make_fused_tw; the constant-geometry kernels then run their SPLIT instantiation), Shoup records
  // {w, floor(w 2^W / q)} otherwise.
  void* d_psi_brv = nullptr;       // [n]   psi^brv(i): merged forward twiddles (fused kernel)
  void* d_psi_inv_brv = nullptr;   // [n]   psi^-brv(i)
  void* d_omega_pow = nullptr;     // [n/2] omega^j   (cg_ntt.py:51,54 — pow(omega_s, i//k) = omega^(k*(i//k)))
  void* d_omega_inv_pow = nullptr; // [n/2] omega^-j
  void* d_psi_pow = nullptr;       // [n]   psi^i     (twist, cg_ntt.py:82-83)
  void* d_psi_inv_pow = nullptr;   // [n]   psi^-i
  void* d_cyc_brv = nullptr;       // [n]   merged twiddles of the cyclic transform (HostTables::cyc_brv): fused cg_ntt
  void* d_cyc_inv_brv = nullptr;   // [n]   their inverses: fused cg_intt
  void* d_psi_bc = nullptr;        // [n]   psi_brv / cyc_brv with the last level squared: forward tables of the base-case product
  void* d_cyc_bc = nullptr;        //       kernel (HostTables::psi_bc; bc_ok plans only)
  void* d_psi_inv_ninv = nullptr;  // [n]   psi^-i * n^-1  (untwist :92 fused with the n^-1 of :74-75)
  // Host-side mutable state (staging scratch, the host pipeline's streams / events, ev0 / ev1 of the timing helper): the
  // *_host entry points and tn_time_poly_mult_dev take this lock, so two host threads may share one plan; *_dev entry
  // points touch none of it.
  mutable std::mutex host_mu;
  // dynamic row scheduling of the persistent fused kernel: SCHED_SLOTS pairs {next row, finished workgroups}, zeroed at
  // plan creation and re-armed by the kernel itself; consecutive launches take consecutive slots
  // a slot is handed out again only after the launch that used it last has retired (an event per slot, queried on reuse:
  // sched_acquire); while it is still busy the new launch falls back to the fixed stride, which is always correct
  static constexpr unsigned SCHED_SLOTS = 1024;     // launches that can be in flight with dynamic scheduling before the fallback applies
  tn::u32* d_sched = nullptr;
  mutable std::mutex sched_mu;
  mutable unsigned sched_seq = 0;
  mutable hipEvent_t sched_ev[SCHED_SLOTS] = {};
  mutable bool sched_used[SCHED_SLOTS] = {};
  void* d_scratch = nullptr;       // host-entry staging (grown on demand)
  size_t scratch_bytes = 0;
};

namespace tn {

enum CgMode { CG_NTT_FWD = 0, CG_NTT_INV = 1, CG_POLYMUL = 2, CG_TWIST_FWD = 3, CG_CYCLIC_POLYMUL = 4 };

template <typename E> struct PlanView {
  typedef typename TwOf<E>::type Tw;
  u32 n, logn;
  Arith<E> ar;
  const Tw* psi_brv;
  const Tw* psi_inv_brv;
  const Tw* omega_pow;
  const Tw* omega_inv_pow;
  const Tw* psi_pow;
  const Tw* psi_inv_ninv;
  const Tw* psi_inv_pow;
  const Tw* cyc_brv;
  const Tw* cyc_inv_brv;
  const Tw* psi_bc;
  const Tw* cyc_bc;
};

template <typename E> inline const Arith<E>& plan_arith(const tn_plan* p);
template <> inline const Arith<u64>& plan_arith<u64>(const tn_plan* p) { return p->ar64; }
template <> inline const Arith<u32>& plan_arith<u32>(const tn_plan* p) { return p->ar32; }

template <typename E> inline PlanView<E> make_view(const tn_plan* p) {
  typedef typename TwOf<E>::type Tw;
  PlanView<E> v;
  v.n = p->n; v.logn = p->logn;
  v.ar = plan_arith<E>(p);
  v.psi_brv = (const Tw*)p->d_psi_brv; v.psi_inv_brv = (const Tw*)p->d_psi_inv_brv;
  v.omega_pow = (const Tw*)p->d_omega_pow; v.omega_inv_pow = (const Tw*)p->d_omega_inv_pow;
  v.psi_pow = (const Tw*)p->d_psi_pow; v.psi_inv_ninv = (const Tw*)p->d_psi_inv_ninv;
  v.psi_inv_pow = (const Tw*)p->d_psi_inv_pow;
  v.cyc_brv = (const Tw*)p->d_cyc_brv; v.cyc_inv_brv = (const Tw*)p->d_cyc_inv_brv;
  v.psi_bc = (const Tw*)p->d_psi_bc; v.cyc_bc = (const Tw*)p->d_cyc_bc;
  return v;
}

// the device table a fused launch's setup names (launch_plan.h)
template <typename E> inline const typename TwOf<E>::type* fused_table(const PlanView<E>& v, FusedTable t) {
  switch (t) {
    case FT_PSI_BRV: return v.psi_brv;
    case FT_PSI_INV_BRV: return v.psi_inv_brv;
    case FT_CYC_BRV: return v.cyc_brv;
    case FT_CYC_INV_BRV: return v.cyc_inv_brv;
    case FT_PSI_BC: return v.psi_bc;
    case FT_CYC_BC: return v.cyc_bc;
  }
  return nullptr;
}

// Dynamic-row-scheduler slot for one launch on stream s, or nullptr (fixed stride, always correct) when
//   * the stream is being captured into a graph: a captured launch would bake the slot pointer into its kernel node while
//     the ring keeps advancing, so a later replay could share a counter pair with a live launch (rows skipped); and
//     hipEventQuery is not allowed while capturing;
//   * the ring's next slot is still in use by an earlier launch (possible across streams).
// A slot counts as used only once its event HAS BEEN RECORDED behind the launch (sched_release, under the same lock as the
// hand-out): sched_acquire returns with the lock held and sched_release drops it, so no other thread can see a slot that
// is handed out but whose event does not yet cover the launch.
struct SchedSlot { u32* ptr = nullptr; int index = -1; bool locked = false; };
inline SchedSlot sched_acquire(const tn_plan* p, hipStream_t stream) {
  SchedSlot r;
  if (!p->d_sched) return r;
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(stream, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) return r;
  p->sched_mu.lock();
  const unsigned i = p->sched_seq % tn_plan::SCHED_SLOTS;
  bool ok = !(p->sched_used[i] && hipEventQuery(p->sched_ev[i]) != hipSuccess);       // still running (or errored): do not share it
  if (ok && !p->sched_ev[i]) ok = hipEventCreateWithFlags(&p->sched_ev[i], hipEventDisableTiming) == hipSuccess;
  if (!ok) { p->sched_mu.unlock(); return r; }
  r.ptr = p->d_sched + 2 * i; r.index = (int)i; r.locked = true;
  return r;
}
// launched: the kernel that uses the slot was enqueued (a failed launch leaves the slot free and the ring where it was)
inline void sched_release(const tn_plan* p, const SchedSlot& s, hipStream_t stream, bool launched = true) {
  if (!s.locked) return;
  if (launched) {
    if (hipEventRecord(p->sched_ev[s.index], stream) == hipSuccess) p->sched_used[s.index] = true;
    else (void)hipStreamSynchronize(stream);       // nothing can tell later when the kernel has finished: wait for it now, the slot stays free
    ++p->sched_seq;
  }
  p->sched_mu.unlock();
}

// Launch a persistent kernel: as many workgroups as can be resident (occupancy query), each looping over rows that come in
// chunks, from a device counter or at a fixed stride (plan_rows).  enqueue(grid, sched, chunk) launches the kernel with its
// own arguments and returns the launch's status; sched is the launch's counter pair (one per launch in flight: ring, each
// pair is re-armed by the kernel that used it) or nullptr for the fixed stride.
template <typename Enqueue>
inline hipError_t launch_persistent(const tn_plan* p, hipStream_t s, const void* kern, u32 threads, size_t lds_bytes, size_t row_bytes,
                                    size_t batch, const RowPolicy& rows, Enqueue&& enqueue) {
  if (lds_bytes > 48 * 1024) {
    hipError_t e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    if (e != hipSuccess) return e;
  }
  int per_cu = 0;
  hipError_t qe = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, (int)threads, lds_bytes);
  if (qe != hipSuccess || per_cu < 1) per_cu = 1;
  const size_t resident = (size_t)per_cu * (size_t)p->num_cus;
  const RowPlan rp = plan_rows(row_bytes, batch, resident, rows);
  u32 chunk = rp.chunk;
  const size_t chunks = (batch + chunk - 1) / chunk;
  const u32 grid = (u32)(chunks < resident ? chunks : resident);
  SchedSlot slot;
  if (rp.dynamic) slot = sched_acquire(p, s);
  if (!slot.ptr && rows.single_rows_without_slot) chunk = 1;
  const hipError_t le = enqueue(grid, slot.ptr, chunk);
  sched_release(p, slot, s, le == hipSuccess);
  return le;
}

// kernels.hip (prepared operand: kernels_prepared.hip; transform domain: kernels_hat.hip; gadget: kernels_gadget.hip;
// automorphisms: kernels_galois.hip; external product: kernels_extprod.hip; CMux rotation step: kernels_cmux.hip; blind rotation: kernels_blindrot.hip;
// automorphism key switch: kernels_galoisks.hip; pack / trace step: kernels_pack.hip; LWE modulus switch, sample extraction, embedding and key switch: kernels_lwe.hip; the key
// switch from a prepared key on the matrix cores: kernels_lwe_mfma.hip)
bool fused_supported(u32 logn, int elem_bytes);
const char* fused_kernel_name(const tn_plan* p);
const char* cg_kernel_name(const tn_plan* p, int group, int layout);
hipError_t launch_polymul_fused(const tn_plan* p, const void* a, const void* b, void* c, size_t batch, hipStream_t s, bool cyclic = false);
hipError_t launch_ntt_fused(const tn_plan* p, int mode, const void* in, void* out, size_t batch, hipStream_t s);
// prepared operand (tn_prepare_dev / tn_poly_mult_prepared_dev; fused plans only).  shared: every row is multiplied by bhat's row 0
hipError_t launch_prepare(const tn_plan* p, const void* b, void* bhat, size_t rows, hipStream_t s);
hipError_t launch_polymul_prepared(const tn_plan* p, const void* a, const void* bhat, bool shared, void* c, size_t batch, hipStream_t s);
// prepared dot product (tn_poly_dot_prepared_dev): c[r] = sum_j a[r][j] * b[shared ? 0 : r][j]; terms == 1 is launch_polymul_prepared
hipError_t launch_polydot_prepared(const tn_plan* p, const void* a, const void* bhat, bool shared, void* c, size_t batch, size_t terms,
                                   hipStream_t s);
// transform domain (tn_unprepare_dev / tn_poly_dot_hat_dev): prepared rows in; coefficients out, or prepared rows (out_prepared)
hipError_t launch_unprepare(const tn_plan* p, const void* xhat, void* x, size_t rows, hipStream_t s);
hipError_t launch_polydot_hat(const tn_plan* p, const void* ahat, const void* bhat, bool shared, void* out, size_t batch, size_t terms,
                              bool out_prepared, hipStream_t s);
// gadget decomposition (tn_gadget_decompose_dev: every plan) and the dot product that decomposes a itself
// (tn_poly_gadget_dot_prepared_dev: fused plans only): c[r] = sum_j digit_j(a[r]) * b[shared ? 0 : r][j]
hipError_t launch_gadget_decompose(const tn_plan* p, const void* a, void* digits, size_t batch, size_t terms, tn::u32 base_log, bool balanced,
                                   hipStream_t s);
hipError_t launch_polydot_gadget(const tn_plan* p, const void* a, const void* bhat, bool shared, void* c, size_t batch, size_t terms,
                                 tn::u32 base_log, bool balanced, hipStream_t s);
// ... with two output components from one forward transform per term (tn_poly_gadget_multidot_prepared_dev, outs == 2):
// c[r][o] = sum_j digit_j(a[r]) * b[shared ? 0 : r][o][j], o < 2
hipError_t launch_polydot_gadget2(const tn_plan* p, const void* a, const void* bhat, bool shared, void* c, size_t batch, size_t terms,
                                  tn::u32 base_log, bool balanced, hipStream_t s);
// external product (kernels_extprod.hip; tn_poly_external_product_prepared_dev, ins >= 2 and outs == 2): the digits of all `ins`
// input polynomials of a row into both components, c[r][o] = sum_i sum_j digit_j(a[r][i]) * b[shared ? 0 : r][o][i][j], o < 2
hipError_t launch_polydot_extprod(const tn_plan* p, const void* a, const void* bhat, bool shared, void* c, size_t batch, size_t ins, size_t terms,
                                  tn::u32 base_log, bool balanced, hipStream_t s);
// CMux rotation step (kernels_cmux.hip).  tn_monomial_mul_dev, every plan: out[item][g] = X^e * a[item][g], or (X^e - 1) * with
// minus_one, e = exps[item] & (2n - 1) read on the device, g < group.  tn_poly_cmux_rotate_prepared_dev, fused plans only:
// c[r][o] = a[r][o] + sum_{i < 2} sum_j digit_j((X^e_r - 1) * a[r][i]) * b[shared ? 0 : r][o][i][j], o < 2
hipError_t launch_monomial_mul(const tn_plan* p, const void* a, const uint32_t* exps, void* out, size_t batch, size_t group, bool minus_one, hipStream_t s);
hipError_t launch_polydot_cmux(const tn_plan* p, const void* a, const uint32_t* exps, const void* bhat, bool shared, void* c, size_t batch, size_t terms,
                               tn::u32 base_log, bool balanced, hipStream_t s);
// blind rotation (kernels_blindrot.hip; tn_poly_blind_rotate_prepared_dev, shapes of blindrot_supported only): `steps` CMux steps
// per row with the accumulator in LDS, step k on key k (bhat [steps][2][2][terms][n], shared by every row) and exps + k * batch;
// c may be a itself
hipError_t launch_polydot_blindrot(const tn_plan* p, const void* a, const uint32_t* exps, const void* bhat, void* c, size_t batch, size_t steps,
                                   size_t terms, tn::u32 base_log, bool balanced, hipStream_t s);
// automorphism key switch (kernels_galoisks.hip; tn_poly_galois_keyswitch_prepared_dev, fused plans only): a, c [batch][2][n],
// c[r][o] = [o == 0] sigma_g(a[r][0]) + sum_j digit_j(sigma_g(a[r][1])) * b[shared ? 0 : r][o][j], o < 2; galois odd, below 2n
hipError_t launch_polydot_galoisks(const tn_plan* p, const void* a, uint32_t galois, const void* bhat, bool shared, void* c, size_t batch, size_t terms,
                                   tn::u32 base_log, bool balanced, hipStream_t s);
// pack / trace step (kernels_pack.hip; tn_poly_pack_step_prepared_dev, fused plans only): ev, od, c [batch][2][n]; with
// t = X^rot od (od == NULL: t = 0), s = ev + t, d = ev - t: c[r][o] = s[o] + [o == 0] sigma_g(d[0]) + sum_j digit_j(sigma_g(d[1])) *
// b[shared ? 0 : r][o][j], o < 2; rot below 2n, galois odd and below 2n
hipError_t launch_polydot_pack(const tn_plan* p, const void* ev, const void* od, uint32_t rot, uint32_t galois, const void* bhat, bool shared, void* c,
                               size_t batch, size_t terms, tn::u32 base_log, bool balanced, hipStream_t s);
// ring automorphisms a(x) -> a(x^g) (kernels_galois.hip): count images of every row, out[r][m] = sigma_{galois[m]}(row r); on
// coefficient rows (tn_automorphism_dev: every plan) and on prepared rows (tn_automorphism_prepared_dev: fused plans only)
hipError_t launch_automorphism(const tn_plan* p, const void* a, void* out, size_t batch, const uint32_t* galois, size_t count, hipStream_t s);
hipError_t launch_automorphism_prepared(const tn_plan* p, const void* xhat, void* out, size_t rows, const uint32_t* galois, size_t count,
                                        hipStream_t s);
// the LWE ends of a bootstrap (kernels_lwe.hip; every plan).  tn_lwe_modswitch_dev: lwe [batch][dim + 1] -> exps [dim + 1][batch],
// round(2n x / q) mod 2n.  tn_sample_extract_dev: a [batch][2][n] -> lwe [batch][n + 1], coefficient `index` (below n) of the
// phase.  tn_lwe_keyswitch_dev: out[r][k] = [k == n_out] b_r + sum_i sum_j digit_j(a_r[i]) * ksk[i][j][k], ksk [n_in][terms][n_out + 1]
hipError_t launch_lwe_modswitch(const tn_plan* p, const void* lwe, uint32_t* exps, size_t batch, size_t dim, hipStream_t s);
hipError_t launch_lwe_sample_extract(const tn_plan* p, const void* a, void* lwe, size_t batch, tn::u32 index, hipStream_t s);
// tn_lwe_embed_dev: lwe [batch][n + 1] -> a [batch][2][n], the inverse of the extraction at `index`
hipError_t launch_lwe_embed(const tn_plan* p, const void* lwe, void* a, size_t batch, tn::u32 index, hipStream_t s);
hipError_t launch_lwe_keyswitch(const tn_plan* p, const void* lwe, const void* ksk, void* out, size_t batch, size_t n_in, size_t n_out, size_t terms,
                                tn::u32 base_log, bool balanced, hipStream_t s);
// the key switch on the matrix cores (kernels_lwe_mfma.hip; every plan).  tn_lwe_ksk_prepare_dev: ksk -> kprep, int8 limb planes in
// B-fragment order (lwe_mfma_core.h).  tn_lwe_keyswitch_prepared_dev: out as launch_lwe_keyswitch writes it, from kprep
hipError_t launch_lwe_ksk_prepare(const tn_plan* p, const void* ksk, void* kprep, size_t n_in, size_t n_out, size_t terms, hipStream_t s);
hipError_t launch_lwe_keyswitch_prepared(const tn_plan* p, const void* lwe, const void* kprep, void* out, size_t batch, size_t n_in, size_t n_out,
                                         size_t terms, tn::u32 base_log, bool balanced, hipStream_t s);
hipError_t launch_cg(const tn_plan* p, int mode, int group, int layout, const void* a, const void* b, void* out,
                     void* trace, size_t batch, hipStream_t s);
hipError_t launch_pointwise(const tn_plan* p, const void* a, const void* b, void* c, size_t batch, hipStream_t s);
hipError_t launch_schoolbook(const tn_plan* p, const void* a, const void* b, void* c, size_t batch, hipStream_t s);
hipError_t launch_fill_lcg(const tn_plan* p, void* dst, size_t batch, u64 seed0, u64 stride, hipStream_t s);
hipError_t launch_checksum(const tn_plan* p, const void* src, u64* out, size_t batch, hipStream_t s);

}  // namespace tn
