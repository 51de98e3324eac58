// devprobe.cpp — TEST INFRASTRUCTURE: per-element wrappers around the arithmetic primitives of
// tiny_ntt_amd/csrc/modarith.h and fused_core.h (the headers the gfx950 kernels are compiled from, included unchanged),
// built twice from this one source by tests/devprobe/Makefile:
//   _build/libdevprobe.so       hipcc, the product's flags: every wrapper is a __global__ kernel (one element per thread,
//                               bounds-checked), one plain launch and one synchronise per call; the DEVICE branches of the
//                               headers run (__umul64hi, __brev, the opaque* register constraints, the AMDGPU lowering of
//                               the 32x32+64 multiply-add columns)
//   _build/libdevprobe_host.so  g++, no HIP: the same bodies in a loop, so the expectations of tests/test_devprobe.py can be
//                               proved without a GPU
// Constants are made the way the product makes them: Arith<E> by h_build_tables + h_make_arith, split records by
// h_make_tw64_split, Shoup records by h_make_tw64 / h_make_tw32, the fused tables' records by h_make_fused_tw.
// Operands and results travel as uint64 columns regardless of the lane width.  Nothing in tiny_ntt_amd/ loads this.
#include <stdint.h>
#include <stddef.h>
#include <string.h>
#include <utility>
#include <vector>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define DP_DEVICE 1
#else
#define DP_DEVICE 0
#endif
#include "../../tiny_ntt_amd/csrc/modarith.h"
#include "../../tiny_ntt_amd/csrc/fused_core.h"
#include "../../tiny_ntt_amd/csrc/plan_tables.h"

using namespace tn;

namespace {

// What a wrapper sees: the plan's constants, the raw (k, c) constants of q = 2^k - c, the operand and result columns.
struct Ctx {
  Arith<u64> a64;
  Arith<u32> a32;
  u64 q, mu;
  int k;
  u32 c;                 // 2^k - q where that fits 32 bits, else 0
  SplitK sk;             // as h_make_arith makes it for a split plan (32 <= k <= 60), else zeros
  const u64* in;         // [nin][n]
  u64* out;              // [nout][n]
  const Tw64* r64;       // records made on the host from the LAST operand column (64-bit lanes)
  const Tw32* r32;       // ... (32-bit lanes)
  size_t n;
};

enum Rec { REC_NONE = 0, REC_SHOUP64, REC_SHOUP32, REC_SPLIT, REC_FUSED64, REC_FUSED32 };
enum Need { NEED_NONE = 0, NEED_SPLIT64, NEED_LAZY32, NEED_CANON64, NEED_CANON32, NEED_RAWSPLIT };

#define IN(j) (c.in[(size_t)(j) * c.n + i])
#define OUT(j) (c.out[(size_t)(j) * c.n + i])
#define DP_OP(NAME, ...) struct NAME { TN_HD static void run(const Ctx& c, size_t i) { __VA_ARGS__ } };

// ---- 64-bit lanes ----
DP_OP(OpMulhi64, OUT(0) = mulhi64(IN(0), IN(1));)
DP_OP(OpMulhi64Lo2, OUT(0) = mulhi64_lo2(IN(0), IN(1));)
DP_OP(OpMulTwAcc64, OUT(0) = mul_tw_acc(IN(0), IN(1), c.r64[i], c.q);)
DP_OP(OpMulTwLazy64, OUT(0) = mul_tw_lazy((u64)IN(0), c.r64[i], c.q);)
DP_OP(OpMulTw64, OUT(0) = mul_tw((u64)IN(0), c.r64[i], c.q);)
DP_OP(OpCsub64, OUT(0) = csub((u64)IN(0), (u64)IN(1));)
DP_OP(OpMulSpAcc, OUT(0) = mul_sp_acc(IN(0), IN(1), c.r64[i], c.sk);)
DP_OP(OpMulSp, OUT(0) = mul_sp(IN(0), c.r64[i], c.sk);)
DP_OP(OpSplitRec, const Tw64 t = split_rec(IN(0), c.k, c.c, c.q); OUT(0) = t.w; OUT(1) = t.wp;)
DP_OP(OpFold64, OUT(0) = fold((u64)IN(0), c.k, c.c);)
DP_OP(OpBarrett64, OUT(0) = mulmod_barrett((u64)IN(0), (u64)IN(1), c.q, c.mu, c.k);)
DP_OP(OpSolinas, OUT(0) = mulmod_solinas_lazy(IN(0), IN(1), c.k, c.c);)
DP_OP(OpPwLazy64, OUT(0) = pointwise_lazy((u64)IN(0), (u64)IN(1), c.a64);)
DP_OP(OpBcPair, u64 a0 = IN(0); u64 a1 = IN(1); basecase_pair(a0, a1, IN(2), IN(3), c.r64[i], c.a64); OUT(0) = a0; OUT(1) = a1;)
// ---- 32-bit lanes ----
DP_OP(OpMulTwLazy32, OUT(0) = mul_tw_lazy((u32)IN(0), c.r32[i], (u32)c.q);)
DP_OP(OpMulTw32, OUT(0) = mul_tw((u32)IN(0), c.r32[i], (u32)c.q);)
DP_OP(OpCsub32, OUT(0) = csub((u32)IN(0), (u32)IN(1));)
DP_OP(OpFold32, OUT(0) = fold((u32)IN(0), c.k, c.c);)
DP_OP(OpBarrett32, OUT(0) = mulmod_barrett((u32)IN(0), (u32)IN(1), (u32)c.q, c.mu, c.k);)
DP_OP(OpBarrettLazy32, OUT(0) = mulmod_barrett_lazy((u32)IN(0), (u32)IN(1), (u32)c.q, c.mu, c.k);)
DP_OP(OpPwLazy32, OUT(0) = pointwise_lazy((u32)IN(0), (u32)IN(1), c.a32);)
// ---- both ----
DP_OP(OpBitrev, OUT(0) = bitrev((u32)IN(0), (int)IN(1));)

template <typename E> struct Lane;
template <> struct Lane<u64> {
  TN_HD static const Arith<u64>& ar(const Ctx& c) { return c.a64; }
  TN_HD static Tw64 rec(const Ctx& c, size_t i) { return c.r64[i]; }
};
template <> struct Lane<u32> {
  TN_HD static const Arith<u32>& ar(const Ctx& c) { return c.a32; }
  TN_HD static Tw32 rec(const Ctx& c, size_t i) { return c.r32[i]; }
};

// The members of Policy<E, LAZY> (fused_core.h); K / BND are the schedule constants of the butterflies.
template <typename E, bool LAZY> struct PolOps {
  typedef Policy<E, LAZY> P;
  typedef Lane<E> L;
  DP_OP(Load, OUT(0) = P::load((E)IN(0), L::ar(c));)
  DP_OP(Canon, OUT(0) = P::canon((E)IN(0), L::ar(c));)
  DP_OP(MulTwCanon, OUT(0) = P::mul_tw_canon((E)IN(0), L::rec(c, i), L::ar(c));)
  template <int K> DP_OP(Ct, E u = (E)IN(0); E v = (E)IN(1); P::template ct<K>(u, v, L::rec(c, i), L::ar(c)); OUT(0) = u; OUT(1) = v;)
  template <int B> DP_OP(Gs, E u = (E)IN(0); E v = (E)IN(1); P::template gs<B>(u, v, L::rec(c, i), L::ar(c)); OUT(0) = u; OUT(1) = v;)
  template <int B> DP_OP(GsLast, E u = (E)IN(0); E v = (E)IN(1); P::template gs_last<B>(u, v, L::ar(c)); OUT(0) = u; OUT(1) = v;)
};

#if DP_DEVICE
template <typename Op> __global__ void dp_kernel(Ctx c) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < c.n) Op::run(c, i);
}
#endif

// one plain launch (device) / one loop (host); returns the launch status
template <typename Op> int launch(const Ctx& c) {
#if DP_DEVICE
  const unsigned block = 256, grid = (unsigned)((c.n + block - 1) / block);
  hipLaunchKernelGGL((dp_kernel<Op>), dim3(grid), dim3(block), 0, 0, c);
  return (int)hipGetLastError();
#else
  for (size_t i = 0; i < c.n; ++i) Op::run(c, i);
  return 0;
#endif
}

constexpr int DP_BAD_K = -2;
template <template <int> class OpT, int... KS> int launch_k(int k, const Ctx& c, std::integer_sequence<int, KS...>) {
  int rc = DP_BAD_K;
  (void)std::initializer_list<int>{(k == KS ? (rc = launch<OpT<KS>>(c), 0) : 0)...};
  return rc;
}
// schedule constants that are instantiated: the split policy reads K q from Arith::qmul[0..16]; the others take any K
typedef std::integer_sequence<int, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16> KsSplit;
typedef std::integer_sequence<int, 1, 2, 4, 8, 16, 32, 64> KsPow2;

struct OpEntry {
  const char* name;
  int nin, nout, rec, need;
  int (*go)(int K, const Ctx&);
};

#define DP_PLAIN(NAME, OP, NIN, NOUT, REC, NEED) {NAME, NIN, NOUT, REC, NEED, [](int, const Ctx& c) { return launch<OP>(c); }}
#define DP_POLICY(PFX, E, LAZY, KS, RECF, NEED) \
  {PFX ".load", 1, 1, REC_NONE, NEED, [](int, const Ctx& c) { return launch<PolOps<E, LAZY>::Load>(c); }}, \
  {PFX ".canon", 1, 1, REC_NONE, NEED, [](int, const Ctx& c) { return launch<PolOps<E, LAZY>::Canon>(c); }}, \
  {PFX ".mul_tw_canon", 2, 1, RECF, NEED, [](int, const Ctx& c) { return launch<PolOps<E, LAZY>::MulTwCanon>(c); }}, \
  {PFX ".ct", 3, 2, RECF, NEED, [](int K, const Ctx& c) { return launch_k<PolOps<E, LAZY>::template Ct>(K, c, KS()); }}, \
  {PFX ".gs", 3, 2, RECF, NEED, [](int K, const Ctx& c) { return launch_k<PolOps<E, LAZY>::template Gs>(K, c, KS()); }}, \
  {PFX ".gs_last", 2, 2, REC_NONE, NEED, [](int K, const Ctx& c) { return launch_k<PolOps<E, LAZY>::template GsLast>(K, c, KS()); }}

const OpEntry OPS[] = {
  DP_PLAIN("mulhi64", OpMulhi64, 2, 1, REC_NONE, NEED_NONE),
  DP_PLAIN("mulhi64_lo2", OpMulhi64Lo2, 2, 1, REC_NONE, NEED_NONE),
  DP_PLAIN("mul_tw_acc64", OpMulTwAcc64, 3, 1, REC_SHOUP64, NEED_NONE),
  DP_PLAIN("mul_tw_lazy64", OpMulTwLazy64, 2, 1, REC_SHOUP64, NEED_NONE),
  DP_PLAIN("mul_tw64", OpMulTw64, 2, 1, REC_SHOUP64, NEED_NONE),
  DP_PLAIN("csub64", OpCsub64, 2, 1, REC_NONE, NEED_NONE),
  DP_PLAIN("mul_sp_acc", OpMulSpAcc, 3, 1, REC_SPLIT, NEED_RAWSPLIT),
  DP_PLAIN("mul_sp", OpMulSp, 2, 1, REC_SPLIT, NEED_RAWSPLIT),
  DP_PLAIN("split_rec", OpSplitRec, 1, 2, REC_NONE, NEED_RAWSPLIT),
  DP_PLAIN("fold64", OpFold64, 1, 1, REC_NONE, NEED_RAWSPLIT),
  DP_PLAIN("mulmod_barrett64", OpBarrett64, 2, 1, REC_NONE, NEED_NONE),
  DP_PLAIN("mulmod_solinas_lazy", OpSolinas, 2, 1, REC_NONE, NEED_RAWSPLIT),
  DP_PLAIN("pointwise_lazy64", OpPwLazy64, 2, 1, REC_NONE, NEED_RAWSPLIT),
  DP_PLAIN("basecase_pair", OpBcPair, 5, 2, REC_SPLIT, NEED_SPLIT64),
  DP_PLAIN("mul_tw_lazy32", OpMulTwLazy32, 2, 1, REC_SHOUP32, NEED_NONE),
  DP_PLAIN("mul_tw32", OpMulTw32, 2, 1, REC_SHOUP32, NEED_NONE),
  DP_PLAIN("csub32", OpCsub32, 2, 1, REC_NONE, NEED_NONE),
  DP_PLAIN("fold32", OpFold32, 1, 1, REC_NONE, NEED_NONE),
  DP_PLAIN("mulmod_barrett32", OpBarrett32, 2, 1, REC_NONE, NEED_NONE),
  DP_PLAIN("mulmod_barrett_lazy32", OpBarrettLazy32, 2, 1, REC_NONE, NEED_NONE),
  DP_PLAIN("pointwise_lazy32", OpPwLazy32, 2, 1, REC_NONE, NEED_LAZY32),
  DP_PLAIN("bitrev", OpBitrev, 2, 1, REC_NONE, NEED_NONE),
  DP_POLICY("split64", u64, true, KsSplit, REC_FUSED64, NEED_SPLIT64),
  DP_POLICY("lazy32", u32, true, KsPow2, REC_FUSED32, NEED_LAZY32),
  DP_POLICY("canon64", u64, false, KsPow2, REC_FUSED64, NEED_CANON64),
  DP_POLICY("canon32", u32, false, KsPow2, REC_FUSED32, NEED_CANON32),
};

// cfg: {q, n (transform length of the plan the constants belong to), psi, allow_lazy, raw_fold}.
// raw_fold: give Arith<u64> the fold constant and SplitK of (k, c) even where the plan of this n is not lazy (pointwise_lazy's
// precondition is h_pw_fast_ok alone).
struct Setup {
  bool ok = false;
  HostTables t;
  Ctx c;
};
bool pow2(u64 n) { return n && !(n & (n - 1)); }
void make_setup(const uint64_t* cfg, Setup& s) {
  const u64 q = cfg[0], n = cfg[1], psi = cfg[2];
  if (q < 3 || !(q & 1) || q >= ((u64)1 << 62) || !pow2(n) || n < 4 || n > 8192) return;
  s.t = h_build_tables((u32)n, q, psi, cfg[3] != 0);
  Ctx& c = s.c;
  memset(&c, 0, sizeof(c));
  c.a64 = h_make_arith<u64>(s.t);
  c.a32 = h_make_arith<u32>(s.t);
  c.q = q; c.mu = s.t.mu; c.k = s.t.k;
  const u64 cc = (((u64)1) << c.k) - q;
  c.c = cc < ((u64)1 << 32) ? (u32)cc : 0;
  if (c.k >= 32 && c.k <= 60 && c.c) {
    const int p = c.k - 31;
    c.sk.mulp = (u32)1 << p;
    c.sk.cf = (u32)((((unsigned __int128)1) << (p + 32)) % q);
    if (cfg[4]) { c.a64.fold_c = c.c; c.a64.sk = c.sk; }
  }
  s.ok = true;
}
bool rawsplit_ok(const Setup& s) {
  const Ctx& c = s.c;
  return c.k >= 32 && c.k <= 60 && c.c && ((((unsigned __int128)1) << (c.k - 31 + 32)) % c.q) < ((u64)1 << 32);
}
bool need_ok(int need, const Setup& s) {
  const HostTables& t = s.t;
  switch (need) {
    case NEED_SPLIT64: return h_uses_split(t);
    case NEED_LAZY32: return t.lazy && t.elem_bytes == 4;
    case NEED_CANON64: return !t.lazy;
    case NEED_CANON32: return !t.lazy && t.q < ((u64)1 << 31);
    case NEED_RAWSPLIT: return rawsplit_ok(s);
  }
  return true;
}
const OpEntry* find_op(const char* name) {
  for (const OpEntry& e : OPS) if (!strcmp(e.name, name)) return &e;
  return nullptr;
}

#if DP_DEVICE
struct DevBuf {
  void* p = nullptr;
  ~DevBuf() { if (p) (void)hipFree(p); }
};
#define DP_HIP(x) do { const hipError_t e_ = (x); if (e_ != hipSuccess) return 1000 + (int)e_; } while (0)
#endif

// values of one schedule constant over the fused shapes
template <typename Cfg, bool CIN, bool BC> void split_values(int member, std::vector<int>& v) {
  typedef SplitSched<Cfg, CIN, BC> S;
  constexpr int LOGN = Cfg::LOGN, R = Cfg::R;
  if (member == 0) {
    for (int s = 0; s < S::FEND; ++s) for (int r = 0; r < R; ++r) if (!(r & (1 << S::bpos_of(s)))) v.push_back(S::D.fk[s][r]);
    return;
  }
  for (int g = BC ? 1 : 0; g < LOGN; ++g) {
    const int s = LOGN - 1 - g;
    if ((member == 2) != (s == 0)) continue;
    for (int r = 0; r < R; ++r) if (!(r & (1 << S::bpos_of(s)))) v.push_back(S::D.ik[g][r]);
  }
}
template <typename P, int LOGN> void sched_values(int member, std::vector<int>& v) {
  typedef Sched<P, LOGN> S;
  if (member == 0) { v.push_back(P::TMUL); return; }
  for (int g = 0; g < LOGN; ++g) if ((member == 2) == (g == LOGN - 1)) v.push_back(S::inv_bnd(g));
}
template <int LOGN> void values_of_shape(int pol, int member, std::vector<int>& v) {
  typedef FusedCfg<u64, LOGN, fused_lpt(LOGN)> C64;
  if (pol == 0) {
    split_values<C64, false, false>(member, v);
    if (LOGN == 12) split_values<C64, true, false>(member, v);                                  // promised-canonical inputs
    if (fused_has_bc<u64, LOGN, fused_lpt(LOGN), true>()) split_values<C64, false, true>(member, v);   // base-case product
  } else if (pol == 1) sched_values<Policy<u32, true>, LOGN>(member, v);
  else if (pol == 2) sched_values<Policy<u64, false>, LOGN>(member, v);
  else sched_values<Policy<u32, false>, LOGN>(member, v);
}

}  // namespace

extern "C" {

int devprobe_is_device(void) { return DP_DEVICE; }

// 0 ok; 1 unknown primitive; 2 K / BND not instantiated; 3 bad arguments; 4 the plan of cfg does not admit the primitive;
// 1000 + hipError_t of the first HIP call that failed
int devprobe_run(const char* name, int K, const uint64_t* cfg, const uint64_t* in, int nin, uint64_t* out, int nout, size_t n) {
  const OpEntry* op = find_op(name);
  if (!op) return 1;
  if (nin != op->nin || nout != op->nout || n == 0 || n > ((size_t)1 << 24) || !cfg || !in || !out) return 3;
  Setup s;
  make_setup(cfg, s);
  if (!s.ok) return 3;
  if (!need_ok(op->need, s)) return 4;
  Ctx& c = s.c;
  c.n = n;
  // records of the constant operand: the last operand column, every entry below q
  std::vector<Tw64> r64;
  std::vector<Tw32> r32;
  const uint64_t* w = in + (size_t)(nin - 1) * n;
  if (op->rec != REC_NONE) for (size_t i = 0; i < n; ++i) if (w[i] >= c.q) return 3;
  if (op->rec == REC_SHOUP32 || op->rec == REC_FUSED32) {
    if (c.q >= ((u64)1 << 31)) return 4;
    r32.resize(n);
    for (size_t i = 0; i < n; ++i) r32[i] = op->rec == REC_SHOUP32 ? h_make_tw32(w[i], c.q) : h_make_fused_tw<u32>(w[i], s.t);
  } else if (op->rec != REC_NONE) {
    r64.resize(n);
    for (size_t i = 0; i < n; ++i)
      r64[i] = op->rec == REC_SHOUP64 ? h_make_tw64(w[i], c.q) : op->rec == REC_SPLIT ? h_make_tw64_split(w[i], c.q, c.k) : h_make_fused_tw<u64>(w[i], s.t);
  }
#if DP_DEVICE
  DevBuf din, dout, drec;
  const size_t in_bytes = (size_t)nin * n * sizeof(u64), out_bytes = (size_t)nout * n * sizeof(u64);
  const size_t rec_bytes = r64.size() * sizeof(Tw64) + r32.size() * sizeof(Tw32);
  DP_HIP(hipMalloc(&din.p, in_bytes));
  DP_HIP(hipMalloc(&dout.p, out_bytes));
  DP_HIP(hipMemcpy(din.p, in, in_bytes, hipMemcpyHostToDevice));
  DP_HIP(hipMemset(dout.p, 0xA5, out_bytes));
  if (rec_bytes) {
    DP_HIP(hipMalloc(&drec.p, rec_bytes));
    DP_HIP(hipMemcpy(drec.p, r64.empty() ? (const void*)r32.data() : (const void*)r64.data(), rec_bytes, hipMemcpyHostToDevice));
  }
  c.in = (const u64*)din.p; c.out = (u64*)dout.p;
  c.r64 = r64.empty() ? nullptr : (const Tw64*)drec.p;
  c.r32 = r32.empty() ? nullptr : (const Tw32*)drec.p;
  const int rc = op->go(K, c);
  if (rc == DP_BAD_K) return 2;
  if (rc != 0) return 1000 + rc;
  DP_HIP(hipDeviceSynchronize());
  DP_HIP(hipMemcpy(out, dout.p, out_bytes, hipMemcpyDeviceToHost));
  return 0;
#else
  c.in = in; c.out = out;
  c.r64 = r64.data(); c.r32 = r32.data();
  const int rc = op->go(K, c);
  return rc == DP_BAD_K ? 2 : rc;
#endif
}

// The plan constants the expectations need (host code in both builds).
// out[16]: 0 lazy, 1 elem_bytes, 2 k, 3 fold_c of the plan, 4 SplitK.mulp, 5 SplitK.cf, 6 n^-1, 7 n^-1 psi_inv_brv[1], 8 h_pw_fast_ok,
//          9 h_split_sched_ok(log2 n), 10 mu, 11 bc_ok, 12 raw split constants valid, 13 h_lazy_ok for 32-bit lanes
int devprobe_info(const uint64_t* cfg, uint64_t* out) {
  Setup s;
  make_setup(cfg, s);
  if (!s.ok) return 3;
  const HostTables& t = s.t;
  const u64 cc = (((u64)1) << t.k) - t.q;
  for (int i = 0; i < 16; ++i) out[i] = 0;
  out[0] = t.lazy; out[1] = (u64)t.elem_bytes; out[2] = (u64)t.k; out[3] = t.fold_c; out[4] = s.c.sk.mulp; out[5] = s.c.sk.cf;
  out[6] = t.n_inv; out[7] = t.ninv_w1; out[8] = h_pw_fast_ok(t.q, t.k, cc); out[9] = h_split_sched_ok(t.logn, t.k, cc);
  out[10] = t.mu; out[11] = t.bc_ok; out[12] = rawsplit_ok(s);
  u32 fc = 0;
  out[13] = t.q < ((u64)1 << 31) && h_lazy_ok(t.q, 4, &fc);
  return 0;
}

// SplitExact (plan_tables.h), the bound the schedules are replayed with: for every a[i], the EXCLUSIVE bound of t' of
// mul_sp_acc for a multiplicand <= a[i], as {low word, high word}; {0, 0} where the replay would refuse (H does not fit).
// data_rec = 0: a record of a constant below q (h_make_tw64_split); 1: a record made by split_rec (x not reduced).
int devprobe_sp_tmax(uint64_t q, int data_rec, const uint64_t* a, uint64_t* lo, uint64_t* hi, size_t n) {
  const int k = h_bitlen(q);
  if (k < 32 || k > 60) return 3;
  for (size_t i = 0; i < n; ++i) {
    SplitExact x(k, (((u64)1) << k) - q);
    if (!x.ok) return 4;
    const unsigned __int128 bv = (unsigned __int128)a[i] + 1;
    const unsigned __int128 t = data_rec ? x.tmax_rec(bv, x.rec_whi(), x.rec_xhi()) : x.tmax(bv);
    lo[i] = x.ok ? (u64)t : 0;
    hi[i] = x.ok ? (u64)(t >> 64) : 0;
  }
  return 0;
}

// The schedule constants the built kernels use, over every fused shape (n = 256 ... 8192).
// pol: 0 split (lazy 64-bit lanes), 1 lazy 32-bit lanes, 2 canonical 64-bit, 3 canonical 32-bit.
// member: 0 K of ct, 1 BND of gs, 2 BND of gs_last.  Returns the count written (duplicates included, at most cap).
int devprobe_sched_values(int pol, int member, int* out, int cap) {
  std::vector<int> v;
  values_of_shape<8>(pol, member, v); values_of_shape<9>(pol, member, v); values_of_shape<10>(pol, member, v);
  values_of_shape<11>(pol, member, v); values_of_shape<12>(pol, member, v); values_of_shape<13>(pol, member, v);
  int cnt = 0;
  for (int x : v) if (cnt < cap) out[cnt++] = x;
  return cnt;
}

}  // extern "C"
