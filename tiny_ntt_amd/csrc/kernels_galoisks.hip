// kernels_galoisks.hip — the homomorphic automorphism of an RLWE ciphertext from one launch: sigma_g on both components, the key
// switch of the second, the first added in (polydot_galoisks_kernel: fused plans), with its launcher.  A translation unit of
// its own, with its own dynamic-LDS symbol: a kernel that shares the family's symbol changes the register allocation of its
// neighbours.  The per-word code is galois_core.h's.
#include "fused_kernels.h"
#include "galois_core.h"

namespace tn {

// ============================================================================
// Automorphism key switch: c[row][o] = [o == 0] sigma_g(a[row][0]) + sum_j digit_j(sigma_g(a[row][1])) * b[SHARED ? 0 : row][o][j], o < 2
// ============================================================================
// polydot_galoisks_kernel: polydot_gadget2_kernel's row (kernels_gadget.hip, where the reasons for its form are given) with two
// changes.  terms + 2 transforms per output row, as there.
//   Permuted load.  The words of a[row][1] come from global memory at unit stride, requested inside the previous row's second
//     inverse (ld_operand, as the gadget kernel requests its row).  At the top of the row they are made canonical and carried
//     through the transpose image: the holder of source word s = r * THREADS + tau (phase 0) writes +-x at (s g) & (n - 1), the
//     sign is bit log2 n of s g mod 2n and a zero stays 0 (galois_dst, galois_scatter_word); one barrier; every thread reads
//     its own phase-0 words r * THREADS + tau back at unit stride.  These are the canonical words of sigma_g(a[row][1]), which
//     is what tn_automorphism_dev writes, so the digits cut from them are the explicit route's: sigma_g comes BEFORE the cut.
//     Lanes are g words apart on the write and one word apart on the read; g is odd, so neither side has a bank conflict at
//     either lane width.  A strided gather from global memory would touch 64 cache lines per wave instruction.
//   Add-in.  a[row][0] is requested at unit stride inside inverse 0 (after_first: behind the inverse's own vector loads, where
//     the CMux kernel requests its add-in words), carried through the image the same way behind that inverse and added to its
//     output with one conditional subtraction (galois_add_in) before the result is stored.
// Hazards on the image (it is the transforms' transpose image; a permutation scatters to words that other threads read back):
//   (1) the image is free of the previous transform's readers before a scatter.  Both scatters stand behind an inverse (the
//       previous row's second, this row's first; the first row's behind the barrier that ends the staging of the twiddles).  An
//       inverse ends with exchange 0, which crosses waves in a workgroup of more than one wave (FusedCfg::ex_wave_local(0) is
//       false when WB > 0, asserted below) and so ends with __syncthreads() behind its last read (exchange, fused_kernels.h).
//       A workgroup of one wave executes its LDS operations in issue order.
//   (2) a scatter is complete before its read-back: the __syncthreads() between the two.
//   (3) a read-back is complete before the next transform's first exchange writes the image.  Behind the load that transform is
//       a forward, whose first exchange is exchange 0 and begins with __syncthreads() (as under (1)).  Behind the add-in it is
//       the second inverse, whose first exchange is the LAST one and in most shapes private to a wave, without a workgroup
//       barrier: the __syncthreads() behind the add-in's read-back, there only (READBACK_BARRIER below).
// No address depends on data: the image index depends on g, a kernel argument, and is masked to the row, so no value of g
// that got past the argument check could address outside the image.  a and c must not overlap (the kernel permutes within a
// row and prefetches the next one): check_galois_keyswitch.
template <typename E, int LOGN, int LPT, bool LAZY, bool BC, bool SHARED, int XL>
__global__ void __launch_bounds__((1 << (LOGN - LPT)), (dot_waves<E, LOGN, LPT, LAZY>()))
polydot_galoisks_kernel(const Arith<E> ar, const typename TwOf<E>::type* __restrict__ tab_fwd, const typename TwOf<E>::type* __restrict__ tab_inv,
                        const E* __restrict__ a, u32 galois, const E* __restrict__ bhat, E* __restrict__ c, u32 batch, u32 terms, u32 base_log,
                        u32 balanced, u32* sched, u32 chunk) {
  typedef FusedCfg<E, LOGN, LPT> Cfg;
  typedef Policy<E, LAZY> Pol;
  typedef typename TwOf<E>::type Tw;
  static_assert(Cfg::PHASES >= 2, "the last phase's twiddles are requested during the phase before it");
  static_assert(Cfg::R <= 32, "one carry bit per word of the thread in a 32-bit mask");
  static_assert(XL >= 0 && XL <= Cfg::R, "words of a per thread kept in LDS");
  static_assert(Cfg::jidx(0, 1, 0) == 1 && Cfg::jidx(0, 0, 1) == (u32)Cfg::THREADS, "phase 0: word r of thread tau is r * THREADS + tau");
  static_assert(Cfg::lds_elems() >= Cfg::N, "the transpose image holds a row");
  static_assert(Cfg::WB == 0 || !Cfg::ex_wave_local(0), "hazards (1) and (3): with more than one wave exchange 0 has workgroup barriers");
  // hazard (3) behind the add-in: the second inverse's first exchange has no workgroup barrier of its own
  constexpr bool READBACK_BARRIER = Cfg::WB > 0 && Cfg::ex_wave_local(Cfg::PHASES - 2);
  extern __shared__ __attribute__((aligned(16))) unsigned char tn_smem_galoisks[];
  const u32 tau = threadIdx.x;
  // LDS: [transpose image][XL * THREADS words of a][staged twiddles, forward][... inverse][next-row slot]
  E* lds = reinterpret_cast<E*>(tn_smem_galoisks);
  E* lds_xw = lds + Cfg::lds_elems() + tau;                                   // word r of this thread at [r * THREADS]
  Tw* lds_fwd = reinterpret_cast<Tw*>(lds + Cfg::lds_elems() + XL * Cfg::THREADS);
  Tw* lds_inv = lds_fwd + Cfg::lds_tw_count();
  u32* lds_next = reinterpret_cast<u32*>(lds_inv + Cfg::lds_tw_count());      // output row this workgroup takes next
  for (u32 i = tau; i < (u32)Cfg::lds_tw_count(); i += Cfg::THREADS) {
    lds_fwd[i] = tab_fwd[Cfg::lds_tw_lo() + i];
    lds_inv[i] = tab_inv[Cfg::lds_tw_lo() + i];
  }
  __syncthreads();
  E acc0[Cfg::R], acc1[Cfg::R], xw[Cfg::R];  // the sums of the two components, then their results; xw: the words of a[row][1]
  u32 row = blockIdx.x * chunk;
  u32 taken = 1;                            // rows taken from the current chunk           (both workgroup-uniform: scalar registers)
  u32 chunk_id = blockIdx.x;                // fixed-stride mode: the chunk being processed
  if (row < batch) {
#pragma unroll
    for (int r = 0; r < Cfg::R; ++r) xw[r] = ld_operand<E, Cfg>(a, 2u * row + 1u, tau, r);
  }
  // x: the thread's phase-0 words of a row of a, any word values -> its words of sigma_g of that row, canonical, through the image
  auto permute = [&](E (&x)[Cfg::R], u32 th) {
#pragma unroll
    for (int r = 0; r < Cfg::R; ++r) {
      bool neg;
      const u32 d = galois_dst((u32)r * Cfg::THREADS + th, galois, (u32)Cfg::LOGN, neg);
      lds[d] = galois_scatter_word<E, Pol>(x[r], neg, ar);
    }
    __syncthreads();                         // hazard (2)
#pragma unroll
    for (int r = 0; r < Cfg::R; ++r) x[r] = lds[(u32)r * Cfg::THREADS + th];
  };
  constexpr int PRE_END = Cfg::LOGN;        // no resident last-stage twiddles (polydot_prepared_kernel)
  Tw prf[Cfg::NPRE];
  constexpr bool KARG = TN_KARG_ARITH != 0;
  u32 prev = row;
  bool have_c = false;
#pragma unroll
  for (int r = 0; r < Cfg::R; ++r) acc1[r] = 0;
  while (row < batch) {
    // one thread determines the next output row now; everyone reads the answer after the last term's transform
    const bool in_chunk = taken != chunk;
    taken = in_chunk ? taken + 1 : 1;
    chunk_id = in_chunk ? chunk_id : chunk_id + gridDim.x;
    if (tau == 0) *lds_next = in_chunk ? row + 1 : (sched ? gridDim.x + atomicAdd(&sched[0], 1u) : chunk_id) * chunk;
    // row of a per-set bhat of this output row's first term of component 0; component 1 follows `terms` rows later
    // (< 2^31: tn_poly_galois_keyswitch_prepared_dev)
    const u32 brow = row * 2u * terms;
    E xa[Cfg::R], xb[Cfg::R];                // the term in flight and the prepared row of the component being multiplied
    u32 tl = opaque_copy(tau);               // thread index for global addressing (see opaque_copy)
    // consume this row's words first (only their loads are in flight here: the wait is exact): sigma_g of them through the image,
    // XL of the result put away; then issue the stores of the previous row's second component (the first iteration writes zeros
    // to this row's own slot, which the same thread overwrites one iteration later)
    permute(xw, tl);
#pragma unroll
    for (int r = 0; r < XL; ++r) lds_xw[r * Cfg::THREADS] = xw[r];
    sched_fence();
    st_result<E, Cfg>(c, 2u * prev + 1u, tl, acc1);
#pragma unroll
    for (int r = 0; r < Cfg::R; ++r) { acc0[r] = 0; acc1[r] = 0; }
    u32 carries = 0;                         // bit r: the carry of word r into its next digit (balanced mode)
    // register r of the prepared row of component o, term j
    auto request1 = [&](u32 o, u32 j, u32 t, int r) {
      xb[r] = SHARED ? ld_prepared<E, Cfg, false>(bhat, o * terms + j, t, r) : ld_prepared<E, Cfg, true>(bhat, brow + o * terms + j, t, r);
    };
    const Tw* zeta = prf + Cfg::pre_off(Cfg::LOGN - 1);      // (the base case's zeta records came with prf)
    u32 next = 0;
    // a counted loop with ONE copy of the two products (polydot_gadget2_kernel)
    for (u32 j = 0; j < terms; ++j) {
      tl = opaque_copy(tau);
      // component 0's prepared row, before the forward's first phase
#pragma unroll
      for (int r = 0; r < Cfg::R; ++r) request1(0u, j, tl, r);
      sched_fence();
      const u32 shift = j * base_log;        // < 64 (tn_poly_galois_keyswitch_prepared_dev)
      u32 next_carries = 0;
#pragma unroll
      for (int r = 0; r < Cfg::R; ++r) {
        u32 cy = (carries >> r) & 1u;
        const E w = r < XL ? (lds + Cfg::lds_elems())[r * Cfg::THREADS + tl] : xw[r];
        xa[r] = gadget_digit<E>(w, shift, base_log, balanced != 0, cy, ar.q);
        next_carries |= cy << r;
      }
      carries = next_carries;
      const TwRefs<E> twf = {tab_fwd, lds_fwd, prf, nullptr, opaque_zero()};
      forward_range<E, Cfg, Pol, 0, Cfg::PHASES, KARG, PRE_END, BC>(xa, tau, twf, ar, lds, true, tl);      // hazard (3): exchange 0 begins with a barrier
      if (j + 1 == terms) {                  // everyone reads the next output row behind the last term's transform, as in the gadget kernel
        __syncthreads();
        next = wave_uniform(*lds_next);
      }
      // component 0's product, the transformed digit row left as it is; component 1's prepared row goes pair by pair into the
      // registers that product has finished with (a thread index of its own: polydot_gadget2_kernel)
      dot_product_into<E, Cfg, Pol, BC>(acc0, xa, xb, zeta, ar, [&](auto i_) {
        constexpr int r = 2 * decltype(i_)::value;
        const u32 t = opaque_copy(tau);
        request1(1u, j, t, r);
        request1(1u, j, t, r + 1);
        sched_fence();
      });
      if constexpr (BC) basecase<Cfg, Pol>(xa, xb, zeta, ar);      // component 1's product may overwrite the digit row
      else pointwise<E, Cfg, Pol>(xa, xb, ar);
      dot_accumulate<E, Cfg, Pol>(acc1, xa, ar);
      sched_fence();
    }
    // the private twiddles the first inverse starts with (behind the loop: requested inside it they are live across it)
    Tw pre[Cfg::NPRE], pre1[Cfg::NPRE];
    if constexpr (BC) tw_prefetch_stages<E, Cfg, Cfg::stage_begin(Cfg::PHASES - 1), Cfg::LOGN - 1>(pre, tl, tab_inv);
    else tw_prefetch<E, Cfg>(pre, tl, tab_inv);
    sched_fence();
    E ad[Cfg::R];                            // the words of a[row][0], for the add-in behind inverse 0
    const TwRefs<E> twi0 = {tab_inv, lds_inv, pre, nullptr, opaque_zero()};
    inverse_all<E, Cfg, Pol, KARG, BC>(acc0, opaque_copy(tau), twi0, ar, lds, [&]() {
#pragma unroll
      for (int r = 0; r < Cfg::R; ++r) ad[r] = ld_operand<E, Cfg>(a, 2u * row, tl, r);
    });
    // sigma_g(a[row][0]) through the image (hazard (1): the inverse above ended with a barrier), added to the first result,
    // which leaves its registers here
    tl = opaque_copy(tau);
    permute(ad, tl);
    if constexpr (READBACK_BARRIER) __syncthreads();      // hazard (3)
#pragma unroll
    for (int r = 0; r < Cfg::R; ++r) acc0[r] = galois_add_in<E>(acc0[r], ad[r], ar.q);
    st_result<E, Cfg>(c, 2u * row, tl, acc0);
    sched_fence();
    // the second inverse's private twiddles, through a thread index of their own (polydot_gadget2_kernel)
    if constexpr (BC) tw_prefetch_stages<E, Cfg, Cfg::stage_begin(Cfg::PHASES - 1), Cfg::LOGN - 1>(pre1, tl, tab_inv);
    else tw_prefetch<E, Cfg>(pre1, tl, tab_inv);
    sched_fence();
    const TwRefs<E> twi1 = {tab_inv, lds_inv, pre1, nullptr, opaque_zero()};
    inverse_all<E, Cfg, Pol, KARG, BC>(acc1, opaque_copy(tau), twi1, ar, lds, [&]() {
      // the words of a[.][1] of the next output row, requested after the inverse's own vector loads have been consumed
      // (inverse_all); this row's last digits have been taken.  Unconditional: after the last row this row's words are read
      // again and dropped.
      const u32 nrow = next < batch ? next : row;
#pragma unroll
      for (int r = 0; r < Cfg::R; ++r) xw[r] = ld_operand<E, Cfg>(a, 2u * nrow + 1u, tl, r);
    });
    prev = row;
    have_c = true;
    row = next;
  }
  if (have_c) st_result<E, Cfg>(c, 2u * prev + 1u, tau, acc1);
  rearm_row_counters(sched, tau);
}

template <typename Sh>
static hipError_t launch_galoisks_t(const tn_plan* p, const void* a, u32 galois, const void* bhat, bool shared, void* c, size_t batch, size_t terms,
                                    u32 base_log, bool balanced, hipStream_t s) {
  typedef typename Sh::E E;
  typedef typename Sh::Cfg Cfg;
  constexpr int LOGN = Sh::LOGN, LPT = Sh::LPT, XL = gadget2_lds_words<Sh>();
  constexpr bool LAZY = Sh::LAZY;
  const FusedProductLaunch<Sh> L(p);
  const u32 b32 = (u32)batch, t32 = (u32)terms, bal = balanced ? 1u : 0u;
  constexpr size_t lds_bytes = fused_lds_bytes<Sh>(2, (size_t)XL * Cfg::THREADS);
  auto kern = shared ? polydot_galoisks_kernel<E, LOGN, LPT, LAZY, false, true, XL> : polydot_galoisks_kernel<E, LOGN, LPT, LAZY, false, false, XL>;
  if constexpr (L.HAS_BC) {
    if (L.use_bc) kern = shared ? polydot_galoisks_kernel<E, LOGN, LPT, LAZY, true, true, XL> : polydot_galoisks_kernel<E, LOGN, LPT, LAZY, true, false, XL>;
  }
  // Rows are planned as the two-component gadget kernel's (dot_row_bytes, `terms` operand rows): an output row is `terms`
  // forward transforms and two inverses between two atomics.
  return launch_persistent(p, s, reinterpret_cast<const void*>(kern), Cfg::THREADS, lds_bytes, dot_row_bytes(Cfg::N * sizeof(E), terms), batch, FUSED_ROWS,
                           [&](u32 grid, u32* sched, u32 chunk) {
    hipLaunchKernelGGL(kern, dim3(grid), dim3(Cfg::THREADS), lds_bytes, s, L.su.ar, L.fwd(), L.inv(),
                       (const E*)a, galois, (const E*)bhat, (E*)c, b32, t32, base_log, bal, sched, chunk);
    return hipGetLastError();
  });
}

// galois: odd and below 2n (check_galois_keyswitch); the kernel masks the index to the row whatever it is
hipError_t launch_polydot_galoisks(const tn_plan* p, const void* a, uint32_t galois, const void* bhat, bool shared, void* c, size_t batch, size_t terms,
                                   u32 base_log, bool balanced, hipStream_t s) {
  if (batch == 0) return hipSuccess;
  return dispatch_fused_shape(p, [&](auto sh) { return launch_galoisks_t<decltype(sh)>(p, a, galois, bhat, shared, c, batch, terms, base_log, balanced, s); });
}

}  // namespace tn
