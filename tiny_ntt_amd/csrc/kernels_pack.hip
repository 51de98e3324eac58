// kernels_pack.hip — one level of the LWE -> RLWE packing tree, or one trace step, from one launch: with t = X^rot * od,
// c = (ev + t) + EvalAuto(ev - t, g) (polydot_pack_kernel: fused plans), with its launcher.  A translation unit of its own,
// with its own dynamic-LDS symbol: a kernel that shares the family's symbol changes the register allocation of its
// neighbours.  The per-word code is pack_core.h's (and galois_core.h's, cmux_core.h's through it).
#include "fused_kernels.h"
#include "pack_core.h"

namespace tn {

// ============================================================================
// Pack step: s = ev + X^rot od, d = ev - X^rot od (od == NULL: s = d = ev), on both components;
//   c[row][o] = s[o] + [o == 0] sigma_g(d[0]) + sum_j digit_j(sigma_g(d[1])) * b[SHARED ? 0 : row][o][j], o < 2
// ============================================================================
// polydot_pack_kernel: polydot_galoisks_kernel's row (kernels_galoisks.hip, where the reasons for its form are given) with the
// inputs formed on the load.  terms + 2 transforms per output row, as there.
//   Loads.  ev[row][o] comes at unit stride (ld_operand).  The word of X^rot od[row][o] of register r of thread tau lies at
//     (jidx(0, tau, r) - rot) & (n - 1) of the same row and its sign is bit log2 n of the difference (ld_rotated,
//     monomial_index, monomial_negated: the CMux kernel's rotated load; rot is a kernel argument, one for the launch): lanes
//     stay consecutive, the access is coalesced but not aligned and wraps once per row.
//   Words.  d[1] is formed in registers at the top of the row (pack_rotated_word, pack_diff_word: canonical residues of what
//     tn_monomial_mul_dev and a subtraction mod q write), scattered under sigma_g (galois_dst, pack_scatter_word) and read
//     back, as the parent does: the subtraction comes BEFORE sigma_g and sigma_g BEFORE the digit cut.  d[0] takes the same
//     way behind inverse 0.  s[0] and s[1] are formed where they are added (pack_sum_word, pack_add_in): one conditional
//     subtraction for the sum, one for the add-in.
//   Where s[1] lives: nowhere.  The rotated od[row][1] is requested AGAIN inside inverse 1 (after_first, where the parent
//     requests the next row) and ev[row][1] again behind it, together with the next row's ev[.][1]; s[1] is formed from them and
//     added in.  Component 1 is stored behind that add-in, BEFORE the next row's rotated words are requested into the
//     registers the sum has left: the parent defers this store to the top of the next row, which here would keep a third row
//     alive beside the next row's two across the top of the loop.  The rotated od[row][0] is requested BEHIND inverse 0:
//     two sums and ev[row][0] are live inside it, the parent's count.  Inside either inverse the live rows are the parent's.
//   Trace step.  od == NULL is the TRACE instantiation (the launcher picks it): no rotated load; s = d = ev.  Its row is the
//     PARENT's, with two add-ins: ev[row][1] goes raw through the scatter (galois_scatter_word makes it canonical), the next
//     row's ev[.][1] rides inside inverse 1, component 1's store waits for the top of the next row; s[0] = ev[row][0] mod q
//     joins the first result before that row's scatter, and ev[row][1] is requested again behind inverse 1 and joins the
//     second (gadget_canon, pack_add_in).  A template flag, not a workgroup-uniform branch, and not the pack form on zeros:
//     both of those spilled at n = 2048 / 64-bit words / canonical policy, the shape whose parent sits at 128 VGPRs (the branch:
//     2 SGPRs and 4 VGPRs, 20 bytes of scratch per lane in the shared-key pack form; the pack form's row on zeros: 1 VGPR, 8
//     bytes, in the trace form with a key per row, wherever its loads were placed).  With the parent's row no instantiation
//     uses scratch.  The flag doubles the unit's instantiations, 50 to 100 (DESIGN.md 3.2m has the table and the build time).
// Hazards on the image (it is the transforms' transpose image; a permutation scatters to words that other threads read back):
//   (1) the image is free of the previous transform's readers before a scatter.  Both scatters stand behind an inverse (the
//       previous row's second, this row's first; the first row's behind the barrier that ends the staging of the twiddles);
//       between inverse and scatter there are only global loads, register arithmetic and global stores.  An inverse ends
//       with exchange 0, which crosses waves in a workgroup of more than one wave (asserted below) and so ends with
//       __syncthreads() behind its last read.  A workgroup of one wave executes its LDS operations in issue order.
//   (2) a scatter is complete before its read-back: the __syncthreads() between the two.
//   (3) a read-back is complete before the next transform's first exchange writes the image.  Behind the top-of-row load that
//       transform is a forward, whose first exchange is exchange 0 and begins with __syncthreads().  Behind the add-in it is
//       the second inverse, whose first exchange is the LAST one and in most shapes private to a wave: the __syncthreads()
//       behind the add-in's read-back, there only (READBACK_BARRIER below).
// No address depends on data: the image index depends on g and the rotated index on rot, both kernel arguments, and both are
// masked to the row, so no value that got past the argument check could address outside the image or the row.  c must not
// overlap ev, od or bhat (the kernel reads a row's inputs again after its first component is stored): check_pack_step.
template <typename E, int LOGN, int LPT, bool LAZY, bool BC, bool SHARED, int XL, bool TRACE>
__global__ void __launch_bounds__((1 << (LOGN - LPT)), (dot_waves<E, LOGN, LPT, LAZY>()))
polydot_pack_kernel(const Arith<E> ar, const typename TwOf<E>::type* __restrict__ tab_fwd, const typename TwOf<E>::type* __restrict__ tab_inv,
                    const E* __restrict__ ev, const E* __restrict__ od, u32 rot, u32 galois, const E* __restrict__ bhat, E* __restrict__ c, u32 batch,
                    u32 terms, u32 base_log, u32 balanced, u32* sched, u32 chunk) {
  typedef FusedCfg<E, LOGN, LPT> Cfg;
  typedef Policy<E, LAZY> Pol;
  typedef typename TwOf<E>::type Tw;
  static_assert(Cfg::PHASES >= 2, "the last phase's twiddles are requested during the phase before it");
  static_assert(Cfg::R <= 32, "one carry bit per word of the thread in a 32-bit mask");
  static_assert(XL >= 0 && XL <= Cfg::R, "words of d[1] per thread kept in LDS");
  static_assert(Cfg::jidx(0, 1, 0) == 1 && Cfg::jidx(0, 0, 1) == (u32)Cfg::THREADS, "phase 0: word r of thread tau is r * THREADS + tau");
  static_assert(Cfg::lds_elems() >= Cfg::N, "the transpose image holds a row");
  static_assert(Cfg::WB == 0 || !Cfg::ex_wave_local(0), "hazards (1) and (3): with more than one wave exchange 0 has workgroup barriers");
  // hazard (3) behind the add-in: the second inverse's first exchange has no workgroup barrier of its own
  constexpr bool READBACK_BARRIER = Cfg::WB > 0 && Cfg::ex_wave_local(Cfg::PHASES - 2);
  extern __shared__ __attribute__((aligned(16))) unsigned char tn_smem_pack[];
  const u32 tau = threadIdx.x;
  // LDS: [transpose image][XL * THREADS words of sigma_g(d[1])][staged twiddles, forward][... inverse][next-row slot]
  E* lds = reinterpret_cast<E*>(tn_smem_pack);
  E* lds_xw = lds + Cfg::lds_elems() + tau;                                   // word r of this thread at [r * THREADS]
  Tw* lds_fwd = reinterpret_cast<Tw*>(lds + Cfg::lds_elems() + XL * Cfg::THREADS);
  Tw* lds_inv = lds_fwd + Cfg::lds_tw_count();
  u32* lds_next = reinterpret_cast<u32*>(lds_inv + Cfg::lds_tw_count());      // output row this workgroup takes next
  for (u32 i = tau; i < (u32)Cfg::lds_tw_count(); i += Cfg::THREADS) {
    lds_fwd[i] = tab_fwd[Cfg::lds_tw_lo() + i];
    lds_inv[i] = tab_inv[Cfg::lds_tw_lo() + i];
  }
  __syncthreads();
  constexpr u32 EMASK = 2u * (u32)Cfg::N - 1u;
  constexpr bool has_od = !TRACE;
  rot &= EMASK;
  E acc0[Cfg::R], acc1[Cfg::R], xw[Cfg::R], xr[Cfg::R];  // the two sums, then their results; xw, xr: words of ev and rotated words of od
  u32 row = blockIdx.x * chunk;
  u32 taken = 1;                            // rows taken from the current chunk           (both workgroup-uniform: scalar registers)
  u32 chunk_id = blockIdx.x;                // fixed-stride mode: the chunk being processed
  // the rotated words of row `arow` of od ([batch * 2][n]) into x, thread index th; zeros in the trace step
  auto request_rotated = [&](E (&x)[Cfg::R], u32 arow, u32 th) {
    const u32 t0 = (th - rot) & EMASK;
#pragma unroll
    for (int r = 0; r < Cfg::R; ++r) x[r] = has_od ? ld_rotated<E, Cfg>(od, arow, t0 + (u32)r * Cfg::THREADS) : (E)0;
  };
  // register r's word of t = X^rot od, canonical, from the rotated word
  auto t_word = [&](E x, u32 th, int r) {
    return pack_rotated_word<E, Pol>(x, monomial_negated(((th - rot) & EMASK) + (u32)r * Cfg::THREADS, Cfg::LOGN), ar);
  };
  if (row < batch) {
#pragma unroll
    for (int r = 0; r < Cfg::R; ++r) xw[r] = ld_operand<E, Cfg>(ev, 2u * row + 1u, tau, r);
    request_rotated(xr, 2u * row + 1u, tau);
  }
  // x: the thread's phase-0 words of d -> its words of sigma_g(d), canonical, through the image.  Pack form: x is canonical
  // already (pack_diff_word).  Trace form: d = ev, any words, made canonical on the way (galois_scatter_word, as the parent does)
  auto permute = [&](E (&x)[Cfg::R], u32 th) {
#pragma unroll
    for (int r = 0; r < Cfg::R; ++r) {
      bool neg;
      const u32 d = galois_dst((u32)r * Cfg::THREADS + th, galois, (u32)Cfg::LOGN, neg);
      lds[d] = TRACE ? galois_scatter_word<E, Pol>(x[r], neg, ar) : pack_scatter_word<E>(x[r], neg, ar.q);
    }
    __syncthreads();                         // hazard (2)
#pragma unroll
    for (int r = 0; r < Cfg::R; ++r) x[r] = lds[(u32)r * Cfg::THREADS + th];
  };
  constexpr int PRE_END = Cfg::LOGN;        // no resident last-stage twiddles (polydot_prepared_kernel)
  Tw prf[Cfg::NPRE];
  constexpr bool KARG = TN_KARG_ARITH != 0;
  u32 prev = row;                           // trace form: the row whose second component waits for its store
  bool have_c = false;
  if constexpr (TRACE) {
#pragma unroll
    for (int r = 0; r < Cfg::R; ++r) acc1[r] = 0;
  }
  while (row < batch) {
    // one thread determines the next output row now; everyone reads the answer after the last term's transform
    const bool in_chunk = taken != chunk;
    taken = in_chunk ? taken + 1 : 1;
    chunk_id = in_chunk ? chunk_id : chunk_id + gridDim.x;
    if (tau == 0) *lds_next = in_chunk ? row + 1 : (sched ? gridDim.x + atomicAdd(&sched[0], 1u) : chunk_id) * chunk;
    // row of a per-set bhat of this output row's first term of component 0; component 1 follows `terms` rows later
    // (< 2^31: tn_poly_pack_step_prepared_dev)
    const u32 brow = row * 2u * terms;
    E xa[Cfg::R], xb[Cfg::R];                // the term in flight and the prepared row of the component being multiplied
    u32 tl = opaque_copy(tau);               // thread index for global addressing (see opaque_copy)
    // consume this row's words first (only their loads are in flight here: the wait is exact): d[1] = ev[1] - t[1], sigma_g of
    // it through the image (hazard (1): the previous row's second inverse ended with a barrier), XL of the result put away
    if constexpr (!TRACE) {
#pragma unroll
      for (int r = 0; r < Cfg::R; ++r) xw[r] = pack_diff_word<E, Pol>(xw[r], t_word(xr[r], tl, r), ar);
    }
    permute(xw, tl);
#pragma unroll
    for (int r = 0; r < XL; ++r) lds_xw[r * Cfg::THREADS] = xw[r];
    sched_fence();
    // trace form: the stores of the previous row's second component, as in the parent (the first iteration writes zeros to this
    // row's own slot, which the same thread overwrites one iteration later)
    if constexpr (TRACE) st_result<E, Cfg>(c, 2u * prev + 1u, tl, acc1);
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
      const u32 shift = j * base_log;        // < 64 (tn_poly_pack_step_prepared_dev)
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
    E ad[Cfg::R];                            // the words of ev[row][o], for d[0] and for the sums
    const TwRefs<E> twi0 = {tab_inv, lds_inv, pre, nullptr, opaque_zero()};
    inverse_all<E, Cfg, Pol, KARG, BC>(acc0, opaque_copy(tau), twi0, ar, lds, [&]() {
#pragma unroll
      for (int r = 0; r < Cfg::R; ++r) ad[r] = ld_operand<E, Cfg>(ev, 2u * row, tl, r);
    });
    // the rotated words of od[row][0], behind the inverse: inside it they are a fourth live row
    tl = opaque_copy(tau);
    request_rotated(xr, 2u * row, tl);
    sched_fence();
    // s[0] joins the first result; d[0] takes the way through the image (hazard (1): the inverse above ended with a barrier)
#pragma unroll
    for (int r = 0; r < Cfg::R; ++r) {
      if constexpr (TRACE) {                 // s[0] = ev[0] mod q; d[0] = ev[0] is made canonical in the scatter
        acc0[r] = pack_add_in<E>(acc0[r], gadget_canon<E, Pol>(ad[r], ar), ar.q);
      } else {
        const E t = t_word(xr[r], tl, r);
        acc0[r] = pack_add_in<E>(acc0[r], pack_sum_word<E, Pol>(ad[r], t, ar), ar.q);
        ad[r] = pack_diff_word<E, Pol>(ad[r], t, ar);
      }
    }
    permute(ad, tl);
    if constexpr (READBACK_BARRIER) __syncthreads();      // hazard (3)
#pragma unroll
    for (int r = 0; r < Cfg::R; ++r) acc0[r] = pack_add_in<E>(acc0[r], ad[r], ar.q);
    st_result<E, Cfg>(c, 2u * row, tl, acc0);      // the first result leaves its registers here
    sched_fence();
    // the second inverse's private twiddles, through a thread index of their own (polydot_gadget2_kernel)
    if constexpr (BC) tw_prefetch_stages<E, Cfg, Cfg::stage_begin(Cfg::PHASES - 1), Cfg::LOGN - 1>(pre1, tl, tab_inv);
    else tw_prefetch<E, Cfg>(pre1, tl, tab_inv);
    sched_fence();
    const TwRefs<E> twi1 = {tab_inv, lds_inv, pre1, nullptr, opaque_zero()};
    const u32 nrow = next < batch ? next : row;
    if constexpr (TRACE) {
      // Trace form, the parent's row end: the next output row's ev[.][1] rides inside the inverse (unconditional: after the
      // last row this row's words are read again and dropped); ev[row][1] again behind it, s[1] = ev[row][1] mod q added in;
      // the store waits for the top of the next row.
      inverse_all<E, Cfg, Pol, KARG, BC>(acc1, opaque_copy(tau), twi1, ar, lds, [&]() {
#pragma unroll
        for (int r = 0; r < Cfg::R; ++r) xw[r] = ld_operand<E, Cfg>(ev, 2u * nrow + 1u, tl, r);
      });
      tl = opaque_copy(tau);
#pragma unroll
      for (int r = 0; r < Cfg::R; ++r) ad[r] = ld_operand<E, Cfg>(ev, 2u * row + 1u, tl, r);
      sched_fence();
#pragma unroll
      for (int r = 0; r < Cfg::R; ++r) acc1[r] = pack_add_in<E>(acc1[r], gadget_canon<E, Pol>(ad[r], ar), ar.q);
      prev = row;
      have_c = true;
    } else {
      inverse_all<E, Cfg, Pol, KARG, BC>(acc1, opaque_copy(tau), twi1, ar, lds, [&]() {
        // the rotated od[row][1] AGAIN, for s[1], requested after the inverse's own vector loads have been consumed (inverse_all):
        // c must not overlap ev or od, so component 0's store above has not touched them.  One row beside the sum being
        // inverted, the parent's count
        request_rotated(xr, 2u * row + 1u, tl);
      });
      // behind the inverse: ev[row][1] again and, with it, the next output row's ev[.][1].  Unconditional: after the last row
      // this row's words are read again and dropped.
      tl = opaque_copy(tau);
#pragma unroll
      for (int r = 0; r < Cfg::R; ++r) ad[r] = ld_operand<E, Cfg>(ev, 2u * row + 1u, tl, r);
#pragma unroll
      for (int r = 0; r < Cfg::R; ++r) xw[r] = ld_operand<E, Cfg>(ev, 2u * nrow + 1u, tl, r);
      sched_fence();
#pragma unroll
      for (int r = 0; r < Cfg::R; ++r) acc1[r] = pack_add_in<E>(acc1[r], pack_sum_word<E, Pol>(ad[r], t_word(xr[r], tl, r), ar), ar.q);
      st_result<E, Cfg>(c, 2u * row + 1u, tl, acc1);
      sched_fence();
      // ... and the next output row's rotated od[.][1], behind the store, into the registers the sum has finished with
      request_rotated(xr, 2u * nrow + 1u, tl);
      sched_fence();
    }
    row = next;
  }
  if constexpr (TRACE) {
    if (have_c) st_result<E, Cfg>(c, 2u * prev + 1u, tau, acc1);
  }
  rearm_row_counters(sched, tau);
}

template <typename Sh>
static hipError_t launch_pack_t(const tn_plan* p, const void* ev, const void* od, u32 rot, u32 galois, const void* bhat, bool shared, void* c, size_t batch,
                                size_t terms, u32 base_log, bool balanced, hipStream_t s) {
  typedef typename Sh::E E;
  typedef typename Sh::Cfg Cfg;
  constexpr int LOGN = Sh::LOGN, LPT = Sh::LPT, XL = gadget2_lds_words<Sh>();
  constexpr bool LAZY = Sh::LAZY;
  const FusedProductLaunch<Sh> L(p);
  const u32 b32 = (u32)batch, t32 = (u32)terms, bal = balanced ? 1u : 0u;
  constexpr size_t lds_bytes = fused_lds_bytes<Sh>(2, (size_t)XL * Cfg::THREADS);
  // od == NULL picks the TRACE instantiation
  auto pick = [&](auto bc_) {
    constexpr bool BC = decltype(bc_)::value;
    return od ? (shared ? polydot_pack_kernel<E, LOGN, LPT, LAZY, BC, true, XL, false> : polydot_pack_kernel<E, LOGN, LPT, LAZY, BC, false, XL, false>)
              : (shared ? polydot_pack_kernel<E, LOGN, LPT, LAZY, BC, true, XL, true> : polydot_pack_kernel<E, LOGN, LPT, LAZY, BC, false, XL, true>);
  };
  auto kern = pick(std::false_type{});
  if constexpr (L.HAS_BC) {
    if (L.use_bc) kern = pick(std::true_type{});
  }
  // Rows are planned as the automorphism key switch's (dot_row_bytes, `terms` operand rows): an output row is `terms` forward
  // transforms and two inverses between two atomics.
  return launch_persistent(p, s, reinterpret_cast<const void*>(kern), Cfg::THREADS, lds_bytes, dot_row_bytes(Cfg::N * sizeof(E), terms), batch, FUSED_ROWS,
                           [&](u32 grid, u32* sched, u32 chunk) {
    hipLaunchKernelGGL(kern, dim3(grid), dim3(Cfg::THREADS), lds_bytes, s, L.su.ar, L.fwd(), L.inv(),
                       (const E*)ev, (const E*)od, rot, galois, (const E*)bhat, (E*)c, b32, t32, base_log, bal, sched, chunk);
    return hipGetLastError();
  });
}

// rot below 2n, galois odd and below 2n (check_pack_step); the kernel masks both indices to the row whatever they are.
// od == NULL: the trace step.
hipError_t launch_polydot_pack(const tn_plan* p, const void* ev, const void* od, uint32_t rot, uint32_t galois, const void* bhat, bool shared, void* c,
                               size_t batch, size_t terms, u32 base_log, bool balanced, hipStream_t s) {
  if (batch == 0) return hipSuccess;
  return dispatch_fused_shape(p, [&](auto sh) { return launch_pack_t<decltype(sh)>(p, ev, od, rot, galois, bhat, shared, c, batch, terms, base_log, balanced, s); });
}

}  // namespace tn
