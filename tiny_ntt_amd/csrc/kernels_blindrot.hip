// kernels_blindrot.hip — a blind rotation from one launch: `steps` CMux rotation steps per row with the accumulator kept in LDS
// across them (polydot_blindrot_kernel: fused plans whose request fits a workgroup's LDS, launch_plan.h: blindrot_supported),
// with its launcher.  A translation unit of its own, with its own dynamic-LDS symbol: a kernel that shares the family's
// symbol changes the register allocation of its neighbours.  The per-word code is cmux_core.h's.
#include "fused_kernels.h"
#include "cmux_core.h"

namespace tn {

// ============================================================================
// Blind rotation: acc = a[row]; for k < steps: acc[o] = acc[o] + sum_{i < 2} sum_{j < terms} digit_j((X^e_k - 1) * acc[i]) * b[k][o][i][j]; c[row] = acc
// ============================================================================
// polydot_blindrot_kernel: polydot_cmux_kernel's row (kernels_cmux.hip, where the reasons for its form are given) with a loop
// over steps around it and the accumulator acc_0, acc_1 in LDS, word t of a component at [t].  A row's blind rotation depends on
// no other row, so the workgroup that takes a row keeps it for all steps: a is read once, c written once, and the only global
// traffic of a step is its key (shared by every row: L2) and one scalar load of the exponent.
//   Load.  The first row's words go from global memory into the accumulator before the loop; a later row's ride inside the two
//     inverses of the LAST step of the row before it (after_first: behind the inverse's own vector loads, where the CMux
//     kernel requests its add-in words; with 64-bit words behind the inverse, NEXT_IN_INVERSE below) and are written into the
//     accumulator where a step writes its result back.  Raw words: cmux_word and cmux_add_in canonicalise.
//   Step.  e = exps[k * batch + row] & (2n - 1), workgroup-uniform (wave_uniform: a scalar load; the next step's is requested
//     behind this step's last rotated read).  An input polynomial's words are cmux_word(acc_i[t], acc_i[(t - e) & (n - 1)],
//     sign) from LDS: thread tau's word r is t = r * THREADS + tau (phase 0), lanes stay consecutive on both reads.  Then the
//     CMux row: digits, one forward transform per term, both products against key k (prepared rows k * 4 * terms + o * 2 * terms
//     + t, shared loads, requested where the CMux kernel requests them: the next row of the key always flies behind a
//     transform), two inverses, cmux_add_in with the own words from LDS, and the result written back over them.
//   Store.  In the last step the result goes to c from the registers instead.
// Hazards on the accumulator (thread tau writes only the words it owns, [r * THREADS + tau]; it reads those and, rotated, words of
// other threads):
//   (1) the write-back of step k comes after every thread's last rotated read of step k.  Those reads (put_away of input i) are
//       followed, for every thread, by the forward transform of that input's first term and by the inverse of the component
//       written back; in a workgroup of more than one wave exchange 0 of every transform crosses waves (thread-id bit 6 is a
//       coefficient-index bit below the register bits in phase 0: FusedCfg::ex_wave_local(0) is false when WB > 0, asserted
//       below) and so begins with __syncthreads().  A workgroup of one wave executes its LDS operations in issue order.
//   (2) the rotated reads of step k + 1, and of the next row's step 0, come after every thread's write-back of both components
//       (or its write of the next row's words): the __syncthreads() at the top of every step.  It also orders the first row's
//       load before its first rotated read, and thread 0's publication of the next row before everyone's read of it.
// The words put away (XL per thread, at lds_xw) are private to their thread.  c == a is allowed: a row is read by the
// workgroup that owns it before that workgroup writes it, and the prefetched row is another row; a and c are therefore NOT
// declared __restrict__.  No address depends on data except through the masked exponent.
template <typename E, int LOGN, int LPT, bool LAZY, bool BC, int XL>
__global__ void __launch_bounds__((1 << (LOGN - LPT)), (dot_waves<E, LOGN, LPT, LAZY>()))
polydot_blindrot_kernel(const Arith<E> ar, const typename TwOf<E>::type* __restrict__ tab_fwd, const typename TwOf<E>::type* __restrict__ tab_inv,
                        const E* a, const u32* __restrict__ exps, const E* __restrict__ bhat, E* c, u32 batch, u32 steps, u32 terms,
                        u32 base_log, u32 balanced, u32* sched, u32 chunk) {
  typedef FusedCfg<E, LOGN, LPT> Cfg;
  typedef Policy<E, LAZY> Pol;
  typedef typename TwOf<E>::type Tw;
  static_assert(Cfg::PHASES >= 2, "the last phase's twiddles are requested during the phase before it");
  static_assert(Cfg::R <= 32, "one carry bit per word of the thread in a 32-bit mask");
  static_assert(XL >= 0 && XL <= Cfg::R, "words of an input per thread kept in LDS");
  static_assert(Cfg::jidx(0, 1, 0) == 1 && Cfg::jidx(0, 0, 1) == (u32)Cfg::THREADS, "phase 0: word r of thread tau is r * THREADS + tau");
  // 32-bit words: the next row's words are requested inside the last step's inverses.  64-bit words: behind them, where the
  // result has left its registers; inside, they are a third row of live words and every 64-bit shape from n = 512 on used
  // scratch (12 - 80 bytes per lane).  The wait is paid once per row, not per step.
  constexpr bool NEXT_IN_INVERSE = sizeof(E) == 4;
  static_assert(Cfg::WB == 0 || !Cfg::ex_wave_local(0), "hazard (1): with more than one wave every transform has a workgroup barrier");
  extern __shared__ __attribute__((aligned(16))) unsigned char tn_smem_blindrot[];
  const u32 tau = threadIdx.x;
  // LDS: [transpose image][XL * THREADS words of an input][acc_0][acc_1][staged twiddles, forward][... inverse][next-row slot]
  E* lds = reinterpret_cast<E*>(tn_smem_blindrot);
  E* lds_xw = lds + Cfg::lds_elems() + tau;                                   // word r of this thread at [r * THREADS]
  E* lds_acc = lds + Cfg::lds_elems() + XL * Cfg::THREADS;                    // component o at [o * N]
  Tw* lds_fwd = reinterpret_cast<Tw*>(lds_acc + 2 * Cfg::N);
  Tw* lds_inv = lds_fwd + Cfg::lds_tw_count();
  u32* lds_next = reinterpret_cast<u32*>(lds_inv + Cfg::lds_tw_count());      // output row this workgroup takes next
  for (u32 i = tau; i < (u32)Cfg::lds_tw_count(); i += Cfg::THREADS) {
    lds_fwd[i] = tab_fwd[Cfg::lds_tw_lo() + i];
    lds_inv[i] = tab_inv[Cfg::lds_tw_lo() + i];
  }
  constexpr u32 EMASK = 2u * (u32)Cfg::N - 1u, NMASK = (u32)Cfg::N - 1u;
  E acc0[Cfg::R], acc1[Cfg::R], xw[Cfg::R];    // the two sums, then their results; xw: an input polynomial's words
  u32 row = blockIdx.x * chunk;
  u32 taken = 1;                            // rows taken from the current chunk           (both workgroup-uniform: scalar registers)
  u32 chunk_id = blockIdx.x;                // fixed-stride mode: the chunk being processed
  if (row < batch) {
#pragma unroll
    for (int o = 0; o < 2; ++o) {
#pragma unroll
      for (int r = 0; r < Cfg::R; ++r) xw[r] = ld_operand<E, Cfg>(a, 2u * row + (u32)o, tau, r);
#pragma unroll
      for (int r = 0; r < Cfg::R; ++r) lds_acc[o * Cfg::N + r * Cfg::THREADS + tau] = xw[r];
    }
  }
  constexpr int PRE_END = Cfg::LOGN;        // no resident last-stage twiddles (polydot_prepared_kernel)
  Tw prf[Cfg::NPRE];
  constexpr bool KARG = TN_KARG_ARITH != 0;
  const u32 comp = 2u * terms;              // prepared rows of one component of a key
  while (row < batch) {
    // one thread determines the next output row now; everyone reads the answer behind the first step's barrier
    const bool in_chunk = taken != chunk;
    taken = in_chunk ? taken + 1 : 1;
    chunk_id = in_chunk ? chunk_id : chunk_id + gridDim.x;
    if (tau == 0) *lds_next = in_chunk ? row + 1 : (sched ? gridDim.x + atomicAdd(&sched[0], 1u) : chunk_id) * chunk;
    u32 next = 0;
    u32 e = wave_uniform(exps[row]) & EMASK;             // step 0's exponent (k * batch + row < 2^31: tn_poly_blind_rotate_prepared_dev)
    for (u32 k = 0; k < steps; ++k) {
      __syncthreads();                       // hazard (2): the accumulator is whole before anyone reads it rotated
      if (k == 0) next = wave_uniform(*lds_next);
      const bool last = k + 1 == steps;
      // first prepared row of this step's key, component 0; component 1 follows 2 * terms rows later (< 2^31: the row limit)
      const u32 brow = k * 2u * comp;
      E xa[Cfg::R], xb[Cfg::R];              // the term in flight and the prepared row of the component being multiplied
      u32 tl = opaque_copy(tau);             // thread index for global addressing (see opaque_copy)
      auto request1 = [&](u32 o, u32 t, u32 th, int r) { xb[r] = ld_prepared<E, Cfg, false>(bhat, brow + o * comp + t, th, r); };
      const Tw* zeta = prf + Cfg::pre_off(Cfg::LOGN - 1);      // (the base case's zeta records came with prf)
      u32 t = 0;                             // the term of the component's sum: i * terms + j
      // an input's words: (X^e - 1) * acc_i as canonical residues, once, XL of them put away
      auto put_away = [&](u32 i, u32 th) {
        const E* src = lds_acc + i * (u32)Cfg::N;
        const u32 t0 = (th - e) & EMASK;
#pragma unroll
        for (int r = 0; r < Cfg::R; ++r) {
          const u32 v = t0 + (u32)r * Cfg::THREADS;
          xw[r] = cmux_word<E, Pol>(src[(u32)r * Cfg::THREADS + th], src[v & NMASK], monomial_negated(v, Cfg::LOGN), ar);
          if (r < XL) lds_xw[r * Cfg::THREADS] = xw[r];
        }
        sched_fence();
      };
      put_away(0u, tl);
#pragma unroll
      for (int r = 0; r < Cfg::R; ++r) { acc0[r] = 0; acc1[r] = 0; }
      for (u32 i = 0;;) {
        u32 carries = 0;                     // bit r: the carry of word r into its next digit (balanced mode); per input polynomial
        for (u32 j = 0; j < terms; ++j, ++t) {
          tl = opaque_copy(tau);
          // component 0's prepared row, before the forward's first phase
#pragma unroll
          for (int r = 0; r < Cfg::R; ++r) request1(0u, t, tl, r);
          sched_fence();
          const u32 shift = j * base_log;    // < 64 (the gadget list)
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
          forward_range<E, Cfg, Pol, 0, Cfg::PHASES, KARG, PRE_END, BC>(xa, tau, twf, ar, lds, true, tl);
          // component 0's product, the transformed digit row left as it is; component 1's prepared row goes pair by pair into
          // the registers that product has finished with (a thread index of its own: polydot_gadget2_kernel)
          dot_product_into<E, Cfg, Pol, BC>(acc0, xa, xb, zeta, ar, [&](auto i_) {
            constexpr int r = 2 * decltype(i_)::value;
            const u32 th = opaque_copy(tau);
            request1(1u, t, th, r);
            request1(1u, t, th, r + 1);
            sched_fence();
          });
          if constexpr (BC) basecase<Cfg, Pol>(xa, xb, zeta, ar);      // component 1's product may overwrite the digit row
          else pointwise<E, Cfg, Pol>(xa, xb, ar);
          dot_accumulate<E, Cfg, Pol>(acc1, xa, ar);
          sched_fence();
        }
        if (++i == 2u) break;
        // the words of the second input polynomial, from the accumulator (no write-back of this step has happened yet)
        tl = opaque_copy(tau);
        put_away(1u, tl);
      }
      // the next step's exponent, behind this step's last rotated read (after the last step: step 0's again, dropped)
      const u32 e_next = wave_uniform(exps[(last ? 0u : (k + 1u) * batch) + row]) & EMASK;
      // the private twiddles the first inverse starts with (behind the loops: requested inside them they are live across them)
      Tw pre[Cfg::NPRE], pre1[Cfg::NPRE];
      if constexpr (BC) tw_prefetch_stages<E, Cfg, Cfg::stage_begin(Cfg::PHASES - 1), Cfg::LOGN - 1>(pre, tl, tab_inv);
      else tw_prefetch<E, Cfg>(pre, tl, tab_inv);
      sched_fence();
      const u32 nrow = next < batch ? next : row;      // after the last row this row's words are read again and dropped
      E nx[Cfg::R];                          // last step: the words of a[nrow][o], requested inside inverse o or behind it
      const TwRefs<E> twi0 = {tab_inv, lds_inv, pre, nullptr, opaque_zero()};
      inverse_all<E, Cfg, Pol, KARG, BC>(acc0, opaque_copy(tau), twi0, ar, lds, [&]() {
        if (NEXT_IN_INVERSE && last) {
#pragma unroll
          for (int r = 0; r < Cfg::R; ++r) nx[r] = ld_operand<E, Cfg>(a, 2u * nrow, tl, r);
        }
      });
      // add-in with the own words from the accumulator; the result back over them, or, in the last step, to c and the next row's
      // words into the accumulator.  Hazard (1): every rotated read of this step lies before the barriers of the inverse above.
      tl = opaque_copy(tau);
#pragma unroll
      for (int r = 0; r < Cfg::R; ++r) acc0[r] = cmux_add_in<E, Pol>(acc0[r], lds_acc[r * Cfg::THREADS + tl], ar);
      if (last) {
        st_result<E, Cfg>(c, 2u * row, tl, acc0);
        if constexpr (!NEXT_IN_INVERSE) {
#pragma unroll
          for (int r = 0; r < Cfg::R; ++r) nx[r] = ld_operand<E, Cfg>(a, 2u * nrow, tl, r);
        }
#pragma unroll
        for (int r = 0; r < Cfg::R; ++r) lds_acc[r * Cfg::THREADS + tl] = nx[r];
      } else {
#pragma unroll
        for (int r = 0; r < Cfg::R; ++r) lds_acc[r * Cfg::THREADS + tl] = acc0[r];
      }
      sched_fence();
      if constexpr (BC) tw_prefetch_stages<E, Cfg, Cfg::stage_begin(Cfg::PHASES - 1), Cfg::LOGN - 1>(pre1, tl, tab_inv);
      else tw_prefetch<E, Cfg>(pre1, tl, tab_inv);
      sched_fence();
      const TwRefs<E> twi1 = {tab_inv, lds_inv, pre1, nullptr, opaque_zero()};
      inverse_all<E, Cfg, Pol, KARG, BC>(acc1, opaque_copy(tau), twi1, ar, lds, [&]() {
        if (NEXT_IN_INVERSE && last) {
#pragma unroll
          for (int r = 0; r < Cfg::R; ++r) nx[r] = ld_operand<E, Cfg>(a, 2u * nrow + 1u, tl, r);
        }
      });
      tl = opaque_copy(tau);
#pragma unroll
      for (int r = 0; r < Cfg::R; ++r) acc1[r] = cmux_add_in<E, Pol>(acc1[r], lds_acc[Cfg::N + r * Cfg::THREADS + tl], ar);
      if (last) {
        st_result<E, Cfg>(c, 2u * row + 1u, tl, acc1);
        if constexpr (!NEXT_IN_INVERSE) {
#pragma unroll
          for (int r = 0; r < Cfg::R; ++r) nx[r] = ld_operand<E, Cfg>(a, 2u * nrow + 1u, tl, r);
        }
#pragma unroll
        for (int r = 0; r < Cfg::R; ++r) lds_acc[Cfg::N + r * Cfg::THREADS + tl] = nx[r];
      } else {
#pragma unroll
        for (int r = 0; r < Cfg::R; ++r) lds_acc[Cfg::N + r * Cfg::THREADS + tl] = acc1[r];
      }
      sched_fence();
      e = e_next;
    }
    row = next;
  }
  rearm_row_counters(sched, tau);
}

template <typename Sh>
static hipError_t launch_blindrot_t(const tn_plan* p, const void* a, const uint32_t* exps, const void* bhat, void* c, size_t batch, size_t steps,
                                    size_t terms, u32 base_log, bool balanced, hipStream_t s) {
  typedef typename Sh::E E;
  typedef typename Sh::Cfg Cfg;
  if constexpr (!blindrot_lds_fits<Sh>()) {
    return hipErrorInvalidValue;             // refused by check_blind_rotate; nothing is instantiated for the shape
  } else {
    constexpr int LOGN = Sh::LOGN, LPT = Sh::LPT, XL = blindrot_lds_words<Sh>();
    constexpr bool LAZY = Sh::LAZY;
    static_assert((size_t)dot_waves<E, LOGN, LPT, LAZY>() == BLINDROT_WAVES || LPT >= 4, "blindrot_lds_words counts with the kernel's waves per SIMD");
    const FusedProductLaunch<Sh> L(p);
    const u32 b32 = (u32)batch, k32 = (u32)steps, t32 = (u32)terms, bal = balanced ? 1u : 0u;
    constexpr size_t lds_bytes = blindrot_lds_bytes<Sh>(XL);
    static_assert(lds_bytes == fused_lds_bytes<Sh>(2, (size_t)XL * Cfg::THREADS + 2 * (size_t)Cfg::N), "the CMux step's layout plus two rows of n words");
    static_assert(lds_bytes <= BLINDROT_WG_LDS, "one workgroup's LDS");
    auto kern = polydot_blindrot_kernel<E, LOGN, LPT, LAZY, false, XL>;
    if constexpr (L.HAS_BC) {
      if (L.use_bc) kern = polydot_blindrot_kernel<E, LOGN, LPT, LAZY, true, XL>;
    }
    // A row is priced as `steps` CMux rows: 2 * terms forward transforms and two inverses, steps times, between two atomics.
    return launch_persistent(p, s, reinterpret_cast<const void*>(kern), Cfg::THREADS, lds_bytes, dot_row_bytes(Cfg::N * sizeof(E), 2 * terms * steps),
                             batch, FUSED_ROWS, [&](u32 grid, u32* sched, u32 chunk) {
      hipLaunchKernelGGL(kern, dim3(grid), dim3(Cfg::THREADS), lds_bytes, s, L.su.ar, L.fwd(), L.inv(),
                         (const E*)a, exps, (const E*)bhat, (E*)c, b32, k32, t32, base_log, bal, sched, chunk);
      return hipGetLastError();
    });
  }
}

hipError_t launch_polydot_blindrot(const tn_plan* p, const void* a, const uint32_t* exps, const void* bhat, void* c, size_t batch, size_t steps,
                                   size_t terms, u32 base_log, bool balanced, hipStream_t s) {
  if (batch == 0) return hipSuccess;
  if (steps == 0) return hipErrorInvalidValue;       // (a row without steps would never hand itself on)
  return dispatch_fused_shape(p, [&](auto sh) { return launch_blindrot_t<decltype(sh)>(p, a, exps, bhat, c, batch, steps, terms, base_log, balanced, s); });
}

}  // namespace tn
