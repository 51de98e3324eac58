// kernels_lwe_mfma.hip — the LWE-to-LWE key switch on the matrix cores: the key prepared once as int8 limb planes in B-fragment
// order (lwe_ksk_prepare_kernel), then out = digits x limbs with v_mfma_i32_16x16x64_i8 and exact sums
// (lwe_keyswitch_mfma_kernel), bit for bit what lwe_keyswitch_kernel writes.  A translation unit of its own; the per-lane and
// per-tile code is lwe_mfma_core.h's.  No launcher allocates, copies or synchronises.
#include <hip/hip_runtime.h>
#include "plan.h"
#include "lwe_mfma_core.h"

namespace tn {

// ksk [n_in terms][n_out + 1] words -> kprep: a transpose through an LDS image of limb bytes at a grid stride, both global sides
// at unit stride.
template <typename E>
__global__ void __launch_bounds__(LWE_THREADS)
lwe_ksk_prepare_kernel(const Arith<E> ar, const E* __restrict__ ksk, signed char* __restrict__ kprep, u32 slots, u32 n_out, u32 limbs) {
  __shared__ __attribute__((aligned(16))) signed char img[LWE_MFMA_PREP_IMAGE];
  const u32 steps = (u32)lwe_mfma_steps(slots, 1), cts = (u32)lwe_mfma_col_tiles(n_out), tiles = lwe_mfma_prep_tiles(steps, cts);
  for (u32 tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const LwePrepTile t = lwe_mfma_prep_tile(tile, steps);
    lwe_mfma_prep_stage<E>(ksk, img, t, slots, n_out, limbs, threadIdx.x, ar);
    __syncthreads();
    lwe_mfma_prep_store(img, kprep, t, steps, cts, limbs, threadIdx.x);
    __syncthreads();
  }
}

// A tile of LWE_MFMA_ROWS rows by LWE_MFMA_COLS columns per pass of the loop; wave v owns column tile ct0 + v with
// LWE_MFMA_ROW_TILES x L accumulator tiles and as many times 4 wide sums.  The digits go through the image chunk by chunk; waves
// whose column tile lies past the key cut digits and keep the barriers.  Row tiles past the batch run no matrix step.
template <typename E, u32 L>
__global__ void __launch_bounds__(LWE_THREADS)
lwe_keyswitch_mfma_kernel(const Arith<E> ar, const LweRed<E> red, const LweAcc offset, const E* __restrict__ lwe, const signed char* __restrict__ kprep,
                          E* __restrict__ out, u32 batch, u32 n_in, u32 n_out, u32 terms, u32 w, u32 balanced) {
  __shared__ __attribute__((aligned(16))) signed char img[LWE_MFMA_IMAGE];
  const u32 slots = n_in * terms, steps = (u32)lwe_mfma_steps(slots, 1), cts = (u32)lwe_mfma_col_tiles(n_out);
  const u32 tiles = lwe_mfma_tiles(batch, n_out);
  const u32 lane = threadIdx.x & (LWE_MFMA_LANES - 1), wave = __builtin_amdgcn_readfirstlane(threadIdx.x / LWE_MFMA_LANES);
  for (u32 tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const LweMfmaTile t = lwe_mfma_tile(tile, batch);
    const u32 ct = t.ct0 + wave, rts = (t.rows + 15) / 16;
    const bool live = ct < cts;
    LweTile acc[LWE_MFMA_ROW_TILES][L];
    LweAcc wide[LWE_MFMA_ROW_TILES][4];
#pragma unroll
    for (u32 rt = 0; rt < LWE_MFMA_ROW_TILES; ++rt) {
#pragma unroll
      for (u32 l = 0; l < L; ++l) acc[rt][l] = {{0, 0, 0, 0}};
#pragma unroll
      for (u32 e = 0; e < 4; ++e) wide[rt][e] = {0, 0};
    }
    u32 chunks = 0;
    for (u32 k0 = 0; k0 < slots; k0 += LWE_MFMA_CHUNK) {
      lwe_mfma_cut<E>(lwe, img, t, n_in, slots, k0, terms, w, balanced != 0, threadIdx.x, ar);
      __syncthreads();
      if (live) {
        const u32 cs = lwe_mfma_chunk_steps(slots, k0), step0 = k0 / LWE_MFMA_K_STEP;
        for (u32 s = 0; s < cs; ++s) {
          LweFrag a[LWE_MFMA_ROW_TILES];
#pragma unroll
          for (u32 rt = 0; rt < LWE_MFMA_ROW_TILES; ++rt) a[rt] = lwe_mfma_a_frag(img, s, rt, lane);
#pragma unroll
          for (u32 l = 0; l < L; ++l) {
            const LweFrag b = lwe_mfma_b_frag(kprep, ct, step0 + s, l, steps, L, lane);
#pragma unroll
            for (u32 rt = 0; rt < LWE_MFMA_ROW_TILES; ++rt)
              if (rt < rts) lwe_mfma_step_lane(a[rt], b, acc[rt][l]);
          }
        }
        if (++chunks == LWE_MFMA_FLUSH_CHUNKS) {       // LWE_MFMA_FLUSH_PRODUCTS products in every 32-bit sum: fold before the next
          chunks = 0;
#pragma unroll
          for (u32 rt = 0; rt < LWE_MFMA_ROW_TILES; ++rt) lwe_mfma_fold<L>(acc[rt], wide[rt]);
        }
      }
      __syncthreads();
    }
    if (live) {
#pragma unroll
      for (u32 rt = 0; rt < LWE_MFMA_ROW_TILES; ++rt) {
        if (rt < rts) {
          lwe_mfma_fold<L>(acc[rt], wide[rt]);
          lwe_mfma_finish<E>(lwe, out, t, rt, lane, ct * LWE_MFMA_COL_TILE + (lane & 15), n_in, n_out, wide[rt], offset, red, ar);
        }
      }
    }
  }
}

// as many workgroups as `per_cu` of them beside each other on every CU, or one per tile when there are fewer tiles
static u32 lwe_mfma_grid(const tn_plan* p, size_t tiles, int per_cu) {
  const size_t resident = (size_t)(per_cu < 1 ? 1 : per_cu) * (size_t)p->num_cus;
  return (u32)(tiles < resident ? tiles : resident);
}

template <typename E>
static hipError_t launch_lwe_ksk_prepare_t(const tn_plan* p, const void* ksk, void* kprep, size_t n_in, size_t n_out, size_t terms, hipStream_t s) {
  const u32 slots = (u32)(n_in * terms);
  const size_t tiles = lwe_mfma_prep_tiles((u32)lwe_mfma_steps(slots, 1), (u32)lwe_mfma_col_tiles(n_out));
  const u32 grid = lwe_mfma_grid(p, tiles, 4);                               // 32 KiB of LDS each
  hipLaunchKernelGGL(lwe_ksk_prepare_kernel<E>, dim3(grid), dim3(LWE_THREADS), 0, s, plan_arith<E>(p), (const E*)ksk, (signed char*)kprep, slots,
                     (u32)n_out, lwe_mfma_limbs(p->q));
  return hipGetLastError();
}
hipError_t launch_lwe_ksk_prepare(const tn_plan* p, const void* ksk, void* kprep, size_t n_in, size_t n_out, size_t terms, hipStream_t s) {
  return p->elem_bytes == 8 ? launch_lwe_ksk_prepare_t<u64>(p, ksk, kprep, n_in, n_out, terms, s)
                            : launch_lwe_ksk_prepare_t<u32>(p, ksk, kprep, n_in, n_out, terms, s);
}

template <typename E, u32 L>
static hipError_t launch_lwe_keyswitch_mfma_t(const tn_plan* p, const void* lwe, const void* kprep, void* out, size_t batch, size_t n_in, size_t n_out,
                                              size_t terms, u32 base_log, bool balanced, hipStream_t s) {
  const auto kern = lwe_keyswitch_mfma_kernel<E, L>;
  int per_cu = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, (int)LWE_THREADS, 0) != hipSuccess || per_cu < 1) per_cu = 1;
  const u32 grid = lwe_mfma_grid(p, lwe_mfma_tiles((u32)batch, (u32)n_out), per_cu);
  hipLaunchKernelGGL(kern, dim3(grid), dim3(LWE_THREADS), 0, s, plan_arith<E>(p), h_lwe_red<E>(p->q), h_lwe_mfma_offset(p->q, (int)sizeof(E)),
                     (const E*)lwe, (const signed char*)kprep, (E*)out, (u32)batch, (u32)n_in, (u32)n_out, (u32)terms, base_log, balanced ? 1u : 0u);
  return hipGetLastError();
}
// L = lwe_mfma_limbs(q): 1 .. 4 on 32-bit lanes (q < 2^31), 4 .. 8 on 64-bit lanes (2^31 <= q < 2^62)
hipError_t launch_lwe_keyswitch_prepared(const tn_plan* p, const void* lwe, const void* kprep, void* out, size_t batch, size_t n_in, size_t n_out,
                                         size_t terms, u32 base_log, bool balanced, hipStream_t s) {
  if (batch == 0) return hipSuccess;
  const u32 limbs = lwe_mfma_limbs(p->q);
#define TN_LWE_MFMA_CASE(E, L) \
  case L: return launch_lwe_keyswitch_mfma_t<E, L>(p, lwe, kprep, out, batch, n_in, n_out, terms, base_log, balanced, s)
  if (p->elem_bytes == 8) {
    switch (limbs) {
      TN_LWE_MFMA_CASE(u64, 4); TN_LWE_MFMA_CASE(u64, 5); TN_LWE_MFMA_CASE(u64, 6); TN_LWE_MFMA_CASE(u64, 7); TN_LWE_MFMA_CASE(u64, 8);
    }
  } else {
    switch (limbs) {
      TN_LWE_MFMA_CASE(u32, 1); TN_LWE_MFMA_CASE(u32, 2); TN_LWE_MFMA_CASE(u32, 3); TN_LWE_MFMA_CASE(u32, 4);
    }
  }
#undef TN_LWE_MFMA_CASE
  return hipErrorInvalidValue;                   // (no modulus of a plan has another limb count)
}

}  // namespace tn
