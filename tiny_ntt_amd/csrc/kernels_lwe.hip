// kernels_lwe.hip — the LWE ends of a programmable bootstrap on every plan: the modulus switch to 2n (lwe_modswitch_kernel),
// the sample extraction (lwe_sample_extract_kernel) and the LWE-to-LWE key switch (lwe_keyswitch_kernel), with their launchers.
// A translation unit of its own: it shares no template and no LDS symbol with the fused families.  The per-word and per-tile
// code is lwe_core.h's.  No launcher allocates, copies or synchronises.
#include <hip/hip_runtime.h>
#include "plan.h"
#include "lwe_core.h"

namespace tn {

// lwe [batch][dim + 1] -> exps [dim + 1][batch], tiles of 64 x 64 words through an LDS image of exponents at a grid stride:
// both global sides at unit stride.
template <typename E>
__global__ void __launch_bounds__(LWE_THREADS)
lwe_modswitch_kernel(const Arith<E> ar, const E* __restrict__ lwe, u32* __restrict__ exps, u32 batch, u32 dim, u32 logn) {
  __shared__ u32 img[LWE_MS_IMAGE];
  const u32 tiles = lwe_ms_tiles(batch, dim);
  for (u32 tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const LweMsTile t = lwe_ms_tile(tile, batch, dim);
    lwe_ms_stage<E>(lwe, img, t, dim, threadIdx.x, ar, logn);
    __syncthreads();
    lwe_ms_store(img, exps, t, batch, threadIdx.x);
    __syncthreads();
  }
}

// a [batch][2][n] -> lwe [batch][n + 1]: the automorphism kernel's tile loop (galois_core.h) over the c1 rows.
template <typename E>
__global__ void __launch_bounds__(LWE_THREADS)
lwe_sample_extract_kernel(const Arith<E> ar, const E* __restrict__ a, E* __restrict__ lwe, u32 batch, u32 logn, u32 index) {
  extern __shared__ __attribute__((aligned(16))) unsigned char tn_smem_lwe[];
  E* img = reinterpret_cast<E*>(tn_smem_lwe);
  const u32 tiles = galois_tiles(batch, logn);
  for (u32 tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const GaloisTile t = galois_tile(tile, batch, logn, 1);
    lwe_extract_stage<E>(a, img, t.row0, t.words, logn, threadIdx.x, ar);
    __syncthreads();
    lwe_extract_gather<E>(a, img, lwe, t.row0, t.words, logn, index, threadIdx.x, ar);
    __syncthreads();
  }
}

// lwe [batch][n + 1] -> a [batch][2][n]: the extraction's inverse, element-wise at a grid stride (lwe_embed_words).
template <typename E>
__global__ void __launch_bounds__(LWE_THREADS)
lwe_embed_kernel(const Arith<E> ar, const E* __restrict__ lwe, E* __restrict__ a, u32 batch, u32 logn, u32 index) {
  lwe_embed_words<E>(lwe, a, batch, logn, index, (size_t)blockIdx.x * LWE_THREADS + threadIdx.x, (size_t)gridDim.x * LWE_THREADS, ar);
}

// A tile of LWE_KS_ROWS rows by LWE_KS_COLS columns per pass of the loop, a thread per column with LWE_KS_ROWS 128-bit sums;
// the input words go through the digit slab chunk by chunk.  Threads past column n_out cut digits and keep the barriers.
template <typename E, bool BAL>
__global__ void __launch_bounds__(LWE_THREADS)
lwe_keyswitch_kernel(const Arith<E> ar, const LweRed<E> red, const E* __restrict__ lwe, const E* __restrict__ ksk, E* __restrict__ out, u32 batch,
                     u32 n_in, u32 n_out, u32 terms, u32 w) {
  __shared__ __attribute__((aligned(16))) u32 dig[LWE_KS_SLOTS * LWE_KS_ROWS];
  const u32 tiles = lwe_ks_tiles(batch, n_out), chunk = lwe_ks_chunk(terms);
  const size_t pitch = (size_t)n_out + 1;
  for (u32 tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const LweKsTile t = lwe_ks_tile(tile, batch);
    const u32 col = t.col0 + threadIdx.x;
    LweAcc acc[LWE_KS_ROWS];
#pragma unroll
    for (u32 r = 0; r < LWE_KS_ROWS; ++r) acc[r] = {0, 0};
    for (u32 i0 = 0; i0 < n_in; i0 += chunk) {
      const u32 len = n_in - i0 < chunk ? n_in - i0 : chunk;
      lwe_ks_cut<E>(lwe, dig, t, n_in, i0, len, terms, w, BAL, threadIdx.x, ar);
      __syncthreads();
      if (col <= n_out) lwe_ks_accumulate<E, BAL>(ksk + col, pitch, (size_t)i0 * terms, dig, len * terms, acc, ar);
      __syncthreads();
    }
    if (col <= n_out) lwe_ks_finish<E>(lwe, out, t, n_in, n_out, col, acc, red, ar);
  }
}

// as many workgroups as `per_cu` of them beside each other on every CU, or one per tile when there are fewer tiles
static u32 lwe_grid(const tn_plan* p, size_t tiles, size_t per_cu) {
  const size_t resident = per_cu * (size_t)p->num_cus;
  return (u32)(tiles < resident ? tiles : resident);
}

template <typename E>
static hipError_t launch_lwe_modswitch_t(const tn_plan* p, const void* lwe, uint32_t* exps, size_t batch, size_t dim, hipStream_t s) {
  const u32 grid = lwe_grid(p, lwe_ms_tiles((u32)batch, (u32)dim), 8);
  hipLaunchKernelGGL(lwe_modswitch_kernel<E>, dim3(grid), dim3(LWE_THREADS), 0, s, plan_arith<E>(p), (const E*)lwe, exps, (u32)batch, (u32)dim, p->logn);
  return hipGetLastError();
}
hipError_t launch_lwe_modswitch(const tn_plan* p, const void* lwe, uint32_t* exps, size_t batch, size_t dim, hipStream_t s) {
  if (batch == 0) return hipSuccess;
  return p->elem_bytes == 8 ? launch_lwe_modswitch_t<u64>(p, lwe, exps, batch, dim, s) : launch_lwe_modswitch_t<u32>(p, lwe, exps, batch, dim, s);
}

template <typename E>
static hipError_t launch_lwe_sample_extract_t(const tn_plan* p, const void* a, void* lwe, size_t batch, u32 index, hipStream_t s) {
  const auto kern = lwe_sample_extract_kernel<E>;
  const size_t lds_bytes = (size_t)galois_tile_words(p->logn) * sizeof(E);       // 64 KiB at most (n = 8192, 64-bit words)
  if (lds_bytes > 48 * 1024) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    if (e != hipSuccess) return e;
  }
  size_t per_cu = (160 * 1024) / lds_bytes;
  if (per_cu > 8) per_cu = 8;
  const u32 grid = lwe_grid(p, galois_tiles((u32)batch, p->logn), per_cu);
  hipLaunchKernelGGL(kern, dim3(grid), dim3(LWE_THREADS), lds_bytes, s, plan_arith<E>(p), (const E*)a, (E*)lwe, (u32)batch, p->logn, index);
  return hipGetLastError();
}
hipError_t launch_lwe_sample_extract(const tn_plan* p, const void* a, void* lwe, size_t batch, u32 index, hipStream_t s) {
  if (batch == 0) return hipSuccess;
  return p->elem_bytes == 8 ? launch_lwe_sample_extract_t<u64>(p, a, lwe, batch, index, s) : launch_lwe_sample_extract_t<u32>(p, a, lwe, batch, index, s);
}

template <typename E>
static hipError_t launch_lwe_embed_t(const tn_plan* p, const void* lwe, void* a, size_t batch, u32 index, hipStream_t s) {
  const size_t words = (batch * 2) << p->logn;                          // below 2^32 (check_lwe_embed)
  const u32 grid = lwe_grid(p, (words + LWE_THREADS - 1) / LWE_THREADS, 8);
  hipLaunchKernelGGL(lwe_embed_kernel<E>, dim3(grid), dim3(LWE_THREADS), 0, s, plan_arith<E>(p), (const E*)lwe, (E*)a, (u32)batch, p->logn, index);
  return hipGetLastError();
}
hipError_t launch_lwe_embed(const tn_plan* p, const void* lwe, void* a, size_t batch, u32 index, hipStream_t s) {
  if (batch == 0) return hipSuccess;
  return p->elem_bytes == 8 ? launch_lwe_embed_t<u64>(p, lwe, a, batch, index, s) : launch_lwe_embed_t<u32>(p, lwe, a, batch, index, s);
}

template <typename E, bool BAL>
static hipError_t launch_lwe_keyswitch_t(const tn_plan* p, const void* lwe, const void* ksk, void* out, size_t batch, size_t n_in, size_t n_out,
                                         size_t terms, u32 base_log, hipStream_t s) {
  // as many workgroups per CU as are resident beside each other (32 KiB of LDS each: at most 4; registers leave 3 of the
  // 32-bit unsigned instantiation), so that the grid-stride loop has no straggling part of the grid
  const auto kern = lwe_keyswitch_kernel<E, BAL>;
  int per_cu = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, (int)LWE_THREADS, 0) != hipSuccess || per_cu < 1) per_cu = 1;
  const u32 grid = lwe_grid(p, lwe_ks_tiles((u32)batch, (u32)n_out), per_cu > 4 ? 4 : (size_t)per_cu);
  hipLaunchKernelGGL(kern, dim3(grid), dim3(LWE_THREADS), 0, s, plan_arith<E>(p), h_lwe_red<E>(p->q), (const E*)lwe,
                     (const E*)ksk, (E*)out, (u32)batch, (u32)n_in, (u32)n_out, (u32)terms, base_log);
  return hipGetLastError();
}
hipError_t launch_lwe_keyswitch(const tn_plan* p, const void* lwe, const void* ksk, void* out, size_t batch, size_t n_in, size_t n_out, size_t terms,
                                u32 base_log, bool balanced, hipStream_t s) {
  if (batch == 0) return hipSuccess;
  if (p->elem_bytes == 8)
    return balanced ? launch_lwe_keyswitch_t<u64, true>(p, lwe, ksk, out, batch, n_in, n_out, terms, base_log, s)
                    : launch_lwe_keyswitch_t<u64, false>(p, lwe, ksk, out, batch, n_in, n_out, terms, base_log, s);
  return balanced ? launch_lwe_keyswitch_t<u32, true>(p, lwe, ksk, out, batch, n_in, n_out, terms, base_log, s)
                  : launch_lwe_keyswitch_t<u32, false>(p, lwe, ksk, out, batch, n_in, n_out, terms, base_log, s);
}

}  // namespace tn
