// kernels_galois.hip — the ring automorphism sigma_g : a(x) -> a(x^g) mod (x^n + 1) on coefficient rows (automorphism_kernel:
// every plan) and on prepared rows (automorphism_hat_kernel: fused plans), with their launchers.  A translation unit of its
// own: it shares no template and no LDS symbol with the fused families.  The per-thread code is galois_core.h's.
#include <hip/hip_runtime.h>
#include "plan.h"
#include "galois_core.h"

namespace tn {

// Both kernels: a workgroup of GALOIS_THREADS threads loops over tiles of galois_tile_rows(logn) rows at a grid stride.  Per
// tile: the rows into the LDS image at unit stride (non-temporal), a barrier, then `count` images of every row out of the
// image, stores at unit stride (non-temporal), and a barrier before the image is written again.  Traffic per input row:
// (1 + count) rows.  LDS reads: the coefficient kernel's lanes walk the image at the odd stride g^-1 and the prepared kernel's
// 32-lane groups hit 32 consecutive words in a permuted order, both conflict free on an unpadded image.
template <typename E>
__global__ void __launch_bounds__(GALOIS_THREADS)
automorphism_kernel(const E* __restrict__ a, E* __restrict__ out, u32 batch, u32 logn, E q, typename TwOf<E>::type one, const GaloisList gl) {
  extern __shared__ __attribute__((aligned(16))) unsigned char tn_smem_galois[];
  E* img = reinterpret_cast<E*>(tn_smem_galois);
  const u32 tiles = galois_tiles(batch, logn);
  for (u32 tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const GaloisTile t = galois_tile(tile, batch, logn, gl.count);
    galois_stage<E, true>(a + t.in_offset, img, t.words, threadIdx.x, q, one);
    __syncthreads();
    galois_gather<E>(img, out + t.out_offset, t.words, logn, gl, q, threadIdx.x);
    __syncthreads();
  }
}

template <typename E, bool BC>
__global__ void __launch_bounds__(GALOIS_THREADS)
automorphism_hat_kernel(const Arith<E> ar, const typename TwOf<E>::type* __restrict__ psi_pow, const E* __restrict__ xhat, E* __restrict__ out,
                        u32 rows_total, u32 logn, u32 lpt, const GaloisList gl) {
  extern __shared__ __attribute__((aligned(16))) unsigned char tn_smem_galois_hat[];
  typedef typename TwOf<E>::type Tw;
  Tw* ftab = reinterpret_cast<Tw*>(tn_smem_galois_hat);                       // BC: the factor records, in front of the image
  E* img = reinterpret_cast<E*>(tn_smem_galois_hat + (BC ? galois_factor_records(logn) * sizeof(Tw) : 0));
  if constexpr (BC) galois_stage_factors<E>(psi_pow, ftab, logn, threadIdx.x);      // (read behind the first tile's barrier)
  const u32 tiles = galois_tiles(rows_total, logn);
  for (u32 tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const GaloisTile t = galois_tile(tile, rows_total, logn, gl.count);
    galois_stage<E, false>(xhat + t.in_offset, img, t.words, threadIdx.x, ar.q, ar.one);
    __syncthreads();
    galois_gather_hat<E, BC>(img, out + t.out_offset, t.words, logn, lpt, gl, ar, ftab, threadIdx.x);
    __syncthreads();
  }
}

// As many workgroups as stay resident beside each other (LDS: one tile each, at most 64 KiB; 8 workgroups fill a CU's wave
// slots), or one per tile when there are fewer tiles.
constexpr size_t GALOIS_CU_LDS = 160 * 1024;
static hipError_t galois_launch_shape(const tn_plan* p, const void* kern, size_t rows, u32& grid, size_t& lds_bytes, size_t extra_lds = 0) {
  lds_bytes = (size_t)galois_tile_words(p->logn) * (size_t)p->elem_bytes + extra_lds;
  if (lds_bytes > 48 * 1024) {
    hipError_t e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    if (e != hipSuccess) return e;
  }
  size_t per_cu = GALOIS_CU_LDS / lds_bytes;
  if (per_cu > 8) per_cu = 8;
  const size_t tiles = galois_tiles((u32)rows, p->logn), resident = per_cu * (size_t)p->num_cus;
  grid = (u32)(tiles < resident ? tiles : resident);
  return hipSuccess;
}

template <typename E>
static hipError_t launch_automorphism_t(const tn_plan* p, const void* a, void* out, size_t batch, const GaloisList& gl, hipStream_t s) {
  const auto kern = automorphism_kernel<E>;
  u32 grid = 0;
  size_t lds_bytes = 0;
  hipError_t e = galois_launch_shape(p, reinterpret_cast<const void*>(kern), batch, grid, lds_bytes);
  if (e != hipSuccess) return e;
  const Arith<E>& ar = plan_arith<E>(p);
  hipLaunchKernelGGL(kern, dim3(grid), dim3(GALOIS_THREADS), lds_bytes, s, (const E*)a, (E*)out, (u32)batch, p->logn, ar.q, ar.one, gl);
  return hipGetLastError();
}

// galois: count odd elements below 2n (check_automorphism); the kernel takes their inverses mod 2n
hipError_t launch_automorphism(const tn_plan* p, const void* a, void* out, size_t batch, const uint32_t* galois, size_t count, hipStream_t s) {
  if (batch == 0) return hipSuccess;
  GaloisList gl = {};
  gl.count = (u32)count;
  for (size_t m = 0; m < count; ++m) gl.v[m] = galois_inverse(galois[m], p->logn);
  return p->elem_bytes == 8 ? launch_automorphism_t<u64>(p, a, out, batch, gl, s) : launch_automorphism_t<u32>(p, a, out, batch, gl, s);
}

template <typename E, bool BC>
static hipError_t launch_automorphism_hat_t(const tn_plan* p, const void* xhat, void* out, size_t rows, const GaloisList& gl, hipStream_t s) {
  const auto kern = automorphism_hat_kernel<E, BC>;
  u32 grid = 0;
  size_t lds_bytes = 0;
  hipError_t e = galois_launch_shape(p, reinterpret_cast<const void*>(kern), rows, grid, lds_bytes,
                                     BC ? galois_factor_records(p->logn) * sizeof(typename TwOf<E>::type) : 0);
  if (e != hipSuccess) return e;
  const PlanView<E> pv = make_view<E>(p);
  hipLaunchKernelGGL(kern, dim3(grid), dim3(GALOIS_THREADS), lds_bytes, s, pv.ar, pv.psi_pow, (const E*)xhat, (E*)out, (u32)rows, p->logn,
                     (u32)fused_lpt((int)p->logn), gl);
  return hipGetLastError();
}

// Prepared rows are in the base-case format exactly where the product family runs the base case (launch_plan.h: fused_use_bc).
hipError_t launch_automorphism_prepared(const tn_plan* p, const void* xhat, void* out, size_t rows, const uint32_t* galois, size_t count, hipStream_t s) {
  if (rows == 0) return hipSuccess;
  if (!p->has_fused) return hipErrorInvalidValue;
  GaloisList gl = {};
  gl.count = (u32)count;
  for (size_t m = 0; m < count; ++m) gl.v[m] = galois[m];
  if (p->elem_bytes == 4) return launch_automorphism_hat_t<u32, false>(p, xhat, out, rows, gl, s);
  const bool bc = with_fused_shape(p->elem_bytes, p->lazy, p->logn, false, [&](auto sh) { return fused_use_bc<decltype(sh)>(p->bc_ok); });
  return bc ? launch_automorphism_hat_t<u64, true>(p, xhat, out, rows, gl, s) : launch_automorphism_hat_t<u64, false>(p, xhat, out, rows, gl, s);
}

}  // namespace tn
