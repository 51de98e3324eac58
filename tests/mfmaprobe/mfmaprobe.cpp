// mfmaprobe.cpp — TEST INFRASTRUCTURE: ONE int8 matrix step of the matrix-core key switch (lwe_mfma_core.h: lwe_mfma_step_lane,
// v_mfma_i32_16x16x64_i8) on caller-given fragments, so tests/test_gpu_lwe_mfma.py checks the lane -> element map of A, B and
// C/D that the header's host loop (lwe_mfma_step_wave) states against the instruction itself.  A library of its own
// (tests/mfmaprobe/_build/libmfmaprobe.so), not part of libtinyntt.so.
#include <hip/hip_runtime.h>
#include "../../tiny_ntt_amd/csrc/lwe_mfma_core.h"

using namespace tn;

__global__ void __launch_bounds__(LWE_MFMA_LANES) mfmaprobe_kernel(const LweFrag* a, const LweFrag* b, LweTile* c) {
  LweTile acc = c[threadIdx.x];
  lwe_mfma_step_lane(a[threadIdx.x], b[threadIdx.x], acc);
  c[threadIdx.x] = acc;
}

namespace {
struct DevBuf {
  void* p = nullptr;
  ~DevBuf() { if (p) (void)hipFree(p); }
};
}  // namespace
#define MP_HIP(x) do { const hipError_t e_ = (x); if (e_ != hipSuccess) return 1000 + (int)e_; } while (0)

// a, b: 64 lanes x 16 bytes; c: 64 lanes x 4 sums, the accumulator in, the result out (host memory).  0 ok, 1000 + hipError_t of
// the first HIP call that failed.
extern "C" int mfmaprobe_step(const void* a, const void* b, int32_t* c) {
  const size_t ab = LWE_MFMA_LANES * sizeof(LweFrag), cd = LWE_MFMA_LANES * sizeof(LweTile);
  DevBuf da, db, dc;
  MP_HIP(hipMalloc(&da.p, ab));
  MP_HIP(hipMalloc(&db.p, ab));
  MP_HIP(hipMalloc(&dc.p, cd));
  MP_HIP(hipMemcpy(da.p, a, ab, hipMemcpyHostToDevice));
  MP_HIP(hipMemcpy(db.p, b, ab, hipMemcpyHostToDevice));
  MP_HIP(hipMemcpy(dc.p, c, cd, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(mfmaprobe_kernel, dim3(1), dim3(LWE_MFMA_LANES), 0, 0, (const LweFrag*)da.p, (const LweFrag*)db.p, (LweTile*)dc.p);
  MP_HIP(hipGetLastError());
  MP_HIP(hipDeviceSynchronize());
  MP_HIP(hipMemcpy(c, dc.p, cd, hipMemcpyDeviceToHost));
  return 0;
}
