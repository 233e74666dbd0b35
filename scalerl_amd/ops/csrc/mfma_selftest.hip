// On-device check of the v_mfma_f32_16x16x32_bf16 fragment maps (mfma.h):
// D = A*B for one 16x16x32 tile, operands and result in plain row-major
// layouts.  Every encoder conv kernel indexes by the same maps.

#include "common.h"
#include "mfma.h"

extern "C" __global__ void mfma_selftest_kernel(
    const float* __restrict__ A,   // [16][32] row-major
    const float* __restrict__ B,   // [32][16] row-major
    float* __restrict__ D) {       // [16][16] row-major
  const int lane = threadIdx.x & (WAVE - 1);
  bf16x8 a, b;
  #pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int ar = lane & 15, ak = (lane >> 4) * 8 + j;
    const int bc = lane & 15, bk = (lane >> 4) * 8 + j;
    a[j] = (bf16_t)A[ar * 32 + ak];
    b[j] = (bf16_t)B[bk * 16 + bc];
  }
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc, 0, 0, 0);
  #pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int col = lane & 15, row = (lane >> 4) * 4 + r;
    D[row * 16 + col] = acc[r];
  }
}

extern "C" int mfma_selftest(const float* A, const float* B, float* D,
                             hipStream_t stream) {
  hipLaunchKernelGGL(mfma_selftest_kernel, dim3(1), dim3(64), 0, stream,
                     A, B, D);
  CHECK_LAUNCH();
  return 0;
}
