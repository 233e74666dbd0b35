// One-pass frame normalisation: uint8 pixel -> bf16 of (float)x / 255.
//
// Replaces the three element-wise passes `x.float() / 255.0` + autocast's
// bf16 cast in front of conv1 (1 B read + 2 B written per pixel instead of
// 19 B moved).  Pure streaming: each lane takes 16 pixels with one 16-byte
// load and writes them with two 16-byte stores; a scalar loop finishes the
// last n % 16 pixels.
//
// The byte -> bf16 expression lives in frame_cast.h, shared with the fused
// encoder forward (encoder_fwd.hip).

#include "common.h"
#include "frame_cast.h"

extern "C" __global__ void frame_cast_u8_bf16_kernel(
    const uint8_t* __restrict__ in,  // [n], 16-byte aligned if n_vec > 0
    uint16_t* __restrict__ out,      // [n] bf16 bits, 16-byte aligned if n_vec > 0
    long n_vec,                      // number of 16-pixel groups done vectorised
    long n) {
  const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long stride = (long)gridDim.x * blockDim.x;
  const uint4* in4 = reinterpret_cast<const uint4*>(in);
  uint4* out4 = reinterpret_cast<uint4*>(out);
  for (long v = tid; v < n_vec; v += stride) {
    const uint4 p = in4[v];
    uint4 a, b;
    frame_bf16_x16(p, a, b);
    out4[2 * v] = a;
    out4[2 * v + 1] = b;
  }
  for (long i = n_vec * 16 + tid; i < n; i += stride)
    out[i] = (uint16_t)frame_bf16_bits(in[i]);
}

extern "C" int frame_cast_u8_bf16(const void* in, void* out, long n,
                                  hipStream_t stream) {
  if (n <= 0) return 0;
  // vector path needs both pointers 16-byte aligned; otherwise all scalar
  const bool aligned =
      (((uintptr_t)in | (uintptr_t)out) & (uintptr_t)15) == 0;
  const long n_vec = aligned ? n / 16 : 0;
  const int block = 256;
  const long work = n_vec > 0 ? n_vec : n;
  hipLaunchKernelGGL(frame_cast_u8_bf16_kernel, dim3(grid_1d(work, block)),
                     dim3(block), 0, stream, (const uint8_t*)in,
                     (uint16_t*)out, n_vec, n);
  CHECK_LAUNCH();
  return 0;
}
