// uint8 pixel -> bf16 bits of (float)x / 255, shared by frame_cast.hip and
// encoder_fwd.hip so that the fused encoder forward and the cast that feeds
// MIOpen's conv1 wgrad see the same bits for all 256 byte values.
//
// Rounding: bf16 is taken from the fp32 value by round-to-nearest-even, the
// same as torch's fp32 -> bf16 cast.  x * (1/255) and x / 255 differ in the
// last fp32 bit for some x but round to the same bf16 for all 256 byte
// values (tests/test_frame_cast.py checks every value), so the cheaper
// multiply is used.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

__device__ __forceinline__ uint32_t frame_bf16_bits(uint32_t byte) {
  const float f = (float)byte * (1.0f / 255.0f);
  uint32_t u = __float_as_uint(f);
  // f is finite and in [0,1]: plain round-to-nearest-even on the top 16 bits
  u += 0x7fffu + ((u >> 16) & 1u);
  return u >> 16;
}

// pixels 2k and 2k+1 of a 4-byte word -> one packed pair of bf16
__device__ __forceinline__ uint32_t frame_bf16_pair(uint32_t word, int k) {
  const uint32_t lo = frame_bf16_bits((word >> (16 * k)) & 0xffu);
  const uint32_t hi = frame_bf16_bits((word >> (16 * k + 8)) & 0xffu);
  return lo | (hi << 16);
}

// 16 pixels (one 16-byte load) -> 16 bf16 (two 16-byte stores)
__device__ __forceinline__ void frame_bf16_x16(const uint4 p, uint4& a,
                                               uint4& b) {
  a.x = frame_bf16_pair(p.x, 0);
  a.y = frame_bf16_pair(p.x, 1);
  a.z = frame_bf16_pair(p.y, 0);
  a.w = frame_bf16_pair(p.y, 1);
  b.x = frame_bf16_pair(p.z, 0);
  b.y = frame_bf16_pair(p.z, 1);
  b.z = frame_bf16_pair(p.w, 0);
  b.w = frame_bf16_pair(p.w, 1);
}
