// bf16 / MFMA vector types shared by the encoder conv kernels, and the one
// statement of the v_mfma_f32_16x16x32_bf16 fragment maps they all index by.
//
//   A (16x32): lane l, elem j -> row = l & 15, k = (l >> 4) * 8 + j
//   B (32x16): lane l, elem j -> col = l & 15, k = (l >> 4) * 8 + j
//   C/D:       lane l, reg r  -> col = l & 15, row = (l >> 4) * 4 + r
//
// The maps are validated on-device by mfma_selftest (mfma_selftest.hip),
// which the gpu tests run before any conv test: if a map is wrong there is
// one place to fix.
#pragma once

typedef __bf16 bf16_t;
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef bf16_t bf16x8 __attribute__((ext_vector_type(8)));
typedef bf16_t bf16x4 __attribute__((ext_vector_type(4)));
typedef bf16_t bf16x2 __attribute__((ext_vector_type(2)));
