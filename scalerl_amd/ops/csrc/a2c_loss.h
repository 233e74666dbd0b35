// Launcher of the fused GAE actor-critic loss (a2c_loss.hip).  Not exported:
// the entry point is gae_scan (scans.hip), which calls it when logits != null.
#pragma once

#include <hip/hip_runtime.h>

#define A2C_TILE_B 8    // batch columns per workgroup
#define A2C_MAX_T 512   // 3 LDS arrays of T*A2C_TILE_B floats = 48 KiB

int a2c_loss_launch(const float* rewards, const float* values,
                    const float* bootstrap, const float* discounts, float lam,
                    long T, long B, float* advantages, float* returns,
                    const float* logits, const long* actions, long A,
                    float value_coef, float entropy_coef, float* grad_logits,
                    float* grad_values, float* loss_out, hipStream_t stream);
