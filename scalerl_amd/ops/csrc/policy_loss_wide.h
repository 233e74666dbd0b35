// Launchers of the wide-row (A > 32) IMPALA and PPO loss kernels
// (policy_loss_wide.hip).  Not exported: the entry points stay
// impala_fused_loss (vtrace_loss.hip) and ppo_fused_loss (ppo_loss.hip),
// which call these above their own 32-action bound.  Arguments and return
// codes are those of the entry points.
#pragma once

#include <hip/hip_runtime.h>

#define PLW_REG_K 8  // logits a lane keeps: a row of <= 8*64 = 512 actions
                     // stays in registers between statistics and gradient

int impala_loss_wide_launch(
    const float* behavior_logits, const float* target_logits,
    const long* actions, const float* rewards, const float* discounts,
    const float* values, const float* bootstrap,
    float clip_rho, float clip_c, float clip_pg_rho,
    float baseline_cost, float entropy_cost,
    long T, long B, long A,
    float* grad_logits, float* grad_values, float* loss_out, float* vs_out,
    hipStream_t stream);

int ppo_loss_wide_launch(const float* logits, const long* actions,
                         const float* old_logp, const float* adv,
                         const float* returns, const float* values,
                         float clip_eps, float vcoef, float ecoef,
                         long N, long A, float* grad_logits,
                         float* grad_values, float* loss_out,
                         hipStream_t stream);
