// Launchers of the fused LSTM cell kernels (lstm.hip), shared with the C++
// sequence loop (lstm_seq.hip).  They only enqueue; callers check the launch.
#pragma once

#include "common.h"

#define LSTM_CELL_BLOCK 256

void lstm_launch_mask_rows(const float* a, const float* b, const float* notdone,
                           float* a_out, float* b_out, long B, long H,
                           hipStream_t stream);

void lstm_launch_cell_fwd(float* gates, const float* c_in, float* h_out,
                          float* c_out, const float* nd_next, float* h_in_next,
                          float* c_in_next, long B, long H, hipStream_t stream);

void lstm_launch_cell_bwd(const float* gates, const float* c_in,
                          const float* c_out, const float* d_hs_t,
                          const float* g, const float* nd_next,
                          const float* nd_t, float* dc_carry, float* dgates,
                          long B, long H, hipStream_t stream);
