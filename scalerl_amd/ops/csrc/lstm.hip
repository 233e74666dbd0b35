// Fused LSTM cell kernels (forward + backward) with done-masking folded in.
//
// Reference semantics: AtariNet's per-step done-masked LSTM unroll
// (algorithms/utils/atari_model.py:109-120) — `state *= notdone[t]`, then
// one LSTM step.  The per-step GEMMs run through rocBLAS/hipBLASLt; every
// element-wise pass of a step is ONE kernel per direction, so a step-layer
// is GEMM + cell kernel forward and cell kernel + GEMM backward.  Gate order
// follows torch.nn.LSTM: [input, forget, cell(g), output] chunks of 4H.
//
// Forward overwrites the preactivation buffer with the ACTIVATED gates so
// backward needs no recompute and no extra memory.  The mask of step t+1
// must precede that step's recurrent GEMM, so the step-t kernel writes the
// NEXT step's masked state (hs_in[t+1], cs_in[t+1]) alongside its own
// outputs; step 0's masked state comes from lstm_mask_rows before the loop.
//
// Backward applies the mask's gradient where the values are consumed: the
// recurrent carry arrives as the RAW product g = dgates[t+1] @ W_hh and is
// masked by notdone[t+1] here; the dc carry leaves already masked by
// notdone[t].  Each thread reads and writes only its own carry element, so
// the dc carry is updated in place.
//
// Both drivers (the per-step Python loop in ops/lstm.py and the C++ loop in
// lstm_seq.hip) launch these same kernels.

#include "lstm_cell.h"

// a_out = a * nd[row], b_out = b * nd[row] (b/b_out may be null).  In-place
// (a_out == a) is safe: one element per thread.
extern "C" __global__ void lstm_mask_rows_kernel(
    const float* a, const float* b,
    const float* __restrict__ notdone,  // [B]
    float* a_out, float* b_out, long B, long H) {
  const long total = B * H;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    const float nd = notdone[i / H];
    a_out[i] = a[i] * nd;
    if (b != nullptr) b_out[i] = b[i] * nd;
  }
}

extern "C" __global__ void lstm_cell_fwd_kernel(
    float* __restrict__ gates,          // [B,4H] in: preact, out: activated
    const float* __restrict__ c_in,     // [B,H] masked cell state entering
    float* __restrict__ h_out,          // [B,H] hs[t]
    float* __restrict__ c_out,          // [B,H] cs_out[t]
    const float* __restrict__ nd_next,  // [B] notdone[t+1], null at t = T-1
    float* __restrict__ h_in_next,      // [B,H] hs_in[t+1] (unused if null nd)
    float* __restrict__ c_in_next,      // [B,H] cs_in[t+1] (unused if null nd)
    long B, long H) {
  const long total = B * H;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    const long b = i / H, j = i % H;
    float* grow = gates + b * 4 * H;
    const float ig = sigmoidf_(grow[j]);
    const float fg = sigmoidf_(grow[H + j]);
    const float gg = tanhf(grow[2 * H + j]);
    const float og = sigmoidf_(grow[3 * H + j]);
    const float c = fg * c_in[i] + ig * gg;
    const float h = og * tanhf(c);
    grow[j] = ig;
    grow[H + j] = fg;
    grow[2 * H + j] = gg;
    grow[3 * H + j] = og;
    c_out[i] = c;
    h_out[i] = h;
    if (nd_next != nullptr) {
      const float nd = nd_next[b];
      h_in_next[i] = h * nd;
      c_in_next[i] = c * nd;
    }
  }
}

extern "C" __global__ void lstm_cell_bwd_kernel(
    const float* __restrict__ gates,    // [B,4H] activated (from fwd)
    const float* __restrict__ c_in,     // [B,H] cs_in[t]
    const float* __restrict__ c_out,    // [B,H] cs_out[t]
    const float* __restrict__ d_hs_t,   // [B,H] upstream grad of hs[t]
    const float* __restrict__ g,        // [B,H] raw dgates[t+1] @ W_hh, or
                                        //       d_hT at t = T-1
    const float* __restrict__ nd_next,  // [B] notdone[t+1], null at t = T-1
    const float* __restrict__ nd_t,     // [B] notdone[t]
    float* dc_carry,                    // [B,H] in: dc from t+1; out: for t-1
    float* __restrict__ dgates,         // [B,4H] out: preact grads
    long B, long H) {
  const long total = B * H;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    const long b = i / H, j = i % H;
    const float* grow = gates + b * 4 * H;
    float* dgrow = dgates + b * 4 * H;
    const float ig = grow[j];
    const float fg = grow[H + j];
    const float gg = grow[2 * H + j];
    const float og = grow[3 * H + j];
    const float tc = tanhf(c_out[i]);
    const float gm = (nd_next != nullptr) ? g[i] * nd_next[b] : g[i];
    const float dh = d_hs_t[i] + gm;
    // tc * tc is rounded on its own (not contracted into an fma with the
    // subtraction), as in the kernel this one replaced: gradients stay
    // bit-equal with it
    float tc2;
    {
#pragma clang fp contract(off)
      tc2 = tc * tc;
    }
    const float dc = dc_carry[i] + dh * og * (1.f - tc2);
    dgrow[j] = dc * gg * ig * (1.f - ig);
    dgrow[H + j] = dc * c_in[i] * fg * (1.f - fg);
    dgrow[2 * H + j] = dc * ig * (1.f - gg * gg);
    dgrow[3 * H + j] = dh * tc * og * (1.f - og);
    dc_carry[i] = (dc * fg) * nd_t[b];
  }
}

void lstm_launch_mask_rows(const float* a, const float* b, const float* notdone,
                           float* a_out, float* b_out, long B, long H,
                           hipStream_t stream) {
  hipLaunchKernelGGL(lstm_mask_rows_kernel,
                     dim3(grid_1d(B * H, LSTM_CELL_BLOCK)),
                     dim3(LSTM_CELL_BLOCK), 0, stream, a, b, notdone, a_out,
                     b_out, B, H);
}

void lstm_launch_cell_fwd(float* gates, const float* c_in, float* h_out,
                          float* c_out, const float* nd_next, float* h_in_next,
                          float* c_in_next, long B, long H,
                          hipStream_t stream) {
  hipLaunchKernelGGL(lstm_cell_fwd_kernel,
                     dim3(grid_1d(B * H, LSTM_CELL_BLOCK)),
                     dim3(LSTM_CELL_BLOCK), 0, stream, gates, c_in, h_out,
                     c_out, nd_next, h_in_next, c_in_next, B, H);
}

void lstm_launch_cell_bwd(const float* gates, const float* c_in,
                          const float* c_out, const float* d_hs_t,
                          const float* g, const float* nd_next,
                          const float* nd_t, float* dc_carry, float* dgates,
                          long B, long H, hipStream_t stream) {
  hipLaunchKernelGGL(lstm_cell_bwd_kernel,
                     dim3(grid_1d(B * H, LSTM_CELL_BLOCK)),
                     dim3(LSTM_CELL_BLOCK), 0, stream, gates, c_in, c_out,
                     d_hs_t, g, nd_next, nd_t, dc_carry, dgates, B, H);
}

extern "C" int lstm_mask_rows(const float* a, const float* b,
                              const float* notdone, float* a_out,
                              float* b_out, long B, long H,
                              hipStream_t stream) {
  if (B <= 0 || H <= 0) return 0;
  lstm_launch_mask_rows(a, b, notdone, a_out, b_out, B, H, stream);
  CHECK_LAUNCH();
  return 0;
}

extern "C" int lstm_cell_fwd(float* gates, const float* c_in, float* h_out,
                             float* c_out, const float* nd_next,
                             float* h_in_next, float* c_in_next, long B,
                             long H, hipStream_t stream) {
  if (B <= 0 || H <= 0) return 0;
  lstm_launch_cell_fwd(gates, c_in, h_out, c_out, nd_next, h_in_next,
                       c_in_next, B, H, stream);
  CHECK_LAUNCH();
  return 0;
}

extern "C" int lstm_cell_bwd(const float* gates, const float* c_in,
                             const float* c_out, const float* d_hs_t,
                             const float* g, const float* nd_next,
                             const float* nd_t, float* dc_carry,
                             float* dgates, long B, long H,
                             hipStream_t stream) {
  if (B <= 0 || H <= 0) return 0;
  lstm_launch_cell_bwd(gates, c_in, c_out, d_hs_t, g, nd_next, nd_t,
                       dc_carry, dgates, B, H, stream);
  CHECK_LAUNCH();
  return 0;
}
