// Whole-sequence masked-LSTM forward/backward driven from C++.
//
// The Python per-step loop costs ~20 ms of enqueue per learner iteration
// at B=128 (measured — profiles/README.md): 162 steps x {addmm +
// pointwise} x Python/launch overhead.  This moves the T-loop into C++:
// per step one rocBLAS SGEMM accumulating the recurrent product into the
// gate buffer (beta = 1) + one fused cell kernel (lstm.hip), all enqueued
// from native code on the caller's stream.  Numerics identical to the
// Python path (fp32 GEMM, fp32 pointwise, same masking order), so the same
// oracle tests apply.
//
// Layouts (row-major):
//   xg      [T,B,4H]  x @ W_ih^T + b  (in); overwritten with ACTIVATED
//                     gates (backward consumes them)
//   w_hh    [4H,H]
//   notdone [T,B]
//   h0, c0  [B,H]     initial state (unmasked)
//   hs      [T,B,H]   per-step outputs; hs[T-1] is the final h
//   hs_in   [T,B,H]   masked h entering each step (for dW_hh)
//   cs_in   [T,B,H]   masked c entering each step
//   cs_out  [T,B,H]   cell state after each step; cs_out[T-1] is the final c

#include "lstm_cell.h"

#include <rocblas/rocblas.h>

static rocblas_handle g_blas = nullptr;

static int ensure_blas(hipStream_t stream) {
  if (g_blas == nullptr) {
    if (rocblas_create_handle(&g_blas) != rocblas_status_success) return -10;
  }
  if (rocblas_set_stream(g_blas, stream) != rocblas_status_success)
    return -11;
  return 0;
}

// Row-major helper: C[m,n] = beta * C + A[m,k] @ B[n,k]^T
static int sgemm_nt(long m, long n, long k, const float* A, const float* Bm,
                    float beta, float* C) {
  const float one = 1.f;
  // column-major view: C_cm[n,m] = B_cm[k,n]^T x A_cm[k,m]
  return (rocblas_sgemm(g_blas, rocblas_operation_transpose,
                        rocblas_operation_none, (rocblas_int)n,
                        (rocblas_int)m, (rocblas_int)k, &one, Bm,
                        (rocblas_int)k, A, (rocblas_int)k, &beta, C,
                        (rocblas_int)n) == rocblas_status_success) ? 0 : -12;
}

// Row-major helper: C[m,n] = A[m,k] @ B[k,n]  (beta = 0)
static int sgemm_nn(long m, long n, long k, const float* A, const float* Bm,
                    float* C) {
  const float one = 1.f, zero = 0.f;
  // column-major view: C_cm[n,m] = B_cm[n,k] x A_cm[k,m]
  return (rocblas_sgemm(g_blas, rocblas_operation_none,
                        rocblas_operation_none, (rocblas_int)n,
                        (rocblas_int)m, (rocblas_int)k, &one, Bm,
                        (rocblas_int)n, A, (rocblas_int)k, &zero, C,
                        (rocblas_int)n) == rocblas_status_success) ? 0 : -12;
}

extern "C" int masked_lstm_seq_fwd(
    float* xg, const float* w_hh, const float* notdone, const float* h0,
    const float* c0, float* hs, float* hs_in, float* cs_in, float* cs_out,
    long T, long B, long H, hipStream_t stream) {
  if (T <= 0 || B <= 0 || H <= 0) return 0;
  int rc = ensure_blas(stream);
  if (rc) return rc;
  // step 0's masked state; later steps get theirs from the cell kernel
  lstm_launch_mask_rows(h0, c0, notdone, hs_in, cs_in, B, H, stream);
  for (long t = 0; t < T; ++t) {
    const long off = t * B * H;
    float* gates = xg + t * B * 4 * H;
    // gates[B,4H] += hs_in[t][B,H] @ w_hh[4H,H]^T
    rc = sgemm_nt(B, 4 * H, H, hs_in + off, w_hh, 1.f, gates);
    if (rc) return rc;
    const bool last = (t == T - 1);
    lstm_launch_cell_fwd(gates, cs_in + off, hs + off, cs_out + off,
                         last ? nullptr : notdone + (t + 1) * B,
                         last ? nullptr : hs_in + off + B * H,
                         last ? nullptr : cs_in + off + B * H, B, H, stream);
  }
  CHECK_LAUNCH();
  return 0;
}

extern "C" int masked_lstm_seq_bwd(
    const float* gates_act,   // [T,B,4H] (activated, from fwd)
    const float* cs_in, const float* cs_out,  // [T,B,H]
    const float* d_hs,        // [T,B,H] upstream
    const float* d_hT,        // [B,H] upstream of the final h (read only)
    const float* notdone,     // [T,B]
    const float* w_hh,        // [4H,H]
    float* dgates_all,        // [T,B,4H] out
    float* dh_carry,          // [B,H] out: d h_0 (post-mask); loop scratch
    float* dc_carry,          // [B,H] in: d c_T; out: d c_0 (post-mask)
    long T, long B, long H, hipStream_t stream) {
  if (T <= 0 || B <= 0 || H <= 0) return 0;
  int rc = ensure_blas(stream);
  if (rc) return rc;
  for (long t = T - 1; t >= 0; --t) {
    const long off = t * B * H;
    const bool last = (t == T - 1);
    float* dgates = dgates_all + t * B * 4 * H;
    lstm_launch_cell_bwd(gates_act + t * B * 4 * H, cs_in + off, cs_out + off,
                         d_hs + off, last ? d_hT : dh_carry,
                         last ? nullptr : notdone + (t + 1) * B,
                         notdone + t * B, dc_carry, dgates, B, H, stream);
    // raw dh_carry[B,H] = dgates[B,4H] @ w_hh[4H,H]; the next (earlier)
    // step's cell kernel applies notdone[t] to it (it consumed the old
    // carry above, so the overwrite is safe)
    rc = sgemm_nn(B, H, 4 * H, dgates, w_hh, dh_carry);
    if (rc) return rc;
  }
  // d h_0 = notdone[0] * (dgates[0] @ w_hh); d c_0 is the carry as it stands
  lstm_launch_mask_rows(dh_carry, nullptr, notdone, dh_carry, nullptr, B, H,
                        stream);
  CHECK_LAUNCH();
  return 0;
}
