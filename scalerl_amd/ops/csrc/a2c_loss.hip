// Fused GAE(lambda) actor-critic (A2C) loss for the A3C-GPU learner: the GAE
// scan, the policy-gradient / value / entropy losses and their analytic
// gradients in one launch.  Entered through gae_scan (scans.hip) when logits
// are given; replaces gae_kernel + log_softmax/gather/exp/3 means/mse_loss
// and their autograd backward.
//
//   delta_t = r_t + d_t*V_{t+1} - V_t              (V_T = bootstrap)
//   adv_t   = delta_t + d_t*lam*adv_{t+1}          ret_t = adv_t + V_t
//   pg      = -mean(logp_t(a_t) * adv_t)
//   value   = 0.5 * mean((V_t - ret_t)^2)          (= 0.5 * mean(adv_t^2))
//   entropy = -mean(sum_j p_j logp_j)
//   total   = pg + value_coef*value - entropy_coef*entropy
//   dtotal/dlogit_j = [-adv*(1{j=a} - p_j) + entropy_coef*p_j*(logp_j - h)]/N
//   dtotal/dV_t     = -value_coef*adv_t/N          h = sum_k p_k logp_k, N = T*B
// adv and ret are constants of the loss (detached); the bootstrap gets no
// gradient.
//
// Work split.  blockIdx.x owns A2C_TILE_B = 8 consecutive batch columns,
// blockIdx.y a chunk [t0,t1) of time steps.  The rows (t, b0..b0+7) of one
// step are contiguous in memory (8*A floats), so the logits loads and the
// gradient stores of a block coalesce; 8 columns keep the scan's LDS at
// 3*T*8 floats, which fits T <= A2C_MAX_T = 512 into 48 KiB, and leave
// B/8 * T/chunk blocks to fill the device even at B = 32.  The chunk is at
// least one full pass of the block over its rows and grows until the grid
// has at most 2048 blocks.
//
// Scan.  rewards, discounts and values of the tile are staged into LDS from
// step t0 to T-1 (adv_t0 depends on everything after it, so a block repeats
// the scan of the later chunks: T*8 LDS steps at most, against the row work it
// parallelises).  One thread per column scans backwards out of LDS and writes
// adv over the reward it has consumed; adv stays there for the loss phase.
// Then the block writes advantages/returns (where asked for) and grad_values
// of its own rows, one row per thread, coalesced.
//
// Rows across lanes, two layouts picked by the launcher from A:
//   A <= 32  a2c_loss_packed_kernel<W>: W = next power of two >= max(A,2)
//            lanes hold one row, 64/W rows share a wave; max/sum butterflies
//            (__shfl_xor) stay inside the W-lane sub-group, the taken
//            log-probability is one __shfl.  A 6-action row idles 2 of 8
//            lanes, not 58 of 64.
//   A > 32   a2c_loss_wide_kernel<RESIDENT>: one wave per row, lanes stride
//            over the actions.  Up to A2C_REG_K = 8 floats per lane (A <= 512)
//            the row is read once and kept in registers; above that the row
//            is re-read per pass (max, sums, gradient).  No cap on A.
// The entropy term uses h = u/s - log s with s = sum e_k, u = sum e_k*(x_k -
// max), e_k = exp(x_k - max): one reduction pass gives both s and h.
// expf/logf, not the fast intrinsics, hold the project's loss tolerances.
//
// grad_logits, grad_values, advantages and returns are written completely and
// are bitwise reproducible (fixed butterfly order, no atomics).  loss_out[3]
// = (pg, value, entropy) means, one atomicAdd per component and block into a
// buffer the caller zeroes; not bitwise reproducible.  An action outside
// [0,A) never indexes memory: that row's logits gradient and the pg loss
// become NaN.  There is no matrix product in this loss, so no MFMA.

#include <climits>

#include "a2c_loss.h"
#include "common.h"

#define A2C_BLOCK 256
#define A2C_REG_K 8

struct A2CArgs {
  const float* rewards;    // [T,B]
  const float* values;     // [T,B]
  const float* bootstrap;  // [B]
  const float* discounts;  // [T,B]
  const float* logits;     // [T,B,A]
  const long* actions;     // [T,B]
  float* advantages;       // [T,B] out or null
  float* returns;          // [T,B] out or null
  float* grad_logits;      // [T,B,A] out
  float* grad_values;      // [T,B] out
  float* loss_out;         // [3] atomic
  float lam, value_coef, entropy_coef, inv_n;
  int T, B, A, chunk;
};

struct A2CTile {
  int t0, b0, kc, nrows;  // first step, first column, columns, own rows
  const float* adv_s;     // LDS, [(t - t0)*kc + c]
  // global row index t*B + b of the tile's local row i
  __device__ __forceinline__ long row(int i, int B) const {
    const int tt = i / kc;
    return (long)(t0 + tt) * B + b0 + (i - tt * kc);
  }
};

template <int W>
__device__ __forceinline__ float group_all_max(float v) {
  #pragma unroll
  for (int off = W / 2; off > 0; off >>= 1)
    v = fmaxf(v, __shfl_xor(v, off, W));
  return v;
}

// a + b == b + a bit for bit, so every lane of the group ends with the same sum
template <int W>
__device__ __forceinline__ float group_all_sum(float v) {
  #pragma unroll
  for (int off = W / 2; off > 0; off >>= 1)
    v += __shfl_xor(v, off, W);
  return v;
}

// Stage, scan, and write the per-row value outputs of the block's own rows.
// Returns this thread's share of sum 0.5*adv^2.
__device__ __forceinline__ float a2c_scan_tile(const A2CArgs& p, float* lds,
                                               A2CTile& tile) {
  const int t0 = blockIdx.y * p.chunk;
  const int t1 = min(p.T, t0 + p.chunk);
  const int b0 = blockIdx.x * A2C_TILE_B;
  const int kc = min(A2C_TILE_B, p.B - b0);
  const int n = (p.T - t0) * kc;
  float* r_s = lds;
  float* d_s = lds + n;
  float* v_s = lds + 2 * n;
  tile.t0 = t0;
  tile.b0 = b0;
  tile.kc = kc;
  tile.nrows = (t1 - t0) * kc;
  tile.adv_s = r_s;
  for (int i = threadIdx.x; i < n; i += A2C_BLOCK) {
    const long g = tile.row(i, p.B);
    r_s[i] = p.rewards[g];
    d_s[i] = p.discounts[g];
    v_s[i] = p.values[g];
  }
  __syncthreads();
  if (threadIdx.x < kc) {
    const int c = threadIdx.x;
    float adv = 0.f;
    float v_tp1 = p.bootstrap[b0 + c];
    for (int i = n - kc + c; i >= 0; i -= kc) {  // t = T-1 .. t0
      const float v = v_s[i];
      const float d = d_s[i];
      const float delta = r_s[i] + d * v_tp1 - v;
      adv = delta + d * p.lam * adv;
      r_s[i] = adv;
      v_tp1 = v;
    }
  }
  __syncthreads();
  float val_acc = 0.f;
  for (int i = threadIdx.x; i < tile.nrows; i += A2C_BLOCK) {
    const long g = tile.row(i, p.B);
    const float adv = r_s[i];
    if (p.advantages) p.advantages[g] = adv;
    if (p.returns) p.returns[g] = adv + v_s[i];
    p.grad_values[g] = -p.value_coef * adv * p.inv_n;
    val_acc += 0.5f * adv * adv;
  }
  return val_acc;
}

__device__ __forceinline__ void a2c_finish(const A2CArgs& p, float pg_acc,
                                           float val_acc, float ent_acc,
                                           float (*red)[16]) {
  const float pg = block_reduce_sum(pg_acc, red[0]);
  const float val = block_reduce_sum(val_acc, red[1]);
  const float ent = block_reduce_sum(ent_acc, red[2]);
  if (threadIdx.x == 0) {
    atomicAdd(p.loss_out + 0, pg * p.inv_n);
    atomicAdd(p.loss_out + 1, val * p.inv_n);
    atomicAdd(p.loss_out + 2, ent * p.inv_n);
  }
}

// d total / d logit_j times N, for one element
__device__ __forceinline__ float a2c_grad(float pj, float logp, float h,
                                          float adv, bool taken,
                                          float entropy_coef) {
  return -adv * ((taken ? 1.f : 0.f) - pj) + entropy_coef * pj * (logp - h);
}

template <int W>
__global__ void __launch_bounds__(A2C_BLOCK) a2c_loss_packed_kernel(A2CArgs p) {
  extern __shared__ __attribute__((aligned(16))) float a2c_lds[];
  __shared__ float red[3][16];
  A2CTile tile;
  const float val_acc = a2c_scan_tile(p, a2c_lds, tile);

  const int j = threadIdx.x & (W - 1);
  const int sub = threadIdx.x / W;
  const bool live = j < p.A;
  float pg_acc = 0.f, ent_acc = 0.f;
  // a W-lane sub-group enters an iteration whole, so the butterflies below
  // only ever read lanes that are active
  for (int i = sub; i < tile.nrows; i += A2C_BLOCK / W) {
    const long g = tile.row(i, p.B);
    long a = p.actions[g];
    const bool ok = a >= 0 && a < p.A;
    if (!ok) a = 0;
    const float adv = ok ? tile.adv_s[i] : NAN;
    const float x = live ? p.logits[g * p.A + j] : -INFINITY;
    const float mx = group_all_max<W>(x);
    const float xm = x - mx;
    const float e = live ? expf(xm) : 0.f;
    const float s = group_all_sum<W>(e);
    const float u = group_all_sum<W>(live ? e * xm : 0.f);
    const float ls = logf(s);
    const float h = u / s - ls;  // sum_k p_k logp_k
    const float la = __shfl(xm - ls, (int)a, W);
    if (live)
      p.grad_logits[g * p.A + j] =
          a2c_grad(e / s, xm - ls, h, adv, j == a, p.entropy_coef) * p.inv_n;
    if (j == 0) {
      pg_acc -= la * adv;
      ent_acc -= h;
    }
  }
  a2c_finish(p, pg_acc, val_acc, ent_acc, red);
}

template <bool RESIDENT>
__global__ void __launch_bounds__(A2C_BLOCK) a2c_loss_wide_kernel(A2CArgs p) {
  extern __shared__ __attribute__((aligned(16))) float a2c_lds[];
  __shared__ float red[3][16];
  A2CTile tile;
  const float val_acc = a2c_scan_tile(p, a2c_lds, tile);

  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x >> 6;
  const int A = p.A;
  float pg_acc = 0.f, ent_acc = 0.f;
  for (int i = wid; i < tile.nrows; i += A2C_BLOCK / WAVE) {
    const long g = tile.row(i, p.B);
    long a = p.actions[g];
    const bool ok = a >= 0 && a < A;
    if (!ok) a = 0;
    const float adv = ok ? tile.adv_s[i] : NAN;
    const float* row = p.logits + g * A;
    float* grow = p.grad_logits + g * A;
    float x[A2C_REG_K];
    float mx = -INFINITY;
    if (RESIDENT) {  // A <= A2C_REG_K * WAVE
      #pragma unroll
      for (int k = 0; k < A2C_REG_K; ++k) {
        const int jj = lane + k * WAVE;
        x[k] = jj < A ? row[jj] : -INFINITY;
        mx = fmaxf(mx, x[k]);
      }
    } else {
      for (int jj = lane; jj < A; jj += WAVE) mx = fmaxf(mx, row[jj]);
    }
    mx = group_all_max<WAVE>(mx);
    float s = 0.f, u = 0.f;
    if (RESIDENT) {
      #pragma unroll
      for (int k = 0; k < A2C_REG_K; ++k) {
        if (lane + k * WAVE < A) {
          const float xm = x[k] - mx;
          const float e = expf(xm);
          s += e;
          u += e * xm;
        }
      }
    } else {
      for (int jj = lane; jj < A; jj += WAVE) {
        const float xm = row[jj] - mx;
        const float e = expf(xm);
        s += e;
        u += e * xm;
      }
    }
    s = group_all_sum<WAVE>(s);
    u = group_all_sum<WAVE>(u);
    const float ls = logf(s);
    const float h = u / s - ls;
    const float la = row[a] - mx - ls;  // one broadcast load
    if (RESIDENT) {
      #pragma unroll
      for (int k = 0; k < A2C_REG_K; ++k) {
        const int jj = lane + k * WAVE;
        if (jj < A) {
          const float xm = x[k] - mx;
          grow[jj] = a2c_grad(expf(xm) / s, xm - ls, h, adv, jj == a,
                              p.entropy_coef) * p.inv_n;
        }
      }
    } else {
      for (int jj = lane; jj < A; jj += WAVE) {
        const float xm = row[jj] - mx;
        grow[jj] = a2c_grad(expf(xm) / s, xm - ls, h, adv, jj == a,
                            p.entropy_coef) * p.inv_n;
      }
    }
    if (lane == 0) {
      pg_acc -= la * adv;
      ent_acc -= h;
    }
  }
  a2c_finish(p, pg_acc, val_acc, ent_acc, red);
}

int a2c_loss_launch(const float* rewards, const float* values,
                    const float* bootstrap, const float* discounts, float lam,
                    long T, long B, float* advantages, float* returns,
                    const float* logits, const long* actions, long A,
                    float value_coef, float entropy_coef, float* grad_logits,
                    float* grad_values, float* loss_out, hipStream_t stream) {
  if (T < 1 || B < 1 || A < 1 || B > INT_MAX || A > INT_MAX || !actions ||
      !grad_logits || !grad_values || !loss_out)
    return (int)hipErrorInvalidValue;
  if (T > A2C_MAX_T) return -3;
  int W = 2;
  while (W < A && W < WAVE) W <<= 1;
  const long rows_per_pass = A <= 32 ? A2C_BLOCK / W : A2C_BLOCK / WAVE;
  const long nbx = (B + A2C_TILE_B - 1) / A2C_TILE_B;
  long chunk = rows_per_pass / A2C_TILE_B;           // one full pass of rows,
  const long fit = (T * nbx + 2047) / 2048;          // at most 2048 blocks
  if (chunk < fit) chunk = fit;
  if (chunk < 1) chunk = 1;
  if (chunk > T) chunk = T;

  A2CArgs p;
  p.rewards = rewards;
  p.values = values;
  p.bootstrap = bootstrap;
  p.discounts = discounts;
  p.logits = logits;
  p.actions = actions;
  p.advantages = advantages;
  p.returns = returns;
  p.grad_logits = grad_logits;
  p.grad_values = grad_values;
  p.loss_out = loss_out;
  p.lam = lam;
  p.value_coef = value_coef;
  p.entropy_coef = entropy_coef;
  p.inv_n = 1.f / ((float)T * (float)B);
  p.T = (int)T;
  p.B = (int)B;
  p.A = (int)A;
  p.chunk = (int)chunk;

  const dim3 grid((unsigned)nbx, (unsigned)((T + chunk - 1) / chunk));
  const dim3 block(A2C_BLOCK);
  const size_t lds = (size_t)3 * T * A2C_TILE_B * sizeof(float);
  if (A > A2C_REG_K * WAVE)
    hipLaunchKernelGGL(a2c_loss_wide_kernel<false>, grid, block, lds, stream, p);
  else if (A > 32)
    hipLaunchKernelGGL(a2c_loss_wide_kernel<true>, grid, block, lds, stream, p);
  else if (W == 2)
    hipLaunchKernelGGL(a2c_loss_packed_kernel<2>, grid, block, lds, stream, p);
  else if (W == 4)
    hipLaunchKernelGGL(a2c_loss_packed_kernel<4>, grid, block, lds, stream, p);
  else if (W == 8)
    hipLaunchKernelGGL(a2c_loss_packed_kernel<8>, grid, block, lds, stream, p);
  else if (W == 16)
    hipLaunchKernelGGL(a2c_loss_packed_kernel<16>, grid, block, lds, stream, p);
  else
    hipLaunchKernelGGL(a2c_loss_packed_kernel<32>, grid, block, lds, stream, p);
  CHECK_LAUNCH();
  return 0;
}
