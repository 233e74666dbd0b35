// Fused DQN TD loss: double/vanilla DQN target + Huber/MSE + PER IS-weights
// + |TD| priorities + analytic gradient w.r.t. the online Q row — one launch.
//
// Reference semantics (reimplemented):
//   dqn_agent.py:155-171  (double-DQN target, MSE),
//   apex/worker.py:134-161 (PER IS weights (1/(N*P))^beta / max_w, priority
//                           update from |TD|).
//
// IS weights are computed in-kernel from raw priorities + (p_total, p_min)
// device scalars so sampling->loss needs no host round-trip:
//   P_i = prio_i / p_total;  w_i = (N * P_i)^-beta / (N * p_min/p_total)^-beta.
// `prios` may be nullptr -> uniform weights (plain DQN).

#include "common.h"

extern "C" __global__ void __launch_bounds__(256)
td_loss_kernel(const float* __restrict__ q,            // [B,A] online Q(s)
               const float* __restrict__ q_next_online,// [B,A] online Q(s') (double) or null
               const float* __restrict__ q_next_target,// [B,A] target Q(s')
               const long* __restrict__ actions,       // [B]
               const float* __restrict__ rewards,      // [B] (n-step folded)
               const float* __restrict__ discounts,    // [B] gamma^m*(1-d)
               const float* __restrict__ prios,        // [B] or null
               const float* __restrict__ p_total,      // [1] or null
               const float* __restrict__ p_min,        // [1] or null
               float beta, long replay_size,
               int B, int A, int huber, float huber_delta,
               float* __restrict__ grad_q,             // [B,A] out (zeroed by caller)
               float* __restrict__ td_abs,             // [B] out (new priorities)
               float* __restrict__ loss_out) {         // [1] out (atomic, mean)
  __shared__ float scratch[16];
  float loss_acc = 0.f;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < B;
       i += gridDim.x * blockDim.x) {
    const float* qrow = q + (long)i * A;
    const long a = actions[i];
    // target: r + gamma * Q_target(s', a*)
    int astar = 0;
    if (q_next_online) {  // double DQN: argmax over online net
      float best = -1e30f;
      for (int j = 0; j < A; ++j) {
        const float v = q_next_online[(long)i * A + j];
        if (v > best) { best = v; astar = j; }
      }
    } else {  // vanilla: argmax over target net
      float best = -1e30f;
      for (int j = 0; j < A; ++j) {
        const float v = q_next_target[(long)i * A + j];
        if (v > best) { best = v; astar = j; }
      }
    }
    const float target = rewards[i] + discounts[i] * q_next_target[(long)i * A + astar];
    const float td = qrow[a] - target;
    td_abs[i] = fabsf(td);

    float w = 1.f;
    if (prios) {
      const float pt = *p_total;
      const float pm = *p_min;
      const float w_i = __powf((float)replay_size * (prios[i] / pt), -beta);
      const float w_max = __powf((float)replay_size * (pm / pt), -beta);
      w = w_i / w_max;
    }
    float l, dldtd;
    if (huber) {
      const float atd = fabsf(td);
      if (atd <= huber_delta) { l = 0.5f * td * td; dldtd = td; }
      else { l = huber_delta * (atd - 0.5f * huber_delta); dldtd = huber_delta * ((td > 0) ? 1.f : -1.f); }
    } else {
      l = td * td;       // MSE as the reference writes it (dqn_agent.py:171)
      dldtd = 2.f * td;
    }
    loss_acc += w * l / (float)B;
    grad_q[(long)i * A + a] = w * dldtd / (float)B;
  }
  const float tot = block_reduce_sum(loss_acc, scratch);
  if (threadIdx.x == 0) atomicAdd(loss_out, tot);
}

// ---------------------------------------------------------------------------
// Fused C51 categorical TD loss (Bellemare et al. 2017, alg. 1): greedy next
// action from expected Q, target softmax, categorical projection, cross
// entropy against the online row, PER IS weights, per-sample priorities and
// the analytic gradient w.r.t. the online logits — one launch.
//
// Inputs are raw logits [B,A,N]; z_k = v_min + k*dz, dz = (v_max-v_min)/(N-1).
// One 64-lane wave per sample, C51_WAVES waves per block, blocks grid-stride
// over samples, lanes stride over atoms (N below, equal to or above 64).
//
// The projection is evaluated in gather form, without atomics:
//   b_j = (clamp(r + d*z_j, v_min, v_max) - v_min) / dz
//   m_k = sum_j p_j * max(0, 1 - |b_j - k|)
// which is the lo/hi scatter of the composed reference written per output
// atom; it is continuous in b, so it does not depend on where a floor lands.
// exp(x_j - max) and b_j of the target row sit in a per-wave LDS slice and
// are read back as broadcasts: N*ceil(N/64) FMAs per lane.
//
// grad_logits is written completely by the kernel (the taken action's row
// and zeros for every other action): the caller does NOT zero it.  kl and
// grad_logits are bitwise reproducible; loss_out is one atomicAdd per block
// into a buffer the caller zeroes, like td_loss_kernel.
//
// An action outside [0,A) never indexes memory: that sample's kl, gradient
// row 0 and the loss become NaN.

#define C51_WAVES 4
#define C51_MAX_ATOMS 1024  // LDS: (16 + 4*3*1024) floats = 49216 B

__device__ __forceinline__ float c51_row_max(const float* __restrict__ row,
                                             int N, int lane) {
  float m = -INFINITY;
  for (int k = lane; k < N; k += WAVE) m = fmaxf(m, row[k]);
  return wave_all_max(m);
}

extern "C" __global__ void __launch_bounds__(64 * C51_WAVES)
c51_loss_kernel(const float* __restrict__ logits,      // [B,A,N] online(s)
                const float* __restrict__ next_online, // [B,A,N] online(s') (double) or null
                const float* __restrict__ next_target, // [B,A,N] target(s')
                const long* __restrict__ actions,      // [B]
                const float* __restrict__ rewards,     // [B] (n-step folded)
                const float* __restrict__ discounts,   // [B] gamma^m*(1-d)
                const float* __restrict__ prios,       // [B] or null
                const float* __restrict__ p_total,     // [1] or null
                const float* __restrict__ p_min,       // [1] or null
                float beta, long replay_size,
                int B, int A, int N, float v_min, float v_max,
                float* __restrict__ grad_logits,       // [B,A,N] out (fully written)
                float* __restrict__ kl_out,            // [B] out (new priorities)
                float* __restrict__ loss_out) {        // [1] out (atomic, mean)
  // all LDS is dynamic: 16 floats for block_reduce_sum, then per wave three
  // slices of N floats (exp(x-max) of the target row, b, projected m)
  extern __shared__ __attribute__((aligned(16))) float c51_lds[];
  float* scratch = c51_lds;
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x >> 6;
  float* e_s = c51_lds + 16 + (long)wid * 3 * N;
  float* b_s = e_s + N;
  float* m_s = b_s + N;
  const float dz = (v_max - v_min) / (float)(N - 1);
  const long row_elems = (long)A * N;

  float loss_acc = 0.f;
  // the trip count depends on blockIdx only, so every wave of the block
  // reaches the barrier below the same number of times
  for (long base = (long)blockIdx.x * C51_WAVES; base < B;
       base += (long)gridDim.x * C51_WAVES) {
    const long i = base + wid;
    const bool active = i < B;  // wave-uniform
    float inv_s = 0.f;
    if (active) {
      // 1. greedy next action: first argmax_j of Q_j = sum_k softmax_k * z_k
      const float* sel = (next_online ? next_online : next_target)
                         + i * row_elems;
      int astar = 0;
      float best = -INFINITY;
      for (int j = 0; j < A; ++j) {
        const float* row = sel + (long)j * N;
        const float mx = c51_row_max(row, N, lane);
        float s = 0.f, sz = 0.f;
        for (int k = lane; k < N; k += WAVE) {
          const float e = expf(row[k] - mx);
          s += e;
          sz += e * (v_min + (float)k * dz);
        }
        const float q = wave_all_sum(sz) / wave_all_sum(s);
        if (q > best) { best = q; astar = j; }
      }
      // 2. target distribution (unnormalised) and 3. b_j, into the slice
      const float* trow = next_target + i * row_elems + (long)astar * N;
      const float mx = c51_row_max(trow, N, lane);
      const float r = rewards[i];
      const float d = discounts[i];
      float s = 0.f;
      for (int k = lane; k < N; k += WAVE) {
        const float e = expf(trow[k] - mx);
        s += e;
        e_s[k] = e;
        const float tz = fminf(fmaxf(r + d * (v_min + (float)k * dz), v_min),
                               v_max);
        b_s[k] = (tz - v_min) / dz;
      }
      inv_s = 1.f / wave_all_sum(s);
    }
    __syncthreads();  // slice written by all lanes, read by all lanes
    if (active) {
      long a = actions[i];
      const bool ok = a >= 0 && a < A;
      if (!ok) a = 0;
      // 4. online row: log-softmax, projection, cross entropy
      const float* orow = logits + i * row_elems + a * N;
      const float mx = c51_row_max(orow, N, lane);
      float se = 0.f;
      for (int k = lane; k < N; k += WAVE) se += expf(orow[k] - mx);
      const float lse = mx + logf(wave_all_sum(se));
      float kl = 0.f, msum = 0.f;
      for (int k = lane; k < N; k += WAVE) {
        const float fk = (float)k;
        float acc = 0.f;
        for (int j = 0; j < N; ++j)
          acc += e_s[j] * fmaxf(0.f, 1.f - fabsf(b_s[j] - fk));
        const float m = acc * inv_s;
        m_s[k] = m;  // read back below by this same lane
        msum += m;
        kl -= m * (orow[k] - lse);
      }
      kl = wave_all_sum(kl);
      msum = wave_all_sum(msum);
      // 5. IS weight, as td_loss_kernel computes it
      float w = 1.f;
      if (prios) {
        const float pt = *p_total;
        const float pm = *p_min;
        const float w_i = __powf((float)replay_size * (prios[i] / pt), -beta);
        const float w_max = __powf((float)replay_size * (pm / pt), -beta);
        w = w_i / w_max;
      }
      if (!ok) { w = NAN; kl = NAN; }
      if (lane == 0) {
        kl_out[i] = kl;
        loss_acc += w * kl / (float)B;
      }
      // 6. gradient: d/dlogit_k of -sum m*logp = softmax_k * sum(m) - m_k
      const float scale = w / (float)B;
      float* g = grad_logits + i * row_elems;
      float* grow = g + a * N;
      for (int k = lane; k < N; k += WAVE)
        grow[k] = scale * (expf(orow[k] - lse) * msum - m_s[k]);
      for (long idx = lane; idx < row_elems; idx += WAVE)
        if (idx / N != a) g[idx] = 0.f;
    }
  }
  const float tot = block_reduce_sum(loss_acc, scratch);
  if (threadIdx.x == 0) atomicAdd(loss_out, tot);
}

// atoms == 0: scalar TD loss, q* are [B,A].  atoms >= 2: C51 categorical
// loss, q* are logits [B,A,atoms], td_abs receives the per-sample cross
// entropy, huber/huber_delta are ignored and grad_q need not be zeroed.
// Returns -4 for an atom count outside 2..C51_MAX_ATOMS.
extern "C" int fused_td_loss(
    const float* q, const float* q_next_online, const float* q_next_target,
    const long* actions, const float* rewards, const float* discounts,
    const float* prios, const float* p_total, const float* p_min,
    float beta, long replay_size, long B, long A, int huber,
    float huber_delta, long atoms, float v_min, float v_max, float* grad_q,
    float* td_abs, float* loss_out, hipStream_t stream) {
  if (atoms != 0) {
    if (atoms < 2 || atoms > C51_MAX_ATOMS) return -4;
    long grid = (B + C51_WAVES - 1) / C51_WAVES;
    if (grid > 32768) grid = 32768;
    const size_t lds = (16 + (size_t)C51_WAVES * 3 * atoms) * sizeof(float);
    hipLaunchKernelGGL(c51_loss_kernel, dim3((int)grid),
                       dim3(64 * C51_WAVES), lds, stream, q, q_next_online,
                       q_next_target, actions, rewards, discounts, prios,
                       p_total, p_min, beta, replay_size, (int)B, (int)A,
                       (int)atoms, v_min, v_max, grad_q, td_abs, loss_out);
    CHECK_LAUNCH();
    return 0;
  }
  const int block = 256;
  hipLaunchKernelGGL(td_loss_kernel, dim3(grid_1d(B, block)), dim3(block), 0,
                     stream, q, q_next_online, q_next_target, actions, rewards,
                     discounts, prios, p_total, p_min, beta, replay_size,
                     (int)B, (int)A, huber, huber_delta, grad_q, td_abs,
                     loss_out);
  CHECK_LAUNCH();
  return 0;
}
