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

// ---------------------------------------------------------------------------
// Fused QR-DQN quantile-Huber loss (Dabney et al. 2018, alg. 1): greedy next
// action from the mean of the quantiles, Bellman targets T_j, the N x N
// pairwise quantile-Huber terms, PER IS weights, per-sample priorities and the
// analytic gradient w.r.t. the online quantiles — one launch.
//
// Inputs are raw quantile values [B,A,N]; tau_i = (i + 0.5)/N, kappa > 0.
//   u_ij = T_j - theta_i,  m = min(|u|, kappa)
//   L_kappa(u) = m * (|u| - m/2)       (u^2/2 inside kappa, linear outside)
//   l_b = sum_i 1/N sum_j |tau_i - 1{u_ij<0}| * L_kappa(u_ij) / kappa
//   dl_b/dtheta_i = -1/N sum_j |tau_i - 1{u_ij<0}| * clamp(u_ij,-k,k) / kappa
//
// The per-sample work is N^2 pair terms without a transcendental (40 000 at
// N = 200), and DQN batches are 32..64 samples, so a wave per sample as in
// c51_loss_kernel would leave the chip idle: here one 256-thread block works
// on one sample and blocks grid-stride over B.
//   1. waves take actions wid, wid+4, ..: row sum with lanes striding k, one
//      candidate per wave in LDS, every thread picks the same first argmax;
//   2. T_j = r + d*next_target[a*,j] and theta_i of the taken row go to LDS;
//   3. lanes own online quantiles i = lane + 64c, waves own contiguous slices
//      of j; T_j is read as an LDS broadcast (one address per wave, no bank
//      conflict) and the two sums over j stay in registers;
//   4. the four waves' partials per i are added in wave order through LDS,
//      then the gradient row, zeros for the other rows, l_b by
//      block_reduce_sum.
// The pair term is no product of an i factor and a j factor, so matrix
// instructions do not apply.
//
// grad is written completely by the kernel; ql_out and grad are bitwise
// reproducible (no atomics); loss_out is one atomicAdd per block into a
// buffer the caller zeroes.  The grid is capped at QR_MAX_GRID blocks (four
// per CU), which also bounds the number of fp32 atomics the loss sums over.
//
// An action outside [0,A) never indexes memory: that sample's l, gradient
// row 0 and the loss become NaN.

#define QR_WAVES 4
#define QR_MAX_ATOMS C51_MAX_ATOMS  // LDS: (24 + 10*1024) floats = 41056 B
#define QR_MAX_GRID 1024

// one pair term: adds |tau - 1{u<0}| * L_kappa(u) to rho and
// |tau - 1{u<0}| * clamp(u, -kappa, kappa) to g (omt = 1 - tau)
__device__ __forceinline__ void qr_pair(float u, float kappa, float tau,
                                        float omt, float& rho, float& g) {
  const float au = fabsf(u);
  const float m = fminf(au, kappa);
  const float wq = u < 0.f ? omt : tau;
  rho += wq * (m * (au - 0.5f * m));
  g += wq * copysignf(m, u);
}

extern "C" __global__ void __launch_bounds__(64 * QR_WAVES)
qr_loss_kernel(const float* __restrict__ theta,       // [B,A,N] online(s)
               const float* __restrict__ next_online, // [B,A,N] online(s') (double) or null
               const float* __restrict__ next_target, // [B,A,N] target(s')
               const long* __restrict__ actions,      // [B]
               const float* __restrict__ rewards,     // [B] (n-step folded)
               const float* __restrict__ discounts,   // [B] gamma^m*(1-d)
               const float* __restrict__ prios,       // [B] or null
               const float* __restrict__ p_total,     // [1] or null
               const float* __restrict__ p_min,       // [1] or null
               float beta, long replay_size,
               int B, int A, int N, float kappa,
               float* __restrict__ grad,              // [B,A,N] out (fully written)
               float* __restrict__ ql_out,            // [B] out (new priorities)
               float* __restrict__ loss_out) {        // [1] out (atomic, mean)
  // all LDS is dynamic: 16 floats for block_reduce_sum, one greedy candidate
  // (row sum, action) per wave, T and theta (N each), then per wave the
  // partial loss and gradient sums per online quantile (2 * 4 * N)
  extern __shared__ __attribute__((aligned(16))) float qr_lds[];
  float* scratch = qr_lds;
  float* cand_v = qr_lds + 16;
  float* cand_a = cand_v + QR_WAVES;  // action index, stored as int bits
  float* T_s = cand_a + QR_WAVES;
  float* th_s = T_s + N;
  float* prho = th_s + N;
  float* pg = prho + (long)QR_WAVES * N;
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  const int wid = tid >> 6;
  const long row_elems = (long)A * N;
  const float inv_nk = 1.f / ((float)N * kappa);
  // this wave's slice of the target quantiles
  const int jper = (N + QR_WAVES - 1) / QR_WAVES;
  const int j0 = min(wid * jper, N);
  const int j1 = min(j0 + jper, N);

  float loss_acc = 0.f;  // thread 0 only
  // the trip count depends on blockIdx only, so every wave of the block
  // reaches every barrier below the same number of times
  for (long b = blockIdx.x; b < B; b += gridDim.x) {
    // 1. greedy next action: first argmax_a of sum_k sel[a,k] (the mean
    // times N, which orders the actions the same way)
    const float* sel = (next_online ? next_online : next_target)
                       + b * row_elems;
    float best = -INFINITY;
    int besta = wid < A ? wid : 0x7fffffff;
    for (int j = wid; j < A; j += QR_WAVES) {
      const float* row = sel + (long)j * N;
      float s = 0.f;
      for (int k = lane; k < N; k += WAVE) s += row[k];
      s = wave_all_sum(s);
      if (s > best) { best = s; besta = j; }
    }
    if (lane == 0) {
      cand_v[wid] = best;
      cand_a[wid] = __int_as_float(besta);
    }
    __syncthreads();
    int astar = 0;
    best = -INFINITY;
    #pragma unroll
    for (int w = 0; w < QR_WAVES; ++w) {
      const float v = cand_v[w];
      const int ca = __float_as_int(cand_a[w]);
      if (v > best || (v == best && ca < astar)) { best = v; astar = ca; }
    }
    long a = actions[b];
    const bool ok = a >= 0 && a < A;
    if (!ok) a = 0;
    // 2. targets and the taken row's online quantiles into LDS
    const float* trow = next_target + b * row_elems + (long)astar * N;
    const float* orow = theta + b * row_elems + a * N;
    const float r = rewards[b];
    const float d = discounts[b];
    for (int k = tid; k < N; k += 64 * QR_WAVES) {
      T_s[k] = r + d * trow[k];
      th_s[k] = orow[k];
    }
    __syncthreads();
    // 3. the N x N tile: this lane's i against this wave's j slice
    for (int i = lane; i < N; i += WAVE) {
      const float th = th_s[i];
      const float tau = ((float)i + 0.5f) / (float)N;
      const float omt = 1.f - tau;
      // four independent accumulators: shorter dependency chains, and a
      // quarter of the rounding a single running sum of like terms collects
      float rho[4] = {0.f, 0.f, 0.f, 0.f}, g[4] = {0.f, 0.f, 0.f, 0.f};
      int j = j0;
      for (; j + 4 <= j1; j += 4) {
        #pragma unroll
        for (int q = 0; q < 4; ++q)
          qr_pair(T_s[j + q] - th, kappa, tau, omt, rho[q], g[q]);
      }
      for (; j < j1; ++j)
        qr_pair(T_s[j] - th, kappa, tau, omt, rho[0], g[0]);
      prho[(long)wid * N + i] = (rho[0] + rho[1]) + (rho[2] + rho[3]);
      pg[(long)wid * N + i] = (g[0] + g[1]) + (g[2] + g[3]);
    }
    __syncthreads();
    // 4. IS weight, as td_loss_kernel computes it
    float w = 1.f;
    if (prios) {
      const float pt = *p_total;
      const float pm = *p_min;
      const float w_i = __powf((float)replay_size * (prios[b] / pt), -beta);
      const float w_max = __powf((float)replay_size * (pm / pt), -beta);
      w = w_i / w_max;
    }
    if (!ok) w = NAN;
    // partials in wave order, gradient row, zeros elsewhere, l_b
    const float gscale = -(w / (float)B) * inv_nk;
    float* gb = grad + b * row_elems;
    float* grow = gb + a * N;
    float lsum = 0.f;
    for (int i = tid; i < N; i += 64 * QR_WAVES) {
      float rs = prho[i], gs = pg[i];
      #pragma unroll
      for (int v = 1; v < QR_WAVES; ++v) {
        rs += prho[(long)v * N + i];
        gs += pg[(long)v * N + i];
      }
      lsum += rs;
      grow[i] = gscale * gs;
    }
    const long lo = a * N, hi = lo + N;
    for (long idx = tid; idx < row_elems; idx += 64 * QR_WAVES)
      if (idx < lo || idx >= hi) gb[idx] = 0.f;
    float l = block_reduce_sum(lsum, scratch) * inv_nk;  // thread 0
    if (tid == 0) {
      if (!ok) l = NAN;
      ql_out[b] = l;
      loss_acc += w * l / (float)B;
    }
  }
  if (tid == 0) atomicAdd(loss_out, loss_acc);
}

// atoms == 0: scalar TD loss, q* are [B,A], huber in {0,1}.  atoms >= 2: q*
// are [B,A,atoms], grad_q is written completely (it need not be zeroed) and
// td_abs receives the per-sample loss.  There huber == 2 selects the QR-DQN
// quantile-Huber loss on raw quantile values with huber_delta as kappa
// (v_min/v_max ignored); any other huber selects the C51 categorical loss on
// raw logits (huber/huber_delta ignored).  Returns -4 for an atom or quantile
// count outside 2..C51_MAX_ATOMS (= QR_MAX_ATOMS).
extern "C" int fused_td_loss(
    const float* q, const float* q_next_online, const float* q_next_target,
    const long* actions, const float* rewards, const float* discounts,
    const float* prios, const float* p_total, const float* p_min,
    float beta, long replay_size, long B, long A, int huber,
    float huber_delta, long atoms, float v_min, float v_max, float* grad_q,
    float* td_abs, float* loss_out, hipStream_t stream) {
  if (atoms != 0) {
    if (atoms < 2 || atoms > C51_MAX_ATOMS) return -4;
    if (huber == 2) {
      const long qgrid = B < QR_MAX_GRID ? B : QR_MAX_GRID;
      const size_t qlds = (24 + (size_t)10 * atoms) * sizeof(float);
      hipLaunchKernelGGL(qr_loss_kernel, dim3((int)qgrid),
                         dim3(64 * QR_WAVES), qlds, stream, q, q_next_online,
                         q_next_target, actions, rewards, discounts, prios,
                         p_total, p_min, beta, replay_size, (int)B, (int)A,
                         (int)atoms, huber_delta, grad_q, td_abs, loss_out);
      CHECK_LAUNCH();
      return 0;
    }
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
