// IMPALA (V-trace) and PPO clip losses for action spaces wider than the 32
// actions of impala_fused_loss_kernel / ppo_fused_loss_kernel.  Entered from
// those kernels' launchers when A > 32; inputs, outputs, reductions and loss
// definitions are theirs (vtrace_loss.hip, ppo_loss.hip), i.e. those of
// impala_loss_reference and ppo_loss_reference.
//
// Rows across lanes.  One wave owns a row of logits: lane l holds the actions
// l, l+64, ..., so global reads and the grad_logits writes coalesce.  A row is
// taken in chunks of PLW_REG_K*64 = 512 actions, 8 independent loads per lane
// in flight.  row_stats keeps a running (max, s = sum e, u = sum e*(x-max)),
// e = exp(x-max): the chunk's wave-wide max is folded in first and, when it
// raises the running max, s and u are rescaled once per chunk (the rescale is
// wave-uniform), so every row is read ONCE for its statistics whatever A is.
// For A <= 512 that is a single chunk: plain max, then sums, and the row is
// still in the lane's registers for the gradient pass.  Above 512 the
// gradient pass reads the row a second time (L2-resident: the wave has just
// streamed it).  lse = max + log s, sum p log p = u/s - log s.  The taken
// action's logit is caught by the lane that loads it and broadcast with one
// __shfl; an action outside [0,A) matches no lane and never indexes memory
// (that row's outputs become NaN).  A tail lane contributes -inf to the max,
// nothing to the sums, and writes nothing.  wave_all_max / wave_all_sum reduce
// in one fixed order, so grad_logits, grad_values and vs are bitwise
// reproducible.  expf/logf, not the fast intrinsics, as in a2c_loss.hip.
//
// impala_loss_wide_kernel<NR>.  A workgroup of 16 waves owns one batch
// column, its waves stride over t.
//   phase 1  per row: behaviour row -> lse and taken logit only (read once,
//            never kept); target row -> lse, sum p log p, taken logit.  Lane 0
//            writes the per-step LDS arrays rho, lse, plogp, logp(a), delta,
//            values, discounts, rewards.  With NR > 0 (A <= 512 and at most
//            NR rows per wave, NR = 2 or 6: T <= 96) the wave keeps its target
//            rows in registers.
//   phase 2  thread 0 runs acc = delta_t + g_t*c_t*acc backwards over LDS, in
//            the reference's order; vs - V overwrites delta.
//   phase 3  per row: pg advantage from the LDS arrays (vs_{t+1} of the last
//            step is the bootstrap, stored as step T), gradient from the kept
//            registers or from a second read of the target row; lane 0 writes
//            grad_values / vs_out and accumulates the three sums.
// The sums are combined per workgroup in wave order, one thread per component,
// then one atomicAdd each.  Dynamic LDS = 8 per-step arrays + the reduction scratch,
// independent of A; the launcher returns -3 above 160 KiB and raises the
// kernel's dynamic-LDS limit once when a launch needs more than 48 KiB.
//
// ppo_loss_wide_kernel<RESIDENT>.  A wave per row, grid-stride over rows, 4
// waves per workgroup; RESIDENT (A <= 512) takes the gradient from registers.
// The three means are summed per wave, per workgroup in wave order, then
// atomicAdd.  There is no matrix product in either loss, so no MFMA.

#include <climits>

#include "common.h"
#include "policy_loss_wide.h"

#define PLW_CHUNK (PLW_REG_K * WAVE)

// ---------------------------------------------------------------- row math

struct RowStats {
  float lse;  // log sum exp x
  float h;    // sum p log p (only with WITH_H)
  float xa;   // logit of the taken action, NaN if it is outside [0,A)
};

// One pass over `row`; the same result in every lane.  On return x holds the
// row's last chunk: the whole row when A <= PLW_CHUNK.
template <bool WITH_H>
__device__ __forceinline__ RowStats row_stats(const float* __restrict__ row,
                                              int A, int lane, long a,
                                              float (&x)[PLW_REG_K]) {
  float mx = -INFINITY, s = 0.f, u = 0.f, xa = NAN;
  for (int base = 0; base < A; base += PLW_CHUNK) {
    float cm = -INFINITY;
    #pragma unroll
    for (int k = 0; k < PLW_REG_K; ++k) {
      const int j = base + k * WAVE + lane;
      x[k] = j < A ? row[j] : -INFINITY;
      if (j < A && j == a) xa = x[k];
      cm = fmaxf(cm, x[k]);
    }
    cm = wave_all_max(cm);
    if (cm > mx) {
      if (base > 0) {  // earlier chunks were summed against a smaller max
        const float d = mx - cm;
        const float c = expf(d);
        if (WITH_H) u = c * (u + s * d);
        s *= c;
      }
      mx = cm;
    }
    #pragma unroll
    for (int k = 0; k < PLW_REG_K; ++k) {
      if (base + k * WAVE + lane < A) {
        const float xm = x[k] - mx;
        const float e = expf(xm);
        s += e;
        if (WITH_H) u += e * xm;
      }
    }
  }
  s = wave_all_sum(s);
  const float ls = logf(s);
  RowStats r;
  r.lse = mx + ls;
  r.h = WITH_H ? wave_all_sum(u) / s - ls : 0.f;
  r.xa = __shfl(xa, (int)(a & (WAVE - 1)), WAVE);
  return r;
}

// scale * d/dx_j of  w*logp(a) + ec*sum_k p_k logp_k
__device__ __forceinline__ float grad_elem(float xj, bool taken, float lse,
                                           float h, float w, float ec,
                                           float scale) {
  const float lp = xj - lse;
  const float pj = expf(lp);
  return (w * ((taken ? 1.f : 0.f) - pj) + ec * pj * (lp - h)) * scale;
}

// Writes the row's gradient: from x where the wave kept the row (KEPT needs
// A <= PLW_CHUNK), otherwise from a second read of `row`.
template <bool KEPT>
__device__ __forceinline__ void row_grad(const float* __restrict__ row,
                                         float* __restrict__ grow, int A,
                                         int lane, long a,
                                         const float (&x)[PLW_REG_K],
                                         float lse, float h, float w, float ec,
                                         float scale) {
  if (KEPT) {
    #pragma unroll
    for (int k = 0; k < PLW_REG_K; ++k) {
      const int j = k * WAVE + lane;
      if (j < A) grow[j] = grad_elem(x[k], j == a, lse, h, w, ec, scale);
    }
    return;
  }
  for (int base = 0; base < A; base += PLW_CHUNK) {
    float y[PLW_REG_K];
    #pragma unroll
    for (int k = 0; k < PLW_REG_K; ++k) {
      const int j = base + k * WAVE + lane;
      y[k] = j < A ? row[j] : 0.f;
    }
    #pragma unroll
    for (int k = 0; k < PLW_REG_K; ++k) {
      const int j = base + k * WAVE + lane;
      if (j < A) grow[j] = grad_elem(y[k], j == a, lse, h, w, ec, scale);
    }
  }
}

// ------------------------------------------------------------------ IMPALA

#define PLW_IMPALA_WAVES 16
#define PLW_IMPALA_BLOCK (PLW_IMPALA_WAVES * WAVE)
#define PLW_LDS_LIMIT (160 * 1024)

struct ImpalaWideArgs {
  const float* behavior_logits;  // [T,B,A]
  const float* target_logits;    // [T,B,A]
  const long* actions;           // [T,B]
  const float* rewards;          // [T,B]
  const float* discounts;        // [T,B]
  const float* values;           // [T,B]
  const float* bootstrap;        // [B]
  float* grad_logits;            // [T,B,A] out
  float* grad_values;            // [T,B] out
  float* loss_out;               // [3] atomic: pg, baseline, entropy sums
  float* vs_out;                 // [T,B] out or null
  float clip_rho, clip_c, clip_pg_rho, baseline_cost, entropy_cost;
  int T, B, A;
};

// The per-step arrays of one column.  delta and v have T+1 entries: step T
// is (0, bootstrap), so that vs_{t+1} = delta[t+1] + v[t+1] holds at t = T-1.
struct ImpalaLds {
  float *rho, *lse, *h, *la, *g, *r, *delta, *v, *red;
  __device__ __forceinline__ ImpalaLds(float* base, int T) {
    rho = base;
    lse = rho + T;
    h = lse + T;
    la = h + T;
    g = la + T;
    r = g + T;
    delta = r + T;
    v = delta + T + 1;
    red = v + T + 1;  // [3][PLW_IMPALA_WAVES]
  }
};

static size_t impala_wide_lds_bytes(long T) {
  return (size_t)(8 * T + 2 + 3 * PLW_IMPALA_WAVES) * sizeof(float);
}

__device__ __forceinline__ void impala_phase1_row(const ImpalaWideArgs& p,
                                                  const ImpalaLds& s, int t,
                                                  int b, int lane,
                                                  float (&x)[PLW_REG_K]) {
  const long row = (long)t * p.B + b;
  const long a = p.actions[row];
  const RowStats bs =
      row_stats<false>(p.behavior_logits + row * p.A, p.A, lane, a, x);
  const RowStats ts =
      row_stats<true>(p.target_logits + row * p.A, p.A, lane, a, x);
  const float v_t = p.values[row];
  const float v_tp1 = t + 1 < p.T ? p.values[row + p.B] : p.bootstrap[b];
  const float r_t = p.rewards[row];
  const float g_t = p.discounts[row];
  if (lane == 0) {
    const float la = ts.xa - ts.lse;
    const float rho = expf(la - (bs.xa - bs.lse));
    s.rho[t] = rho;
    s.lse[t] = ts.lse;
    s.h[t] = ts.h;
    s.la[t] = la;
    s.g[t] = g_t;
    s.r[t] = r_t;
    s.v[t] = v_t;
    s.delta[t] = fminf(rho, p.clip_rho) * (r_t + g_t * v_tp1 - v_t);
  }
}

template <bool KEPT>
__device__ __forceinline__ void impala_phase3_row(
    const ImpalaWideArgs& p, const ImpalaLds& s, int t, int b, int lane,
    const float (&x)[PLW_REG_K], float& pg_acc, float& base_acc,
    float& ent_acc) {
  const long row = (long)t * p.B + b;
  const float vs_minus_v = s.delta[t];
  const float v_t = s.v[t];
  const float vs_tp1 = s.delta[t + 1] + s.v[t + 1];
  const float adv =
      fminf(s.rho[t], p.clip_pg_rho) * (s.r[t] + s.g[t] * vs_tp1 - v_t);
  const float h = s.h[t];
  row_grad<KEPT>(p.target_logits + row * p.A, p.grad_logits + row * p.A, p.A,
                 lane, p.actions[row], x, s.lse[t], h, -adv, p.entropy_cost,
                 1.f);
  if (lane == 0) {
    if (p.vs_out) p.vs_out[row] = vs_minus_v + v_t;
    p.grad_values[row] = p.baseline_cost * (-vs_minus_v);
    pg_acc += -s.la[t] * adv;
    base_acc += 0.5f * vs_minus_v * vs_minus_v;
    ent_acc += h;
  }
}

// NR = target rows a wave keeps in registers (needs A <= PLW_CHUNK and
// T <= NR * PLW_IMPALA_WAVES); 0 = phase 3 reads the target row again.
template <int NR>
__global__ void __launch_bounds__(PLW_IMPALA_BLOCK)
impala_loss_wide_kernel(ImpalaWideArgs p) {
  extern __shared__ __attribute__((aligned(16))) float plw_lds[];
  const ImpalaLds s(plw_lds, p.T);
  const int b = blockIdx.x;
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x >> 6;
  const int T = p.T;

  float kept[NR > 0 ? NR : 1][PLW_REG_K];
  if (NR > 0) {
    #pragma unroll
    for (int i = 0; i < NR; ++i) {
      const int t = wid + i * PLW_IMPALA_WAVES;  // wave-uniform
      if (t < T) impala_phase1_row(p, s, t, b, lane, kept[i]);
    }
  } else {
    for (int t = wid; t < T; t += PLW_IMPALA_WAVES)
      impala_phase1_row(p, s, t, b, lane, kept[0]);
  }
  if (threadIdx.x == 0) {
    s.delta[T] = 0.f;
    s.v[T] = p.bootstrap[b];
  }
  __syncthreads();

  if (threadIdx.x == 0) {
    float acc = 0.f;
    #pragma unroll 4
    for (int t = T - 1; t >= 0; --t) {
      acc = s.delta[t] + s.g[t] * fminf(s.rho[t], p.clip_c) * acc;
      s.delta[t] = acc;  // vs_t - V_t
    }
  }
  __syncthreads();

  float pg_acc = 0.f, base_acc = 0.f, ent_acc = 0.f;
  if (NR > 0) {
    #pragma unroll
    for (int i = 0; i < NR; ++i) {
      const int t = wid + i * PLW_IMPALA_WAVES;
      if (t < T)
        impala_phase3_row<true>(p, s, t, b, lane, kept[i], pg_acc, base_acc,
                                ent_acc);
    }
  } else {
    for (int t = wid; t < T; t += PLW_IMPALA_WAVES)
      impala_phase3_row<false>(p, s, t, b, lane, kept[0], pg_acc, base_acc,
                               ent_acc);
  }
  if (lane == 0) {
    s.red[wid] = pg_acc;
    s.red[PLW_IMPALA_WAVES + wid] = base_acc;
    s.red[2 * PLW_IMPALA_WAVES + wid] = ent_acc;
  }
  __syncthreads();
  if (threadIdx.x < 3) {  // one thread per component, waves in order
    float tot = 0.f;
    for (int w = 0; w < PLW_IMPALA_WAVES; ++w)
      tot += s.red[threadIdx.x * PLW_IMPALA_WAVES + w];
    atomicAdd(p.loss_out + threadIdx.x, tot);
  }
}

template <int NR>
static int impala_wide_launch_nr(const ImpalaWideArgs& p, size_t lds,
                                 hipStream_t stream) {
  static bool raised = false;  // per instantiation
  if (lds > 48 * 1024 && !raised) {
    const hipError_t err = hipFuncSetAttribute(
        reinterpret_cast<const void*>(impala_loss_wide_kernel<NR>),
        hipFuncAttributeMaxDynamicSharedMemorySize, PLW_LDS_LIMIT);
    if (err != hipSuccess) return (int)err;
    raised = true;
  }
  hipLaunchKernelGGL(impala_loss_wide_kernel<NR>, dim3((unsigned)p.B),
                     dim3(PLW_IMPALA_BLOCK), lds, stream, p);
  CHECK_LAUNCH();
  return 0;
}

int impala_loss_wide_launch(
    const float* behavior_logits, const float* target_logits,
    const long* actions, const float* rewards, const float* discounts,
    const float* values, const float* bootstrap,
    float clip_rho, float clip_c, float clip_pg_rho,
    float baseline_cost, float entropy_cost,
    long T, long B, long A,
    float* grad_logits, float* grad_values, float* loss_out, float* vs_out,
    hipStream_t stream) {
  if (T < 1 || B < 1 || A < 1 || T > INT_MAX || B > INT_MAX || A > INT_MAX)
    return (int)hipErrorInvalidValue;
  const size_t lds = impala_wide_lds_bytes(T);
  if (lds > PLW_LDS_LIMIT) return -3;

  ImpalaWideArgs p;
  p.behavior_logits = behavior_logits;
  p.target_logits = target_logits;
  p.actions = actions;
  p.rewards = rewards;
  p.discounts = discounts;
  p.values = values;
  p.bootstrap = bootstrap;
  p.grad_logits = grad_logits;
  p.grad_values = grad_values;
  p.loss_out = loss_out;
  p.vs_out = vs_out;
  p.clip_rho = clip_rho;
  p.clip_c = clip_c;
  p.clip_pg_rho = clip_pg_rho;
  p.baseline_cost = baseline_cost;
  p.entropy_cost = entropy_cost;
  p.T = (int)T;
  p.B = (int)B;
  p.A = (int)A;

  const long rows_per_wave = (T + PLW_IMPALA_WAVES - 1) / PLW_IMPALA_WAVES;
  // 6 kept rows (48 registers) is what fits 16 waves per CU without scratch
  if (A > PLW_CHUNK || rows_per_wave > 6)
    return impala_wide_launch_nr<0>(p, lds, stream);
  if (rows_per_wave > 2) return impala_wide_launch_nr<6>(p, lds, stream);
  return impala_wide_launch_nr<2>(p, lds, stream);
}

// --------------------------------------------------------------------- PPO

#define PLW_PPO_WAVES 4
#define PLW_PPO_BLOCK (PLW_PPO_WAVES * WAVE)

template <bool RESIDENT>
__global__ void __launch_bounds__(PLW_PPO_BLOCK)
ppo_loss_wide_kernel(const float* __restrict__ logits,    // [N,A]
                     const long* __restrict__ actions,    // [N]
                     const float* __restrict__ old_logp,  // [N]
                     const float* __restrict__ adv,       // [N]
                     const float* __restrict__ returns,   // [N]
                     const float* __restrict__ values,    // [N]
                     float clip_eps, float vcoef, float ecoef, long N, int A,
                     float* __restrict__ grad_logits,     // [N,A] out
                     float* __restrict__ grad_values,     // [N] out
                     float* __restrict__ loss_out) {      // [3]: pg, v, ent
  __shared__ float red[3][PLW_PPO_WAVES];
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x >> 6;
  const float invN = 1.0f / (float)N;
  float pg_acc = 0.f, v_acc = 0.f, ent_acc = 0.f;
  for (long i = (long)blockIdx.x * PLW_PPO_WAVES + wid; i < N;
       i += (long)gridDim.x * PLW_PPO_WAVES) {
    const float* row = logits + i * A;
    const long a = actions[i];
    float x[PLW_REG_K];
    const RowStats st = row_stats<true>(row, A, lane, a, x);
    const float ratio = expf((st.xa - st.lse) - old_logp[i]);
    const float rc = fminf(fmaxf(ratio, 1.f - clip_eps), 1.f + clip_eps);
    const float s1 = ratio * adv[i];
    const float s2 = rc * adv[i];
    // d(-min)/d logp_a: the s1 branch when s1 <= s2 (d s1/d logp_a = s1);
    // the s2 branch only where its clamp is not saturated (then s2 == s1)
    float dmin_dlogpa = 0.f;
    if (s1 <= s2) dmin_dlogpa = -s1;
    else if (ratio > 1.f - clip_eps && ratio < 1.f + clip_eps)
      dmin_dlogpa = -s1;
    row_grad<RESIDENT>(row, grad_logits + i * A, A, lane, a, x, st.lse, st.h,
                       dmin_dlogpa, ecoef, invN);
    if (lane == 0) {
      const float vd = values[i] - returns[i];
      grad_values[i] = vcoef * 2.f * vd * invN;
      pg_acc += -fminf(s1, s2);
      v_acc += vd * vd;
      ent_acc += -st.h;
    }
  }
  if (lane == 0) {
    red[0][wid] = pg_acc;
    red[1][wid] = v_acc;
    red[2][wid] = ent_acc;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    float tot = 0.f;
    for (int w = 0; w < PLW_PPO_WAVES; ++w) tot += red[threadIdx.x][w];
    atomicAdd(loss_out + threadIdx.x, tot * invN);
  }
}

int ppo_loss_wide_launch(const float* logits, const long* actions,
                         const float* old_logp, const float* adv,
                         const float* returns, const float* values,
                         float clip_eps, float vcoef, float ecoef,
                         long N, long A, float* grad_logits,
                         float* grad_values, float* loss_out,
                         hipStream_t stream) {
  if (N < 1 || A < 1 || A > INT_MAX) return (int)hipErrorInvalidValue;
  // a wave per row; at most 8 workgroups' worth of rows per CU, then stride
  long grid = (N + PLW_PPO_WAVES - 1) / PLW_PPO_WAVES;
  if (grid > 2048) grid = 2048;
  if (A <= PLW_CHUNK)
    hipLaunchKernelGGL(ppo_loss_wide_kernel<true>, dim3((unsigned)grid),
                       dim3(PLW_PPO_BLOCK), 0, stream, logits, actions,
                       old_logp, adv, returns, values, clip_eps, vcoef, ecoef,
                       N, (int)A, grad_logits, grad_values, loss_out);
  else
    hipLaunchKernelGGL(ppo_loss_wide_kernel<false>, dim3((unsigned)grid),
                       dim3(PLW_PPO_BLOCK), 0, stream, logits, actions,
                       old_logp, adv, returns, values, clip_eps, vcoef, ecoef,
                       N, (int)A, grad_logits, grad_values, loss_out);
  CHECK_LAUNCH();
  return 0;
}
