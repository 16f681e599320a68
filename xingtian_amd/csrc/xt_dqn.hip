// DQN on the device: the row gather out of the HBM replay ring and the TD-target / MSE head
// (xt/algorithm/dqn/dqn.py:61-103 + `model.compile(loss='mse')` of xt/model/dqn/dqn_cnn.py, dqn_mlp.py).
// Both kernels are bandwidth- and latency-trivial (a minibatch is 32 rows); what matters is 64-bit addressing into a
// ring of several GB, 16-byte accesses and a fixed reduction order.
#include <cmath>

#include "xt_common.h"

namespace xt {

// dst[b] = ring[slots[b]], rows of row_bytes = 16 * nvec bytes.  Grid (ceil(nvec / 256), B): one 16-byte vector per
// thread.  The row offset slot * row_bytes is formed in 64 bits (a 400 000-row ring of 84x84x4 frames is 11.3 GB).  A slot
// outside [0, capacity) reads nothing and leaves a zero row.
__global__ __launch_bounds__(256) void replay_gather_kernel(const uint4* __restrict__ ring, long long nvec,
                                                            long long capacity, const int32_t* __restrict__ slots,
                                                            uint4* __restrict__ dst) {
  const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
  if (v >= nvec) return;
  const long long b = blockIdx.y;
  const long long slot = slots[b];
  uint4 x = make_uint4(0u, 0u, 0u, 0u);
  if (slot >= 0 && slot < capacity) x = ring[slot * nvec + v];
  dst[b * nvec + v] = x;
}

// replay_gather_kernel with the n-step walk of DESIGN.md section 7 in front: the workgroup's start slot s = slots[b] is walked
// over the rows that follow it in its message -- R = reward[s]; g = gamma; while k < n - 1, k < follow[s] and not
// done[s + k]: ++k, R = R + g * reward[s + k] (product rounded, then sum rounded), g = g * gamma -- and the row copied is
// ring[(s + k) % capacity].  The at most n <= 256 reward / done entries the walk can touch are loaded by one thread each
// (one memory round trip whatever n is), thread 0 walks them in LDS and hands the boot slot to the others through LDS.
// Every workgroup of a row repeats the walk (7 for an 84x84x4 frame); those with blockIdx.x == 0 store the labels
// boot_slots / action_n / reward_n / disc_n / done_n [B].  All indices are taken modulo capacity.  A start slot outside
// [0, capacity) reads nothing: zero row, labels (slot, 0, 0, gamma, 1).
__global__ __launch_bounds__(256) void replay_gather_nstep_kernel(
    const uint4* __restrict__ ring, long long nvec, long long capacity, const int32_t* __restrict__ slots,
    const int32_t* __restrict__ action, const double* __restrict__ reward, const uint8_t* __restrict__ done,
    const int32_t* __restrict__ follow, int n, double gamma, uint4* __restrict__ dst, int32_t* __restrict__ boot_slots,
    int32_t* __restrict__ action_n, double* __restrict__ reward_n, double* __restrict__ disc_n,
    uint8_t* __restrict__ done_n) {
  __shared__ double s_reward[256];
  __shared__ uint8_t s_done[256];
  __shared__ long long s_boot;
  const int t = threadIdx.x;
  const long long b = blockIdx.y;
  const long long slot = slots[b];
  const bool live = slot >= 0 && slot < capacity;
  int steps = 0;                                    // rows behind the start row the walk may reach
  if (live) {
    const int f = follow[slot];
    steps = f < n - 1 ? f : n - 1;
    steps = steps < 0 ? 0 : steps;
  }
  if (live && t <= steps) {
    long long j = slot + t;
    if (j >= capacity) j %= capacity;
    s_reward[t] = reward[j];
    s_done[t] = done[j];
  }
  __syncthreads();
  if (t == 0) {
    long long j = slot;
    double R = 0.0, g = gamma;
    int32_t act = 0;
    uint8_t dn = 1;
    if (live) {
      int k = 0;
      R = s_reward[0];
      while (k < steps && !s_done[k]) {
        ++k;
        R = R + g * s_reward[k];
        g = g * gamma;
      }
      j = slot + k;
      if (j >= capacity) j %= capacity;
      dn = s_done[k];
      act = action[slot];
    }
    s_boot = j;
    if (blockIdx.x == 0) {
      boot_slots[b] = (int32_t)j; action_n[b] = act; reward_n[b] = R; disc_n[b] = g; done_n[b] = dn;
    }
  }
  __syncthreads();
  const long long v = (long long)blockIdx.x * 256 + t;
  if (v >= nvec) return;
  uint4 x = make_uint4(0u, 0u, 0u, 0u);
  if (live) x = ring[s_boot * nvec + v];
  dst[b * nvec + v] = x;
}

// Q of one row from the two heads: the [A] head as it is, or s + (l_a - mean_a l) with the 1-wide head s (dueling)
__device__ __forceinline__ float dqn_mean(const float* __restrict__ l, int A) {
  float s = 0.f;
  for (int a = 0; a < A; ++a) s += l[a];
  return s / (float)A;
}
__device__ __forceinline__ float dqn_q(const float* __restrict__ l, float s, float mean, int a, bool dueling) {
  return dueling ? s + (l[a] - mean) : l[a];
}
// first maximal index, as np.argmax
__device__ __forceinline__ int dqn_argmax(const float* __restrict__ l, float s, float mean, int A, bool dueling) {
  int best = 0;
  float qb = dqn_q(l, s, mean, 0, dueling);
  for (int a = 1; a < A; ++a) {
    const float q = dqn_q(l, s, mean, a, dueling);
    if (q > qb) { qb = q; best = a; }
  }
  return best;
}

// One thread per sample: bootstrap action, TD target, d loss / d heads.  terms[b] = (delta_b, maxq_b).  weights (may be
// NULL): the importance weight w_b of prioritised replay, rounded once to float32, scales g_b.  disc (may be NULL): the
// per-sample discount gamma^m of an m-step target, in gamma's place.
__global__ __launch_bounds__(256) void dqn_loss_kernel(const float* __restrict__ logits, const float* __restrict__ value,
                                                       const float* __restrict__ t_logits, const float* __restrict__ t_value,
                                                       const float* __restrict__ o_logits, const float* __restrict__ o_value,
                                                       int B, int A, int dueling, const int32_t* __restrict__ slots,
                                                       const int32_t* __restrict__ action, const double* __restrict__ reward,
                                                       const uint8_t* __restrict__ done, double gamma,
                                                       float* __restrict__ dlogits, float* __restrict__ dvalue,
                                                       float2* __restrict__ terms, float* __restrict__ y_out,
                                                       int32_t* __restrict__ astar_out, float* __restrict__ maxq_out,
                                                       const double* __restrict__ weights,
                                                       const double* __restrict__ disc) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const bool du = dueling != 0;
  const long long row = slots ? (long long)slots[b] : (long long)b;
  const float* tl = t_logits + (size_t)b * A;
  const float ts = du ? t_value[b] : 0.f;
  const float tmean = du ? dqn_mean(tl, A) : 0.f;
  int astar;
  if (o_logits) {                                  // double DQN: the online net picks, the target net evaluates
    const float* ol = o_logits + (size_t)b * A;
    astar = dqn_argmax(ol, du ? o_value[b] : 0.f, du ? dqn_mean(ol, A) : 0.f, A, du);
  } else {
    astar = dqn_argmax(tl, ts, tmean, A, du);
  }
  const float maxq = dqn_q(tl, ts, tmean, astar, du);
  const double r = reward[row];
  const double gm = disc ? disc[b] : gamma;
  const float y = done[row] ? (float)r : (float)(r + gm * (double)maxq);
  int act = action[row];
  act = act < 0 ? 0 : (act >= A ? A - 1 : act);    // (an action outside [0, A) never indexes outside the row)
  const float* l = logits + (size_t)b * A;
  const float mean = du ? dqn_mean(l, A) : 0.f;
  const float delta = dqn_q(l, du ? value[b] : 0.f, mean, act, du) - y;
  const float g = 2.f * (weights ? (float)weights[b] * delta : delta) / ((float)B * (float)A);
  const float inv_a = 1.f / (float)A;
  for (int a = 0; a < A; ++a) {
    const float hot = a == act ? 1.f : 0.f;
    dlogits[(size_t)b * A + a] = du ? g * (hot - inv_a) : g * hot;
  }
  dvalue[b] = du ? g : 0.f;
  terms[b] = make_float2(delta, maxq);
  if (y_out) y_out[b] = y;
  if (astar_out) astar_out[b] = astar;
  if (maxq_out) maxq_out[b] = maxq;
}

// fixed-order reduction of the per-sample terms by one block (double precision, LDS tree).  Scalar head (kDist false):
// terms[b] = (delta_b, maxq_b); out = sum_b w_b delta_b^2 / (B A), sum_b |delta_b| / B, sum_b maxq_b / B.  Distributional
// head (kDist true): terms[b] = (loss_b, dist_q_target(a*_b)); out = sum_b w_b loss_b / B, sum_b loss_b / B,
// sum_b terms[b].y / B (A is not read).  weights may be NULL (w_b = 1); the two means stay unweighted.
template <bool kDist>
__global__ __launch_bounds__(256) void dqn_loss_reduce_kernel(const float2* __restrict__ terms, int B, int A,
                                                              float* __restrict__ out, float* __restrict__ acc,
                                                              const double* __restrict__ weights) {
  __shared__ double sq[256], sa[256], sm[256];
  double q = 0.0, a = 0.0, m = 0.0;
  for (int b = threadIdx.x; b < B; b += 256) {
    if constexpr (kDist) {
      const double d = (double)terms[b].x;
      q += weights ? (double)(float)weights[b] * d : d; a += d; m += (double)terms[b].y;
    } else {
      const float d = terms[b].x;
      const double d2 = (double)d * (double)d;
      q += weights ? (double)(float)weights[b] * d2 : d2; a += (double)fabsf(d); m += (double)terms[b].y;
    }
  }
  sq[threadIdx.x] = q; sa[threadIdx.x] = a; sm[threadIdx.x] = m;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      sq[threadIdx.x] += sq[threadIdx.x + o]; sa[threadIdx.x] += sa[threadIdx.x + o]; sm[threadIdx.x] += sm[threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float l = (float)(sq[0] / (kDist ? (double)B : (double)B * (double)A));
    out[0] = l; out[1] = (float)(sa[0] / (double)B); out[2] = (float)(sm[0] / (double)B);
    if (acc) { acc[0] += l; acc[1] += 1.f; }
  }
}

// ---------------------------------------------------------------- distributional (C51) head, DESIGN.md section 7
__device__ __forceinline__ float dist_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float dist_wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
// the float32 atom z_i = (float)(v_min + i * delta), product and sum rounded separately in float64
__device__ __forceinline__ double dist_atom(double v_min, double delta, int i) { return v_min + (double)i * delta; }

// dist_q of one action's N logits by the whole wave (lanes stride the atoms; every lane returns the same bits):
// mx = max l, e_i = expf(l_i - mx), Q = (sum z_i e_i) / (sum e_i).  *mx_out / *se_out: mx and sum e_i.
__device__ __forceinline__ float dist_q_wave(const float* __restrict__ l, int N, double v_min, double delta, int lane,
                                             float* mx_out, float* se_out) {
  float mx = -INFINITY;
  for (int i = lane; i < N; i += 64) mx = fmaxf(mx, l[i]);
  mx = dist_wave_max(mx);
  float se = 0.f, sz = 0.f;
  for (int i = lane; i < N; i += 64) {
    const float e = expf(l[i] - mx);
    se += e;
    sz += (float)dist_atom(v_min, delta, i) * e;
  }
  se = dist_wave_sum(se);
  sz = dist_wave_sum(sz);
  *mx_out = mx; *se_out = se;
  return sz / se;
}

// ---- the dueling form of the two distributional heads (kDuel; DESIGN.md section 7, "Dueling distributional heads").
// A row is (A + 1) * N wide: adv[a, i] = row[a N + i] (a < A), v[i] = row[A N + i], and everything the heads read as
// "logits[a, i]" is l[a, i] = v[i] + (adv[a, i] - mean_i), mean_i = (sum over ascending a of adv[a, i]) / (float)A, as
// dqn_mean / dqn_q.  A lane forms mean_i of its own columns i = lane + 64 k once per net it reads (A strided loads per i)
// and combines on the fly: nothing of the A * N row is staged.
__device__ __forceinline__ void duel_means(const float* __restrict__ row, int A, int N, int lane, float (&mean)[4]) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int i = lane + 64 * k;
    mean[k] = 0.f;
    if (i < N) {
      float s = 0.f;
      for (int a = 0; a < A; ++a) s += row[(size_t)a * N + i];
      mean[k] = s / (float)A;
    }
  }
}
__device__ __forceinline__ float duel_at(const float* __restrict__ row, int A, int N, int a, int i, float mean) {
  return row[(size_t)A * N + i] + (row[(size_t)a * N + i] - mean);
}
// dist_q_wave on the combined logits of action a of a dueling row (mean: the lane's duel_means of that row)
__device__ __forceinline__ float dist_q_wave_duel(const float* __restrict__ row, int A, int N, int a, const float (&mean)[4],
                                                  double v_min, double delta, int lane, float* mx_out, float* se_out) {
  float l[4];
  float mx = -INFINITY;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int i = lane + 64 * k;
    l[k] = 0.f;
    if (i < N) { l[k] = duel_at(row, A, N, a, i, mean[k]); mx = fmaxf(mx, l[k]); }
  }
  mx = dist_wave_max(mx);
  float se = 0.f, sz = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int i = lane + 64 * k;
    if (i < N) {
      const float e = expf(l[k] - mx);
      se += e;
      sz += (float)dist_atom(v_min, delta, i) * e;
    }
  }
  se = dist_wave_sum(se);
  sz = dist_wave_sum(sz);
  *mx_out = mx; *se_out = se;
  return sz / se;
}
// the gradient row of a dueling head from d_i of the lane's columns: dcol[a N + i] = d_i (hot(a == act) - 1 / A) for every
// a < A and dcol[A N + i] = d_i -- the whole (A + 1) * N row, each entry by the one lane that owns column i
__device__ __forceinline__ void duel_store_grad(float* __restrict__ dl, int A, int N, int act, int lane, const float (&d)[4]) {
  const float inv_a = 1.f / (float)A;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int i = lane + 64 * k;
    if (i < N) {
      for (int a = 0; a < A; ++a) dl[(size_t)a * N + i] = d[k] * ((a == act ? 1.f : 0.f) - inv_a);
      dl[(size_t)A * N + i] = d[k];
    }
  }
}

// One wavefront per sample (grid B, 64 threads), lanes stride the atoms (up to 4 per lane at N = 256).  In order:
// dist_q of every action of the picking logits (o_logits, else t_logits) and a* = the first maximal one; p_j = softmax of
// the target logits of a* and b_j = (clamp(dn ? R : R + g z_j) - v_min) / delta into LDS as float64; every lane forms its
// m_i = (float) sum_j p_j max(0, 1 - |b_j - i|) over ascending j (a gather: no atomics, no dependence on thread order);
// then the log-softmax of the taken action's online logits, loss_b = -sum_i m_i logq_i, the gradient row
// w_b (q_i M_b - m_i) / B with exact zeros in every other column, dvalue = 0 and terms[b] = (loss_b, dist_q_target(a*)).
// kDuel: rows are (A + 1) * N wide and every logit read is the combined one (above); the gradient row is duel_store_grad's.
template <bool kDuel>
__global__ __launch_bounds__(64) void dqn_loss_dist_kernel(const float* __restrict__ logits, const float* __restrict__ t_logits,
                                                           const float* __restrict__ o_logits, int B, int A, int N,
                                                           double v_min, double v_max, const int32_t* __restrict__ slots,
                                                           const int32_t* __restrict__ action,
                                                           const double* __restrict__ reward, const uint8_t* __restrict__ done,
                                                           double gamma, float* __restrict__ dlogits,
                                                           float* __restrict__ dvalue, float2* __restrict__ terms,
                                                           int32_t* __restrict__ astar_out, float* __restrict__ maxq_out,
                                                           float* __restrict__ m_out, const double* __restrict__ weights,
                                                           const double* __restrict__ disc) {
  __shared__ double s_p[256], s_b[256];
  const int lane = threadIdx.x;
  const int b = blockIdx.x;
  if (b >= B) return;
  const double delta = (v_max - v_min) / (double)(N - 1);
  const size_t W = (size_t)(kDuel ? A + 1 : A) * N;
  const long long row = slots ? (long long)slots[b] : (long long)b;
  const float* tl = t_logits + (size_t)b * W;
  const float* pl = o_logits ? o_logits + (size_t)b * W : tl;
  float tmean[4], lo[4];                           // kDuel: the target row's means; the combined online logits
  float mx, se;
  int astar = 0;
  float qstar;
  if constexpr (kDuel) {
    float pmean[4];
    duel_means(pl, A, N, lane, pmean);
    float qb = dist_q_wave_duel(pl, A, N, 0, pmean, v_min, delta, lane, &mx, &se);
    for (int a = 1; a < A; ++a) {
      const float q = dist_q_wave_duel(pl, A, N, a, pmean, v_min, delta, lane, &mx, &se);
      if (q > qb) { qb = q; astar = a; }
    }
    if (o_logits) {
      duel_means(tl, A, N, lane, tmean);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) tmean[k] = pmean[k];
    }
    qstar = dist_q_wave_duel(tl, A, N, astar, tmean, v_min, delta, lane, &mx, &se);
  } else {
    float qb = dist_q_wave(pl, N, v_min, delta, lane, &mx, &se);
    for (int a = 1; a < A; ++a) {
      const float q = dist_q_wave(pl + (size_t)a * N, N, v_min, delta, lane, &mx, &se);
      if (q > qb) { qb = q; astar = a; }
    }
    qstar = dist_q_wave(tl + (size_t)astar * N, N, v_min, delta, lane, &mx, &se);
  }
  // (the wave sums leave the same bits in every lane, so a* is uniform)
  const float* ts = tl + (size_t)astar * N;
  const double R = reward[row];
  const double g = disc ? disc[b] : gamma;
  const bool dn = done[row] != 0;
  if constexpr (kDuel) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int j = lane + 64 * k;
      if (j < N) {
        const double z = dist_atom(v_min, delta, j);
        double tz = dn ? R : R + g * z;
        tz = tz < v_min ? v_min : (tz > v_max ? v_max : tz);
        s_p[j] = (double)(expf(duel_at(tl, A, N, astar, j, tmean[k]) - mx) / se);
        s_b[j] = (tz - v_min) / delta;
      }
    }
  } else {
    for (int j = lane; j < N; j += 64) {
      const double z = dist_atom(v_min, delta, j);
      double tz = dn ? R : R + g * z;
      tz = tz < v_min ? v_min : (tz > v_max ? v_max : tz);
      s_p[j] = (double)(expf(ts[j] - mx) / se);
      s_b[j] = (tz - v_min) / delta;
    }
  }
  __syncthreads();
  int act = action[row];
  act = act < 0 ? 0 : (act >= A ? A - 1 : act);    // (an action outside [0, A) never indexes outside the row)
  const float* l = logits + (size_t)b * W + (size_t)act * N;
  float lmx = -INFINITY;
  float lse = 0.f;
  if constexpr (kDuel) {
    const float* lr = logits + (size_t)b * W;
    float omean[4];
    duel_means(lr, A, N, lane, omean);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int i = lane + 64 * k;
      lo[k] = 0.f;
      if (i < N) { lo[k] = duel_at(lr, A, N, act, i, omean[k]); lmx = fmaxf(lmx, lo[k]); }
    }
    lmx = dist_wave_max(lmx);
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (lane + 64 * k < N) lse += expf(lo[k] - lmx);
  } else {
    for (int i = lane; i < N; i += 64) lmx = fmaxf(lmx, l[i]);
    lmx = dist_wave_max(lmx);
    for (int i = lane; i < N; i += 64) lse += expf(l[i] - lmx);
  }
  lse = logf(dist_wave_sum(lse));
  float m[4], lq[4];
  float loss = 0.f, mass = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int i = lane + 64 * k;
    m[k] = 0.f; lq[k] = 0.f;
    if (i < N) {
      double s = 0.0;
      const double di = (double)i;
      for (int j = 0; j < N; ++j) {
        const double w = 1.0 - fabs(s_b[j] - di);
        s += s_p[j] * (w > 0.0 ? w : 0.0);
      }
      m[k] = (float)s;
      if constexpr (kDuel) lq[k] = (lo[k] - lmx) - lse;
      else lq[k] = (l[i] - lmx) - lse;
      loss += m[k] * lq[k];
      mass += m[k];
      if (m_out) m_out[(size_t)b * N + i] = m[k];
    }
  }
  loss = -dist_wave_sum(loss);
  mass = dist_wave_sum(mass);
  const float fb = (float)B;
  float* dl = dlogits + (size_t)b * W;
  if constexpr (kDuel) {
    float dd[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      dd[k] = 0.f;
      if (lane + 64 * k < N) {
        const float d = expf(lq[k]) * mass - m[k];
        dd[k] = (weights ? (float)weights[b] * d : d) / fb;
      }
    }
    duel_store_grad(dl, A, N, act, lane, dd);
  } else {
    const size_t c0 = (size_t)act * N;
    for (size_t c = lane; c < W; c += 64)
      if (c < c0 || c >= c0 + N) dl[c] = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int i = lane + 64 * k;
      if (i < N) {
        const float d = expf(lq[k]) * mass - m[k];
        dl[c0 + i] = (weights ? (float)weights[b] * d : d) / fb;
      }
    }
  }
  if (lane == 0) {
    dvalue[b] = 0.f;
    terms[b] = make_float2(loss, qstar);
    if (astar_out) astar_out[b] = astar;
    if (maxq_out) maxq_out[b] = qstar;
  }
}

// ---------------------------------------------------------------- quantile-regression (QR-DQN) head, DESIGN.md section 7
// quant_q of one action's N quantiles by one thread: the float64 sum over ascending i, divided by N, rounded once
__device__ __forceinline__ float quant_q_of(const float* __restrict__ th, int N) {
  double s = 0.0;
  for (int i = 0; i < N; ++i) s += (double)th[i];
  return (float)(s / (double)N);
}

// One wavefront per sample (grid B, 64 threads), lanes stride the quantiles (up to 4 per lane at N = 256).  In order:
// lane a < A forms quant_q of action a of the picking quantiles (o_logits, else t_logits) by its own ordered sum and a
// butterfly picks a* = the first maximal one; the N targets T_j = (float)(dn ? R : R + g theta'_j) of the target net's
// quantiles of a* go into LDS; every lane forms r_i and g_i of its quantiles of the taken action by the float64 sum over
// ascending j (LDS broadcasts: no atomics, no dependence on thread order); loss_b = sum_i r_i by a wave reduction; then
// the gradient row w_b g_i / B with exact zeros in every other column, dvalue = 0 and terms[b] = (loss_b, quant_q_target(a*)).
// kDuel: rows are (A + 1) * N wide and every quantile read is the combined one (above dqn_loss_dist_kernel).  quant_q stays
// one thread's float64 sum over ascending i, so the lanes leave the mean_i they formed (N floats per net read, not the
// A * N row) in LDS, where the thread that sums action a finds them; the gradient row is duel_store_grad's.
// quant_q of the combined quantiles of action a of a dueling row by one thread (mean: the row's N means)
__device__ __forceinline__ float quant_q_duel(const float* __restrict__ row, int A, int N, int a, const float* mean) {
  double s = 0.0;
  for (int i = 0; i < N; ++i) s += (double)duel_at(row, A, N, a, i, mean[i]);
  return (float)(s / (double)N);
}
__device__ __forceinline__ void duel_means_lds(const float* __restrict__ row, int A, int N, int lane, float* s_mean) {
  float mean[4];
  duel_means(row, A, N, lane, mean);
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (lane + 64 * k < N) s_mean[lane + 64 * k] = mean[k];
}
template <bool kDuel>
__global__ __launch_bounds__(64) void dqn_loss_quant_kernel(const float* __restrict__ logits, const float* __restrict__ t_logits,
                                                            const float* __restrict__ o_logits, int B, int A, int N,
                                                            float kappa, const int32_t* __restrict__ slots,
                                                            const int32_t* __restrict__ action,
                                                            const double* __restrict__ reward, const uint8_t* __restrict__ done,
                                                            double gamma, float* __restrict__ dlogits,
                                                            float* __restrict__ dvalue, float2* __restrict__ terms,
                                                            int32_t* __restrict__ astar_out, float* __restrict__ maxq_out,
                                                            const double* __restrict__ weights,
                                                            const double* __restrict__ disc) {
  __shared__ float s_t[256];
  const int lane = threadIdx.x;
  const int b = blockIdx.x;
  if (b >= B) return;
  __shared__ float s_mean[kDuel ? 3 : 1][kDuel ? 256 : 1];   // kDuel: mean_i of the picking, the target and the online row
  const size_t W = (size_t)(kDuel ? A + 1 : A) * N;
  const long long row = slots ? (long long)slots[b] : (long long)b;
  const float* tl = t_logits + (size_t)b * W;
  const float* pl = o_logits ? o_logits + (size_t)b * W : tl;
  const float* tmean = s_mean[0];
  if constexpr (kDuel) {
    duel_means_lds(pl, A, N, lane, s_mean[0]);
    if (o_logits) { duel_means_lds(tl, A, N, lane, s_mean[1]); tmean = s_mean[1]; }
    duel_means_lds(logits + (size_t)b * W, A, N, lane, s_mean[2]);
    __syncthreads();
  }
  // (A <= 64: one action per lane; a lane without one holds -inf under an index no action has)
  float q;
  if constexpr (kDuel) q = lane < A ? quant_q_duel(pl, A, N, lane, s_mean[0]) : -INFINITY;
  else q = lane < A ? quant_q_of(pl + (size_t)lane * N, N) : -INFINITY;
  float qb = q;
  int astar = lane;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float qo = __shfl_xor(qb, o, 64);
    const int io = __shfl_xor(astar, o, 64);
    if (qo > qb || (qo == qb && io < astar)) { qb = qo; astar = io; }
  }
  astar = __shfl(astar, 0, 64);                    // (uniform whatever the quantiles hold)
  astar = astar < A ? astar : A - 1;
  const float* ts = tl + (size_t)astar * N;
  float qstar;
  if constexpr (kDuel) qstar = o_logits ? quant_q_duel(tl, A, N, astar, tmean) : __shfl(q, astar, 64);
  else qstar = o_logits ? quant_q_of(ts, N) : __shfl(q, astar, 64);
  const double R = reward[row];
  const double g = disc ? disc[b] : gamma;
  const bool dn = done[row] != 0;
  for (int j = lane; j < N; j += 64) {
    float tj;
    if constexpr (kDuel) tj = duel_at(tl, A, N, astar, j, tmean[j]);
    else tj = ts[j];
    s_t[j] = dn ? (float)R : (float)(R + g * (double)tj);
  }
  __syncthreads();
  int act = action[row];
  act = act < 0 ? 0 : (act >= A ? A - 1 : act);    // (an action outside [0, A) never indexes outside the row)
  const float* l = logits + (size_t)b * W + (size_t)act * N;
  const double dN = (double)N;
  float gr[4];
  float loss = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int i = lane + 64 * k;
    gr[k] = 0.f;
    if (i < N) {
      float th;
      if constexpr (kDuel) th = duel_at(logits + (size_t)b * W, A, N, act, i, s_mean[2][i]);
      else th = l[i];
      const double tau = (double)(2 * i + 1) / (2.0 * dN);
      const float w_neg = (float)(1.0 - tau), w_pos = (float)tau;
      double sr = 0.0, sg = 0.0;
      for (int j = 0; j < N; ++j) {
        const float u = s_t[j] - th;
        const float wt = u < 0.f ? w_neg : w_pos;
        const float au = fabsf(u);
        const float hub = au <= kappa ? 0.5f * u * u : kappa * (au - 0.5f * kappa);
        const float cl = u < -kappa ? -kappa : (u > kappa ? kappa : u);
        sr += (double)(wt * hub / kappa);
        sg += (double)(wt * cl / kappa);
      }
      loss += (float)(sr / dN);
      gr[k] = (float)(-sg / dN);
    }
  }
  loss = dist_wave_sum(loss);
  const float fb = (float)B;
  float* dl = dlogits + (size_t)b * W;
  if constexpr (kDuel) {
    float dd[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) dd[k] = lane + 64 * k < N ? (weights ? (float)weights[b] * gr[k] : gr[k]) / fb : 0.f;
    duel_store_grad(dl, A, N, act, lane, dd);
  } else {
    const size_t c0 = (size_t)act * N;
    for (size_t c = lane; c < W; c += 64)
      if (c < c0 || c >= c0 + N) dl[c] = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int i = lane + 64 * k;
      if (i < N) dl[c0 + i] = (weights ? (float)weights[b] * gr[k] : gr[k]) / fb;
    }
  }
  if (lane == 0) {
    dvalue[b] = 0.f;
    terms[b] = make_float2(loss, qstar);
    if (astar_out) astar_out[b] = astar;
    if (maxq_out) maxq_out[b] = qstar;
  }
}

// The checks the two gather entries share (`who` names the entry in refusals); *nvec: 16-byte vectors per row
static int replay_gather_check(const char* who, const void* ring, const void* dst, int64_t row_bytes, int64_t capacity,
                               int32_t B, long long* nvec) {
  XT_REQUIRE(row_bytes > 0 && row_bytes % 16 == 0,
             "%s: row_bytes = %lld is not a positive multiple of 16 (rows are stored as the first layer reads them: "
             "channel-padded images / feature-padded vectors)", who, (long long)row_bytes);
  XT_REQUIRE(capacity > 0 && B > 0 && B <= 65535, "%s: bad sizes (capacity=%lld B=%d)", who, (long long)capacity, B);
  XT_REQUIRE((((uintptr_t)ring | (uintptr_t)dst) & 15) == 0, "%s: ring and dst must be 16-byte aligned", who);
  *nvec = row_bytes / 16;
  XT_REQUIRE((*nvec + 255) / 256 < (1ll << 31), "%s: row_bytes = %lld is too large", who, (long long)row_bytes);
  return 0;
}

// xt_dqn_loss_dist / xt_dqn_loss_dist_duel: the checks and the two launches (`who` names the entry in refusals).  duel: A
// actions on rows (A + 1) * atoms wide, so at most 63 of them (the folded head keeps the step's 64-group limit).
static int dqn_loss_dist_entry(const char* who, bool duel, const float* logits, const float* t_logits, const float* o_logits,
                               int32_t B, int32_t A, int32_t atoms, double v_min, double v_max, const int32_t* slots,
                               const int32_t* action, const double* reward, const uint8_t* done, double gamma, float* dlogits,
                               float* dvalue, float* out, int32_t* astar, float* maxq, float* m, float* acc,
                               const double* weights, const double* disc, void* stream) {
  const int amax = duel ? 63 : 64;
  XT_REQUIRE(logits && t_logits && action && reward && done && dlogits && dvalue && out, "%s: null argument", who);
  XT_REQUIRE(atoms >= 2 && atoms <= 256, "%s: atoms = %d outside [2, 256]", who, atoms);
  XT_REQUIRE(B > 0 && A >= 1 && A <= amax, "%s: bad sizes (B=%d A=%d; 1 <= A <= %d)", who, B, A, amax);
  XT_REQUIRE(std::isfinite(v_min) && std::isfinite(v_max) && v_min < v_max,
             "%s: the support needs finite v_min < v_max (got %g, %g)", who, v_min, v_max);
  XT_REQUIRE(((uintptr_t)out & 7) == 0, "%s: out must be 8-byte aligned", who);
  hipStream_t st = as_stream(stream);
  float2* terms = reinterpret_cast<float2*>(out + 4);       // out: >= 4 + 2*B floats
  if (duel)
    hipLaunchKernelGGL(dqn_loss_dist_kernel<true>, dim3(B), dim3(64), 0, st, logits, t_logits, o_logits, B, A, atoms, v_min,
                       v_max, slots, action, reward, done, gamma, dlogits, dvalue, terms, astar, maxq, m, weights, disc);
  else
    hipLaunchKernelGGL(dqn_loss_dist_kernel<false>, dim3(B), dim3(64), 0, st, logits, t_logits, o_logits, B, A, atoms, v_min,
                       v_max, slots, action, reward, done, gamma, dlogits, dvalue, terms, astar, maxq, m, weights, disc);
  XT_LAUNCH_CHECK();
  hipLaunchKernelGGL(dqn_loss_reduce_kernel<true>, dim3(1), dim3(256), 0, st, terms, B, A, out, acc, weights);
  XT_LAUNCH_CHECK();
  return 0;
}

// xt_dqn_loss_quant / xt_dqn_loss_quant_duel, likewise
static int dqn_loss_quant_entry(const char* who, bool duel, const float* logits, const float* t_logits, const float* o_logits,
                                int32_t B, int32_t A, int32_t quantiles, double kappa, const int32_t* slots,
                                const int32_t* action, const double* reward, const uint8_t* done, double gamma, float* dlogits,
                                float* dvalue, float* out, int32_t* astar, float* maxq, float* acc, const double* weights,
                                const double* disc, void* stream) {
  const int amax = duel ? 63 : 64;
  XT_REQUIRE(logits && t_logits && action && reward && done && dlogits && dvalue && out, "%s: null argument", who);
  XT_REQUIRE(quantiles >= 2 && quantiles <= 256, "%s: quantiles = %d outside [2, 256]", who, quantiles);
  XT_REQUIRE(B > 0 && A >= 1 && A <= amax, "%s: bad sizes (B=%d A=%d; 1 <= A <= %d)", who, B, A, amax);
  XT_REQUIRE(std::isfinite(kappa) && (float)kappa > 0.f && std::isfinite((float)kappa),
             "%s: kappa must be finite and > 0 as a float32 (got %g)", who, kappa);
  XT_REQUIRE(((uintptr_t)out & 7) == 0, "%s: out must be 8-byte aligned", who);
  hipStream_t st = as_stream(stream);
  float2* terms = reinterpret_cast<float2*>(out + 4);       // out: >= 4 + 2*B floats
  if (duel)
    hipLaunchKernelGGL(dqn_loss_quant_kernel<true>, dim3(B), dim3(64), 0, st, logits, t_logits, o_logits, B, A, quantiles,
                       (float)kappa, slots, action, reward, done, gamma, dlogits, dvalue, terms, astar, maxq, weights, disc);
  else
    hipLaunchKernelGGL(dqn_loss_quant_kernel<false>, dim3(B), dim3(64), 0, st, logits, t_logits, o_logits, B, A, quantiles,
                       (float)kappa, slots, action, reward, done, gamma, dlogits, dvalue, terms, astar, maxq, weights, disc);
  XT_LAUNCH_CHECK();
  hipLaunchKernelGGL(dqn_loss_reduce_kernel<true>, dim3(1), dim3(256), 0, st, terms, B, A, out, acc, weights);
  XT_LAUNCH_CHECK();
  return 0;
}

}  // namespace xt

extern "C" {

int xt_dqn_loss_dist(const float* logits, const float* t_logits, const float* o_logits, int32_t B, int32_t A, int32_t atoms,
                     double v_min, double v_max, const int32_t* slots, const int32_t* action, const double* reward,
                     const uint8_t* done, double gamma, float* dlogits, float* dvalue, float* out, int32_t* astar,
                     float* maxq, float* m, float* acc, const double* weights, const double* disc, void* stream) {
  return xt::dqn_loss_dist_entry("xt_dqn_loss_dist", false, logits, t_logits, o_logits, B, A, atoms, v_min, v_max, slots, action,
                                 reward, done, gamma, dlogits, dvalue, out, astar, maxq, m, acc, weights, disc, stream);
}

int xt_dqn_loss_dist_duel(const float* logits, const float* t_logits, const float* o_logits, int32_t B, int32_t A,
                          int32_t atoms, double v_min, double v_max, const int32_t* slots, const int32_t* action,
                          const double* reward, const uint8_t* done, double gamma, float* dlogits, float* dvalue, float* out,
                          int32_t* astar, float* maxq, float* m, float* acc, const double* weights, const double* disc,
                          void* stream) {
  return xt::dqn_loss_dist_entry("xt_dqn_loss_dist_duel", true, logits, t_logits, o_logits, B, A, atoms, v_min, v_max, slots,
                                 action, reward, done, gamma, dlogits, dvalue, out, astar, maxq, m, acc, weights, disc, stream);
}

int xt_dqn_loss_quant(const float* logits, const float* t_logits, const float* o_logits, int32_t B, int32_t A,
                      int32_t quantiles, double kappa, const int32_t* slots, const int32_t* action, const double* reward,
                      const uint8_t* done, double gamma, float* dlogits, float* dvalue, float* out, int32_t* astar, float* maxq,
                      float* acc, const double* weights, const double* disc, void* stream) {
  return xt::dqn_loss_quant_entry("xt_dqn_loss_quant", false, logits, t_logits, o_logits, B, A, quantiles, kappa, slots, action,
                                  reward, done, gamma, dlogits, dvalue, out, astar, maxq, acc, weights, disc, stream);
}

int xt_dqn_loss_quant_duel(const float* logits, const float* t_logits, const float* o_logits, int32_t B, int32_t A,
                           int32_t quantiles, double kappa, const int32_t* slots, const int32_t* action, const double* reward,
                           const uint8_t* done, double gamma, float* dlogits, float* dvalue, float* out, int32_t* astar,
                           float* maxq, float* acc, const double* weights, const double* disc, void* stream) {
  return xt::dqn_loss_quant_entry("xt_dqn_loss_quant_duel", true, logits, t_logits, o_logits, B, A, quantiles, kappa, slots,
                                  action, reward, done, gamma, dlogits, dvalue, out, astar, maxq, acc, weights, disc, stream);
}

int xt_replay_gather(const void* ring, int64_t row_bytes, int64_t capacity, const int32_t* slots, int32_t B, void* dst,
                     void* stream) {
  XT_REQUIRE(ring && slots && dst, "xt_replay_gather: null argument");
  long long nvec;
  if (int rc = xt::replay_gather_check("xt_replay_gather", ring, dst, row_bytes, capacity, B, &nvec)) return rc;
  hipLaunchKernelGGL(xt::replay_gather_kernel, dim3((unsigned)((nvec + 255) / 256), (unsigned)B), dim3(256), 0,
                     xt::as_stream(stream), static_cast<const uint4*>(ring), nvec, (long long)capacity, slots,
                     static_cast<uint4*>(dst));
  XT_LAUNCH_CHECK();
  return 0;
}

int xt_replay_gather_nstep(const void* next_ring, int64_t row_bytes, int64_t capacity, const int32_t* slots, int32_t B,
                           const int32_t* action, const double* reward, const uint8_t* done, const int32_t* follow,
                           int32_t n, double gamma, void* dst, int32_t* boot_slots, int32_t* action_n, double* reward_n,
                           double* disc_n, uint8_t* done_n, void* stream) {
  XT_REQUIRE(next_ring && slots && dst && action && reward && done && follow, "xt_replay_gather_nstep: null argument");
  XT_REQUIRE(boot_slots && action_n && reward_n && disc_n && done_n, "xt_replay_gather_nstep: null label output");
  XT_REQUIRE(n >= 1 && n <= 256, "xt_replay_gather_nstep: n = %d outside [1, 256]", n);
  long long nvec;
  if (int rc = xt::replay_gather_check("xt_replay_gather_nstep", next_ring, dst, row_bytes, capacity, B, &nvec))
    return rc;
  hipLaunchKernelGGL(xt::replay_gather_nstep_kernel, dim3((unsigned)((nvec + 255) / 256), (unsigned)B), dim3(256), 0,
                     xt::as_stream(stream), static_cast<const uint4*>(next_ring), nvec, (long long)capacity, slots, action,
                     reward, done, follow, n, gamma, static_cast<uint4*>(dst), boot_slots, action_n, reward_n, disc_n,
                     done_n);
  XT_LAUNCH_CHECK();
  return 0;
}

int xt_dqn_loss_n(const float* logits, const float* value, const float* t_logits, const float* t_value,
                  const float* o_logits, const float* o_value, int32_t B, int32_t A, int32_t dueling, const int32_t* slots,
                  const int32_t* action, const double* reward, const uint8_t* done, double gamma, float* dlogits,
                  float* dvalue, float* out, float* y, int32_t* astar, float* maxq, float* acc, const double* weights,
                  const double* disc, void* stream) {
  XT_REQUIRE(logits && t_logits && action && reward && done && dlogits && dvalue && out, "xt_dqn_loss: null argument");
  XT_REQUIRE(!dueling || (value && t_value && (!o_logits || o_value)), "xt_dqn_loss: dueling needs the 1-wide heads");
  XT_REQUIRE(B > 0 && A > 0 && A <= 64, "xt_dqn_loss: bad sizes (B=%d A=%d; A <= 64)", B, A);
  XT_REQUIRE(((uintptr_t)out & 7) == 0, "xt_dqn_loss: out must be 8-byte aligned");
  hipStream_t st = xt::as_stream(stream);
  float2* terms = reinterpret_cast<float2*>(out + 4);       // out: >= 4 + 2*B floats
  hipLaunchKernelGGL(xt::dqn_loss_kernel, dim3((B + 255) / 256), dim3(256), 0, st, logits, value, t_logits, t_value, o_logits,
                     o_value, B, A, dueling, slots, action, reward, done, gamma, dlogits, dvalue, terms, y, astar, maxq, weights,
                     disc);
  XT_LAUNCH_CHECK();
  hipLaunchKernelGGL(xt::dqn_loss_reduce_kernel<false>, dim3(1), dim3(256), 0, st, terms, B, A, out, acc, weights);
  XT_LAUNCH_CHECK();
  return 0;
}

int xt_dqn_loss_w(const float* logits, const float* value, const float* t_logits, const float* t_value,
                  const float* o_logits, const float* o_value, int32_t B, int32_t A, int32_t dueling, const int32_t* slots,
                  const int32_t* action, const double* reward, const uint8_t* done, double gamma, float* dlogits,
                  float* dvalue, float* out, float* y, int32_t* astar, float* maxq, float* acc, const double* weights,
                  void* stream) {
  return xt_dqn_loss_n(logits, value, t_logits, t_value, o_logits, o_value, B, A, dueling, slots, action, reward, done, gamma,
                       dlogits, dvalue, out, y, astar, maxq, acc, weights, nullptr, stream);
}

int xt_dqn_loss(const float* logits, const float* value, const float* t_logits, const float* t_value,
                const float* o_logits, const float* o_value, int32_t B, int32_t A, int32_t dueling, const int32_t* slots,
                const int32_t* action, const double* reward, const uint8_t* done, double gamma, float* dlogits,
                float* dvalue, float* out, float* y, int32_t* astar, float* maxq, float* acc, void* stream) {
  return xt_dqn_loss_w(logits, value, t_logits, t_value, o_logits, o_value, B, A, dueling, slots, action, reward, done, gamma,
                       dlogits, dvalue, out, y, astar, maxq, acc, nullptr, stream);
}

}  // extern "C"
