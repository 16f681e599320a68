// QMIX: GRU agents and the monotonic mixer (xt_qmix_* of include/xt_mi355x.h).
//
//   qmix_gru_fwd_kernel   persistent recurrent forward: a workgroup owns 16 sequences and walks all steps itself; the
//                         recurrent halves of the two GRU kernels stay in registers as fp32 MFMA B-fragments
//   qmix_gru_bwd_kernel   persistent BPTT on the same tiling, walking t downward with the transposed fragments
//   qmix_mix_kernel       action gather, masking, double-Q arg-max, both mixers, TD error and the eval mixer's backward,
//                         one wavefront per (episode, step) row
//   qmix_norm_kernel / qmix_rmsprop_kernel   centred RMSProp with tf.clip_by_norm per tensor
// Everything that is not sequential (dense, the input half of the GRU, dense_1, the hypernet layers; forward, input
// gradient, weight gradient) runs on the two plain kernels dense_gemm_kernel / dense_wgrad_kernel of xt_dense_dev.h over the
// stacked rows, any width; the agent's forward and backward are agent_fwd / agent_bwd of xt_qmix_dev.h, shared with SCC.
// All of it float32 without contraction, no atomics, every sum in a fixed order: a train is bit-identical from run to run.
#include <cmath>
#include <new>

#include "xt_common.h"
#include "xt_qmix_dev.h"

namespace xt {

// ------------------------------------------------------------------ the fused head
// A hypernet row is [w1_raw (n E) | b1 (E) | wf_raw (E) | v (1)], P = n E + 2 E + 1 floats.
struct QmMix {
  const float* q_eval; const float* q_tgt;      // [T + 1, S, A] time-major
  const float* avail;                           // [B, T + 1, n, A]
  const int32_t* actions;                       // [B, T, n]
  const float* hyp_e; const float* hyp_t;       // [B T, P]
  const float *rewards, *terminated, *mask;     // [B T]
  const double* masksum;
  float gamma;
  int double_q, B, T, n, A, E;
  float* dq;                                    // [T + 1, S, A]
  float* dhyp;                                  // [B T, P]
  double* rowloss;                              // [B T]
  float* qtot;                                  // [B T, 2] (q_tot, y) or null
};

__device__ __forceinline__ float qm_wave_sum(float v) {
  for (int o = 32; o; o >>= 1) v = v + __shfl_xor(v, o);      // (a butterfly: every lane ends with the same bits)
  return v;
}
__device__ __forceinline__ float qm_sign(float x) { return x > 0.f ? 1.f : (x < 0.f ? -1.f : 0.f); }
__device__ __forceinline__ float qm_elu(float z) { return z > 0.f ? z : expm1f(z); }

__global__ __launch_bounds__(256) void qmix_mix_kernel(const QmMix a) {
  const int l = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= (long long)a.B * a.T) return;      // (a whole wavefront leaves; the kernel has no barrier)
  const int n = a.n, A = a.A, E = a.E, T = a.T, T1 = a.T + 1, S = a.B * a.n, P = n * E + 2 * E + 1;
  const int b = (int)(row / T), t = (int)(row % T);
  const float kMasked = -999999.0f;
  float ch = 0.f, tq = 0.f;
  int act = -1;
  if (l < n) {
    const int s = b * n + l;
    const float* qe0 = a.q_eval + ((long long)t * S + s) * A;
    const float* qe1 = a.q_eval + ((long long)(t + 1) * S + s) * A;
    const float* qt1 = a.q_tgt + ((long long)(t + 1) * S + s) * A;
    const float* av = a.avail + (((long long)b * T1 + t + 1) * n + l) * A;
    act = a.actions[((long long)b * T + t) * n + l];
    ch = act >= 0 && act < A ? qe0[act] : 0.f;  // (tf.one_hot: an index outside the depth makes a zero row)
    if (a.double_q) {
      float best = -INFINITY;
      int bi = 0;
      for (int k = 0; k < A; ++k) {
        const float m = av[k] == 0.f ? kMasked : qe1[k];
        if (m > best) { best = m; bi = k; }       // strict: the first index of a tie wins, as tf.argmax
      }
      tq = av[bi] == 0.f ? kMasked : qt1[bi];
    } else {
      float best = -INFINITY;
      for (int k = 0; k < A; ++k) best = fmaxf(best, av[k] == 0.f ? kMasked : qt1[k]);
      tq = best;
    }
  }
  const bool on = l < E;
  const int e = on ? l : E - 1;
  const float* he = a.hyp_e + row * P;
  const float* ht = a.hyp_t + row * P;
  float pre_e = 0.f, pre_t = 0.f;
  for (int k = 0; k < n; ++k) {
    const float ca = __shfl(ch, k), ta = __shfl(tq, k);
    pre_e = pre_e + ca * fabsf(he[k * E + e]);
    pre_t = pre_t + ta * fabsf(ht[k * E + e]);
  }
  pre_e = pre_e + he[n * E + e];
  pre_t = pre_t + ht[n * E + e];
  const float hid_e = qm_elu(pre_e), hid_t = qm_elu(pre_t);
  const float wf_raw = he[n * E + E + e];
  const float q_tot = qm_wave_sum(on ? hid_e * fabsf(wf_raw) : 0.f) + he[n * E + 2 * E];
  const float q_tot_t = qm_wave_sum(on ? hid_t * fabsf(ht[n * E + E + e]) : 0.f) + ht[n * E + 2 * E];
  const float y = a.rewards[row] + a.gamma * (1.f - a.terminated[row]) * q_tot_t;
  const float mk = a.mask[row];
  const float mtd = (q_tot - y) * mk;
  if (l == 0) {
    a.rowloss[row] = (double)mtd * (double)mtd;
    if (a.qtot) { a.qtot[row * 2] = q_tot; a.qtot[row * 2 + 1] = y; }
  }
  // ---- the eval mixer's backward; gq = d loss / d q_tot
  const float gq = (float)(2.0 * (double)(mtd * mk) / a.masksum[0]);
  const float dpre = gq * fabsf(wf_raw) * (pre_e > 0.f ? 1.f : hid_e + 1.f);
  float* dh = a.dhyp + row * P;
  if (on) {
    dh[n * E + E + e] = gq * hid_e * qm_sign(wf_raw);
    dh[n * E + e] = dpre;
  }
  if (l == 0) dh[n * E + 2 * E] = gq;
  float dch = 0.f;
  for (int k = 0; k < n; ++k) {
    const float ca = __shfl(ch, k);
    const float w1 = he[k * E + e];
    if (on) dh[k * E + e] = dpre * ca * qm_sign(w1);
    const float d = qm_wave_sum(on ? dpre * fabsf(w1) : 0.f);
    if (l == k) dch = d;
  }
  // ---- d q_eval as whole [n, A] rows of step t (and zero rows of the last step, which no chosen action reads)
  for (int base = 0; base < n * A; base += 64) {
    const int idx = base + l;
    const int k = idx < n * A ? idx / A : n - 1, c = idx % A;
    const float da = __shfl(dch, k);
    const int aa = __shfl(act, k);
    if (idx < n * A) {
      a.dq[((long long)t * S + b * n + k) * A + c] = c == aa ? da : 0.f;
      if (t == T - 1) a.dq[((long long)T * S + b * n + k) * A + c] = 0.f;
    }
  }
}

static int launch_mix(const QmMix& a, double* loss_out, hipStream_t st) {
  XT_REQUIRE(a.n >= 1 && a.n <= 32 && a.A >= 1 && a.A <= 64 && a.E >= 1 && a.E <= 64,
             "xt_qmix_mix: n_agents = %d, n_actions = %d, mixing_embed_dim = %d beyond the head kernel's limits (32, 64, 64)", a.n, a.A,
             a.E);
  XT_REQUIRE(a.B >= 1 && a.T >= 1 && (long long)a.B * a.T * (a.n * a.E + 2 * a.E + 1) < (1ll << 31) &&
             (long long)a.B * (a.T + 1) * a.n * a.A < (1ll << 31), "xt_qmix_mix: B = %d, T = %d out of range", a.B, a.T);
  XT_REQUIRE(a.q_eval && a.q_tgt && a.avail && a.actions && a.hyp_e && a.hyp_t && a.rewards && a.terminated && a.mask && a.masksum &&
             a.dq && a.dhyp && a.rowloss, "xt_qmix_mix: null argument");
  const long long rows = (long long)a.B * a.T;
  double* msum = const_cast<double*>(a.masksum);
  if (int rc = launch_dense_sum(a.mask, rows, nullptr, msum, st)) return rc;
  hipLaunchKernelGGL(qmix_mix_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, a);
  XT_LAUNCH_CHECK();
  if (loss_out) return launch_dense_sum((const double*)a.rowloss, rows, a.masksum, loss_out, st);
  return 0;
}

// TF's ApplyCenteredRMSProp (momentum 0) on g' = g * clip / max(||g||, clip); blockIdx.y = tensor
__global__ __launch_bounds__(256) void qmix_rmsprop_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ mg,
                                                           float* __restrict__ ms, const QmSegs s, const double* __restrict__ norm2,
                                                           float lr, float decay, float eps, float clip, float* __restrict__ state) {
  const int seg = blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;
  const float norm = (float)sqrt(norm2[seg]);
  if (i == 0) {
    state[8 + seg] = norm;
    if (seg == 0) state[0] = state[0] + 1.f;
  }
  if (i >= s.cnt[seg]) return;
  const long long o = (long long)s.off[seg] + i;
  const float gc = (g[o] * clip) / fmaxf(norm, clip);
  const float one_rho = 1.f - decay;
  const float ms1 = ms[o] + (gc * gc - ms[o]) * one_rho;
  const float mg1 = mg[o] + (gc - mg[o]) * one_rho;
  const float denom = (ms1 - mg1 * mg1) + eps;
  ms[o] = ms1;
  mg[o] = mg1;
  p[o] = p[o] - (lr * gc) / sqrtf(denom);
}

}  // namespace xt

// ------------------------------------------------------------------ the handle
struct xt_qmix {
  xt_qmix_desc d;
  int max_batch;
  int64_t off[xt::kQmTensors + 1];       // flat offsets of the 22 tensors; [22] = floats of one parameter set
  int cnt[xt::kQmTensors];
  float *pe, *pt, *grads, *mg, *ms, *state, *ws;
  int64_t ws_floats;
  // workspace offsets (floats); [2] = eval, target
  int64_t o_x1[2], o_xg[2], o_out[2], o_q[2], o_saved;
  int64_t o_ahw1[2], o_ahwf[2], o_av[2], o_hyp[2];
  int64_t o_dq, o_dout, o_dg3, o_dx1, o_dhyp, o_dahw1, o_dahwf, o_dav, o_slabs, o_rowloss, o_scalars;
};

namespace xt {

// (the agent's eight tensors AW1 .. AB2 come first)
enum { HW1K0 = kQmAgentTensors, HW1B0, HW1K1, HW1B1, HB1K, HB1B, HWFK0, HWFB0, HWFK1, HWFB1, HVK0, HVB0, HVK1, HVB1 };

static int qm_check_desc(const xt_qmix_desc& d, const char* who) {
  XT_REQUIRE(d.hidden == 32 || d.hidden == 64, "%s: rnn_hidden_dim = %d (the recurrent kernels take 32 or 64)", who, d.hidden);
  XT_REQUIRE(d.n_agents >= 1 && d.n_agents <= 32 && d.n_actions >= 1 && d.n_actions <= 64 && d.embed >= 1 && d.embed <= 64,
             "%s: n_agents = %d, n_actions = %d, mixing_embed_dim = %d beyond the head kernel's limits (32, 64, 64)", who, d.n_agents,
             d.n_actions, d.embed);
  XT_REQUIRE(d.obs_dim >= 1 && d.state_dim >= 1 && d.hyper_embed >= 1 && d.seq_len >= 1 && d.obs_dim <= 65536 && d.state_dim <= 65536 &&
             d.hyper_embed <= 4096 && d.seq_len <= 65536,
             "%s: obs_dim = %d, state_dim = %d, hypernet_embed = %d, seq_len = %d out of range", who, d.obs_dim, d.state_dim, d.hyper_embed,
             d.seq_len);
  return 0;
}

static void qm_layout(const xt_qmix_desc& d, int64_t* off, int* cnt) {
  const int D = d.obs_dim, H = d.hidden, A = d.n_actions, sd = d.state_dim, E = d.embed, HE = d.hyper_embed, n = d.n_agents;
  const int c[kQmTensors] = {D * H, H, 4 * H * H, 2 * H, 2 * H * H, H, H * A, A, sd * HE, HE, HE * E * n, E * n, sd * E, E,
                             sd * HE, HE, HE * E, E, sd * E, E, E, 1};
  int64_t o = 0;
  for (int i = 0; i < kQmTensors; ++i) {
    off[i] = o;
    if (cnt) cnt[i] = c[i];
    o += al4(c[i]);
  }
  off[kQmTensors] = o;
}

static void qm_plan(xt_qmix* z) {
  const xt_qmix_desc& d = z->d;
  const int64_t B = z->max_batch, T = d.seq_len, T1 = T + 1, n = d.n_agents, S = B * n, M = T1 * S, R = B * T;
  const int64_t H = d.hidden, A = d.n_actions, E = d.embed, HE = d.hyper_embed, P = n * E + 2 * E + 1, D = d.obs_dim, sd = d.state_dim;
  int64_t off = 0;
  auto take = [&](int64_t k) { const int64_t o = off; off += al4(k); return o; };
  for (int s = 0; s < 2; ++s) {
    z->o_x1[s] = take(M * H); z->o_xg[s] = take(M * 3 * H); z->o_out[s] = take(M * H); z->o_q[s] = take(M * A);
    z->o_ahw1[s] = take(R * HE); z->o_ahwf[s] = take(R * HE); z->o_av[s] = take(R * E); z->o_hyp[s] = take(R * P);
  }
  z->o_saved = take(M * 4 * H);
  z->o_dq = take(M * A); z->o_dout = take(M * H); z->o_dg3 = take(M * 3 * H); z->o_dx1 = take(M * H);
  z->o_dhyp = take(R * P); z->o_dahw1 = take(R * HE); z->o_dahwf = take(R * HE); z->o_dav = take(R * E);
  const int64_t km = (D > H ? D : H) + 1, nm = 2 * H > A ? 2 * H : A;
  int64_t kr = sd > HE ? sd : HE; kr = (kr > E ? kr : E) + 1;
  int64_t nr = HE > n * E ? HE : n * E;
  const int64_t sl_m = qm_nslab(M) * km * nm, sl_r = qm_nslab(R) * kr * nr;
  z->o_slabs = take(sl_m > sl_r ? sl_m : sl_r);
  z->o_rowloss = take(2 * R + 4);            // doubles
  z->o_scalars = take(2 * (kQmTensors + 2)); // doubles: [0] sum of the mask, [2 ..] the tensors' squared norms
  z->ws_floats = off;
}

// the agent's view of the handle: its tensors and its part of the workspace
static RnnAgent qm_agent(const xt_qmix* z) {
  RnnAgent g{};
  g.obs_dim = z->d.obs_dim; g.H = z->d.hidden; g.A = z->d.n_actions; g.n = z->d.n_agents;
  for (int i = 0; i < kQmAgentTensors; ++i) g.off[i] = z->off[i];
  float* ws = z->ws;
  for (int s = 0; s < 2; ++s) { g.x1[s] = ws + z->o_x1[s]; g.xg[s] = ws + z->o_xg[s]; g.out[s] = ws + z->o_out[s]; g.q[s] = ws + z->o_q[s]; }
  g.saved = ws + z->o_saved; g.dq = ws + z->o_dq; g.dout = ws + z->o_dout; g.dg3 = ws + z->o_dg3; g.dx1 = ws + z->o_dx1;
  g.slabs = ws + z->o_slabs;
  return g;
}

// y [R, N] at column `c0` of a [R, ldy] array = act(x . w + b) of Dense tensor pair (k, k + 1)
static int qm_dense(const xt_qmix* z, const float* p, int k, const float* x, int K, int R, int N, int relu, float* y, int ldy, hipStream_t st) {
  DenseGemm a{};
  a.x = x; a.ldx = K; a.K = K; a.w = p + z->off[k]; a.ldw = N; a.M = R; a.N = N; a.bias = p + z->off[k + 1]; a.relu = relu; a.y = y; a.ldy = ldy;
  return launch_dense_gemm(a, st);
}

static int qm_hyper_fwd(const xt_qmix* z, const float* p, int s, const float* state, int R, hipStream_t st) {
  const xt_qmix_desc& d = z->d;
  const int E = d.embed, HE = d.hyper_embed, n = d.n_agents, sd = d.state_dim, P = n * E + 2 * E + 1;
  float* ws = z->ws;
  float* hyp = ws + z->o_hyp[s];
  if (int rc = qm_dense(z, p, HW1K0, state, sd, R, HE, 1, ws + z->o_ahw1[s], HE, st)) return rc;
  if (int rc = qm_dense(z, p, HW1K1, ws + z->o_ahw1[s], HE, R, n * E, 0, hyp, P, st)) return rc;
  if (int rc = qm_dense(z, p, HB1K, state, sd, R, E, 0, hyp + n * E, P, st)) return rc;
  if (int rc = qm_dense(z, p, HWFK0, state, sd, R, HE, 1, ws + z->o_ahwf[s], HE, st)) return rc;
  if (int rc = qm_dense(z, p, HWFK1, ws + z->o_ahwf[s], HE, R, E, 0, hyp + n * E + E, P, st)) return rc;
  if (int rc = qm_dense(z, p, HVK0, state, sd, R, E, 1, ws + z->o_av[s], E, st)) return rc;
  return qm_dense(z, p, HVK1, ws + z->o_av[s], E, R, 1, 0, hyp + n * E + 2 * E, P, st);
}

// gradient of Dense pair (k, k + 1): dW = x^T dy, db = sum dy
static int qm_dense_wgrad(const xt_qmix* z, int k, const float* x, int K, const float* dy, int ldy, int R, int N, hipStream_t st) {
  DenseWgrad a{};
  a.x = x; a.ldx = K; a.dy = dy; a.ldy = ldy; a.M = R; a.K = K; a.N = N;
  return launch_dense_wgrad(a, z->grads + z->off[k], z->grads + z->off[k + 1], z->ws + z->o_slabs, kQmWgradRows, false, st);
}

// dx [R, K] = relu'(xact) * (dy . w^T) of Dense kernel k ([K, N])
static int qm_dense_dgrad(const xt_qmix* z, int k, const float* dy, int ldy, int R, int K, int N, const float* xact, float* dx, hipStream_t st) {
  DenseGemm a{};
  a.x = dy; a.ldx = ldy; a.K = N; a.w = z->pe + z->off[k]; a.ldw = N; a.wt = 1; a.M = R; a.N = K; a.maskx = xact; a.ldm = K; a.y = dx; a.ldy = K;
  return launch_dense_gemm(a, st);
}

}  // namespace xt

extern "C" {

int xt_qmix_layout(const xt_qmix_desc* desc, int64_t* offsets) {
  using namespace xt;
  XT_REQUIRE(desc && offsets, "xt_qmix_layout: null argument");
  if (int rc = qm_check_desc(*desc, "xt_qmix_layout")) return rc;
  qm_layout(*desc, offsets, nullptr);
  return 0;
}

int xt_qmix_create(const xt_qmix_desc* desc, int32_t max_batch, xt_qmix** out) {
  using namespace xt;
  XT_REQUIRE(desc && out, "xt_qmix_create: null argument");
  *out = nullptr;
  if (int rc = qm_check_desc(*desc, "xt_qmix_create")) return rc;
  XT_REQUIRE(max_batch >= 1 && max_batch <= (1 << 20), "xt_qmix_create: max_batch = %d outside [1, 2^20]", max_batch);
  const xt_qmix_desc& d = *desc;
  const long long M = (long long)(d.seq_len + 1) * max_batch * d.n_agents;
  long long widest = 4ll * d.hidden > d.obs_dim ? 4ll * d.hidden : d.obs_dim;
  widest = widest > d.n_actions ? widest : d.n_actions;
  const long long P = (long long)d.n_agents * d.embed + 2 * d.embed + 1;
  long long wr = P > d.hyper_embed ? P : d.hyper_embed;
  wr = wr > d.state_dim ? wr : d.state_dim;
  XT_REQUIRE(M * widest < (1ll << 31) && (long long)max_batch * d.seq_len * wr < (1ll << 31),
             "xt_qmix_create: (seq_len + 1) * max_batch * n_agents * %lld elements exceed 2^31", widest);
  xt_qmix* z = new (std::nothrow) xt_qmix();
  XT_REQUIRE(z, "xt_qmix_create: out of memory");
  z->d = d;
  z->max_batch = max_batch;
  qm_layout(d, z->off, z->cnt);
  qm_plan(z);
  *out = z;
  return 0;
}

void xt_qmix_destroy(xt_qmix* h) { delete h; }

int64_t xt_qmix_workspace_bytes(const xt_qmix* h) { return h ? h->ws_floats * 4 : 0; }

int xt_qmix_bind(xt_qmix* h, float* params_eval, float* params_target, float* grads, float* mg, float* ms, float* state, void* workspace,
                 int64_t workspace_bytes) {
  XT_REQUIRE(h && params_eval && params_target && grads && mg && ms && state && workspace, "xt_qmix_bind: null argument");
  XT_REQUIRE(workspace_bytes >= h->ws_floats * 4, "xt_qmix_bind: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
             (long long)h->ws_floats * 4);
  XT_REQUIRE((((uintptr_t)params_eval | (uintptr_t)params_target | (uintptr_t)grads | (uintptr_t)mg | (uintptr_t)ms | (uintptr_t)workspace) & 15) == 0,
             "xt_qmix_bind: buffers must be 16-byte aligned");
  h->pe = params_eval; h->pt = params_target; h->grads = grads; h->mg = mg; h->ms = ms; h->state = state;
  h->ws = static_cast<float*>(workspace);
  return 0;
}

int xt_qmix_step(xt_qmix* h, const float* obs, const int32_t* lens, const float* avail, const int32_t* actions, const float* state_cur,
                 const float* state_next, const float* rewards, const float* terminated, const float* mask, int32_t B,
                 const xt_qmix_cfg* cfg, double* loss_out, void* stream) {
  using namespace xt;
  if (int rc = check_bound(h, &xt_qmix::pe, B, "xt_qmix_step")) return rc;
  XT_REQUIRE(obs && avail && actions && state_cur && state_next && rewards && terminated && mask && cfg && loss_out,
             "xt_qmix_step: null argument");
  const xt_qmix* z = h;
  const xt_qmix_desc& d = z->d;
  const hipStream_t st = as_stream(stream);
  const int A = d.n_actions, n = d.n_agents, E = d.embed, HE = d.hyper_embed, sd = d.state_dim, T = d.seq_len, T1 = T + 1;
  const int R = B * T, P = n * E + 2 * E + 1;
  float* ws = z->ws;
  const RnnAgent ag = qm_agent(z);

  // ---- forward: both agents (one recurrent launch), both hypernets
  const float* const ps[2] = {z->pe, z->pt};
  if (int rc = agent_fwd(ag, ps, 2, obs, B, T1, nullptr, lens, true, nullptr, nullptr, st)) return rc;
  if (int rc = qm_hyper_fwd(z, z->pe, 0, state_cur, R, st)) return rc;
  if (int rc = qm_hyper_fwd(z, z->pt, 1, state_next, R, st)) return rc;

  // ---- the head: loss, d q, d hypernet outputs
  double* scal = reinterpret_cast<double*>(ws + z->o_scalars);
  QmMix m{};
  m.q_eval = ws + z->o_q[0]; m.q_tgt = ws + z->o_q[1]; m.avail = avail; m.actions = actions; m.hyp_e = ws + z->o_hyp[0];
  m.hyp_t = ws + z->o_hyp[1]; m.rewards = rewards; m.terminated = terminated; m.mask = mask; m.masksum = scal; m.gamma = cfg->gamma;
  m.double_q = d.double_q; m.B = B; m.T = T; m.n = n; m.A = A; m.E = E; m.dq = ws + z->o_dq; m.dhyp = ws + z->o_dhyp;
  m.rowloss = reinterpret_cast<double*>(ws + z->o_rowloss);
  if (int rc = launch_mix(m, loss_out, st)) return rc;

  // ---- the eval hypernets' backward
  const float* dhyp = ws + z->o_dhyp;
  if (int rc = qm_dense_wgrad(z, HW1K1, ws + z->o_ahw1[0], HE, dhyp, P, R, n * E, st)) return rc;
  if (int rc = qm_dense_dgrad(z, HW1K1, dhyp, P, R, HE, n * E, ws + z->o_ahw1[0], ws + z->o_dahw1, st)) return rc;
  if (int rc = qm_dense_wgrad(z, HW1K0, state_cur, sd, ws + z->o_dahw1, HE, R, HE, st)) return rc;
  if (int rc = qm_dense_wgrad(z, HB1K, state_cur, sd, dhyp + n * E, P, R, E, st)) return rc;
  if (int rc = qm_dense_wgrad(z, HWFK1, ws + z->o_ahwf[0], HE, dhyp + n * E + E, P, R, E, st)) return rc;
  if (int rc = qm_dense_dgrad(z, HWFK1, dhyp + n * E + E, P, R, HE, E, ws + z->o_ahwf[0], ws + z->o_dahwf, st)) return rc;
  if (int rc = qm_dense_wgrad(z, HWFK0, state_cur, sd, ws + z->o_dahwf, HE, R, HE, st)) return rc;
  if (int rc = qm_dense_wgrad(z, HVK1, ws + z->o_av[0], E, dhyp + n * E + 2 * E, P, R, 1, st)) return rc;
  if (int rc = qm_dense_dgrad(z, HVK1, dhyp + n * E + 2 * E, P, R, E, 1, ws + z->o_av[0], ws + z->o_dav, st)) return rc;
  if (int rc = qm_dense_wgrad(z, HVK0, state_cur, sd, ws + z->o_dav, E, R, E, st)) return rc;

  // ---- the eval agent's backward
  return agent_bwd(ag, z->pe, z->grads, obs, lens, B, T1, st);
}

int xt_qmix_apply(xt_qmix* h, const xt_qmix_cfg* cfg, void* stream) {
  using namespace xt;
  XT_REQUIRE(h && h->pe && h->ws && cfg, "xt_qmix_apply: the handle is not bound");
  XT_REQUIRE(cfg->grad_norm_clip > 0.f, "xt_qmix_apply: grad_norm_clip = %g is not positive", cfg->grad_norm_clip);
  QmSegs s{};
  s.n = kQmTensors;
  int widest = 0;
  for (int i = 0; i < kQmTensors; ++i) {
    s.off[i] = (int)h->off[i]; s.cnt[i] = h->cnt[i];
    widest = h->cnt[i] > widest ? h->cnt[i] : widest;
  }
  double* norm2 = reinterpret_cast<double*>(h->ws + h->o_scalars) + 2;
  const hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(qmix_norm_kernel, dim3(kQmTensors), dim3(256), 0, st, h->grads, s, norm2);
  XT_LAUNCH_CHECK();
  hipLaunchKernelGGL(qmix_rmsprop_kernel, dim3((unsigned)((widest + 255) / 256), kQmTensors), dim3(256), 0, st, h->pe, h->grads, h->mg,
                     h->ms, s, norm2, cfg->lr, cfg->decay, cfg->eps, cfg->grad_norm_clip, h->state);
  XT_LAUNCH_CHECK();
  return 0;
}

int xt_qmix_sync_target(xt_qmix* h, void* stream) {
  XT_REQUIRE(h && h->pe && h->pt, "xt_qmix_sync_target: the handle is not bound");
  XT_CHECK_HIP(hipMemcpyAsync(h->pt, h->pe, (size_t)h->off[xt::kQmTensors] * 4, hipMemcpyDeviceToDevice, xt::as_stream(stream)));
  return 0;
}

int xt_qmix_agent_forward(xt_qmix* h, const float* agent_params, const float* obs, int32_t B, int32_t T, const float* hidden_in,
                          const int32_t* lens, float* q, float* hidden_out, void* stream) {
  using namespace xt;
  if (int rc = check_bound(h, &xt_qmix::pe, B, "xt_qmix_agent_forward")) return rc;
  XT_REQUIRE(agent_params && obs && q, "xt_qmix_agent_forward: null argument");
  XT_REQUIRE(T >= 1 && T <= h->d.seq_len + 1, "xt_qmix_agent_forward: T = %d outside [1, %d]", T, h->d.seq_len + 1);
  return agent_fwd(qm_agent(h), &agent_params, 1, obs, B, T, hidden_in, lens, false, q, hidden_out, as_stream(stream));
}

int xt_qmix_gru_fwd(const float* wg, const float* wc, const float* xg, const float* h0, const int32_t* lens, int32_t T1, int32_t S,
                    int32_t H, float* saved, float* out, float* hT, void* stream) {
  using namespace xt;
  QmGruFwd a{};
  a.wg[0] = wg; a.wc[0] = wc; a.xg[0] = xg; a.h0[0] = h0; a.saved[0] = saved; a.out[0] = out; a.hT[0] = hT; a.lens = lens; a.T1 = T1; a.S = S;
  return launch_gru_fwd(a, H, 1, as_stream(stream));
}

int xt_qmix_gru_bwd(const float* wg, const float* wc, const float* saved, const float* h0, const float* dout, const float* dhT,
                    const int32_t* lens, int32_t T1, int32_t S, int32_t H, float* dg3, float* dh0, void* stream) {
  using namespace xt;
  QmGruBwd a{};
  a.wg = wg; a.wc = wc; a.saved = saved; a.h0 = h0; a.dout = dout; a.dhT = dhT; a.lens = lens; a.dg3 = dg3; a.dh0 = dh0; a.T1 = T1; a.S = S;
  return launch_gru_bwd(a, H, as_stream(stream));
}

int xt_qmix_mix(const float* q_eval, const float* q_tgt, const float* avail, const int32_t* actions, const float* hyp_eval,
                const float* hyp_tgt, const float* rewards, const float* terminated, const float* mask, int32_t B, int32_t T, int32_t n,
                int32_t A, int32_t E, float gamma, int32_t double_q, float* dq, float* dhyp, float* qtot, double* rowloss,
                double* masksum, double* loss_out, void* stream) {
  using namespace xt;
  QmMix a{};
  a.q_eval = q_eval; a.q_tgt = q_tgt; a.avail = avail; a.actions = actions; a.hyp_e = hyp_eval; a.hyp_t = hyp_tgt; a.rewards = rewards;
  a.terminated = terminated; a.mask = mask; a.masksum = masksum; a.gamma = gamma; a.double_q = double_q; a.B = B; a.T = T; a.n = n; a.A = A;
  a.E = E; a.dq = dq; a.dhyp = dhyp; a.rowloss = rowloss; a.qtot = qtot;
  return launch_mix(a, loss_out, as_stream(stream));
}

}  // extern "C"
