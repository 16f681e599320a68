// Device code shared by the QMIX and SCC learners (xt_qmix.hip, xt_scc.hip): the two persistent GRU kernels and their
// launchers, the Dense -> GRU -> Dense agent built from them and the plain Dense kernels of xt_dense_dev.h (agent_fwd,
// agent_bwd), and the per-tensor norm.
// Every translation unit that includes this file gets its own copy (internal linkage).
#pragma once
#include <cmath>

#include "xt_common.h"
#include "xt_dense_dev.h"

namespace xt {
namespace {

typedef float qm_f4 __attribute__((ext_vector_type(4)));
constexpr int kQmWgradRows = 512;       // rows of one weight-gradient slab
constexpr int kQmTensors = XT_QMIX_TENSORS;
constexpr int kQmAgentTensors = 8;

static inline int qm_nslab(long long M) { return dense_nslab(M, kQmWgradRows); }

// ------------------------------------------------------------------ the persistent GRU forward
// Tile = 16 sequences x all T1 steps; H / 16 wavefronts, wavefront w owns the hidden columns [16 w, 16 w + 16) of r, u and c.
// v_mfma_f32_16x16x4_f32: lane l holds A[i = l % 16][k = l / 16], B[k = l / 16][j = l % 16], D[i = 4 (l / 16) + v][j = l % 16].
// The 16-row instruction (not the 32x32x2 one): the batch of the shipped example is 64 sequences, 16-row tiles make 4 workgroups
// per parameter set instead of 2, and a 32-row tile would double the serial MFMA chain of every step (the step is latency-bound:
// H / 4 dependent instructions per accumulator either way) without using more of the machine.
struct QmGruFwd {
  const float* wg[2];                    // [2H, 2H] gates kernel: rows [H, 2H) are the recurrent half, columns r | u
  const float* wc[2];                    // [2H, H] candidate kernel
  const float* xg[2];                    // [T1, S, 3H]: x . Wg[:H] + bg | x . Wc[:H] + bc
  const float* h0[2];                    // [S, H] or null (zero)
  float* saved[2];                       // [T1, S, 4H] r | u | c | h' (the carried state past the length) or null
  float* out[2];                         // [T1, S, H]: h', zero past the length
  float* hT[2];                          // [S, H] or null
  const int32_t* lens;                   // [S] or null (all T1)
  int T1, S;
};

__device__ __forceinline__ float qm_sigmoid(float z) { return 1.f / (1.f + expf(-z)); }

template <int H>
__global__ __launch_bounds__(H * 4) void qmix_gru_fwd_kernel(const QmGruFwd a) {
  constexpr int LD = H + 1, KS = H / 4;
  __shared__ float hs[2][16 * LD];
  __shared__ float rh[16 * LD];
  const int set = blockIdx.y, w = threadIdx.x >> 6, l = threadIdx.x & 63;
  const int j = l & 15, g = l >> 4, col = 16 * w + j, s0 = blockIdx.x * 16;
  const int T1 = a.T1, S = a.S;
  const float* __restrict__ wg = a.wg[set];
  const float* __restrict__ wc = a.wc[set];
  const float* __restrict__ xg = a.xg[set];
  float* __restrict__ saved = a.saved[set];
  float* __restrict__ out = a.out[set];
  float br[KS], bu[KS], bc[KS];
#pragma unroll
  for (int kk = 0; kk < KS; ++kk) {
    const int k = H + 4 * kk + g;
    br[kk] = wg[k * 2 * H + col];
    bu[kk] = wg[k * 2 * H + H + col];
    bc[kk] = wc[k * H + col];
  }
  int row[4], ln[4];
  bool ok[4];
  float h[4];
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    const int s = s0 + 4 * g + v;
    ok[v] = s < S;
    row[v] = ok[v] ? s : S - 1;
    ln[v] = a.lens ? a.lens[row[v]] : T1;
    h[v] = a.h0[set] ? a.h0[set][(long long)row[v] * H + col] : 0.f;
    hs[0][(4 * g + v) * LD + col] = h[v];
  }
  __syncthreads();
  int cur = 0;
  for (int t = 0; t < T1; ++t) {
    qm_f4 ar, au, ac;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const float* base = xg + ((long long)t * S + row[v]) * 3 * H;
      ar[v] = base[col]; au[v] = base[H + col]; ac[v] = base[2 * H + col];
    }
#pragma unroll
    for (int kk = 0; kk < KS; ++kk) {
      const float av = hs[cur][j * LD + 4 * kk + g];
      ar = __builtin_amdgcn_mfma_f32_16x16x4f32(av, br[kk], ar, 0, 0, 0);
      au = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bu[kk], au, 0, 0, 0);
    }
    float r[4], u[4];
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      r[v] = qm_sigmoid(ar[v]);
      u[v] = qm_sigmoid(au[v]);
      rh[(4 * g + v) * LD + col] = r[v] * h[v];
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < KS; ++kk) ac = __builtin_amdgcn_mfma_f32_16x16x4f32(rh[j * LD + 4 * kk + g], bc[kk], ac, 0, 0, 0);
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const float c = tanhf(ac[v]);
      const float hn = u[v] * h[v] + (1.f - u[v]) * c;
      const bool valid = t < ln[v];
      const float keep = valid ? hn : h[v];
      const long long o = (long long)t * S + row[v];
      if (ok[v]) {
        if (saved) {
          float* sv = saved + o * 4 * H;
          sv[col] = r[v]; sv[H + col] = u[v]; sv[2 * H + col] = c; sv[3 * H + col] = keep;
        }
        out[o * H + col] = valid ? hn : 0.f;
      }
      h[v] = keep;
      hs[cur ^ 1][(4 * g + v) * LD + col] = keep;
    }
    __syncthreads();
    cur ^= 1;
  }
  if (a.hT[set]) {
#pragma unroll
    for (int v = 0; v < 4; ++v)
      if (ok[v]) a.hT[set][(long long)row[v] * H + col] = h[v];
  }
}

static int launch_gru_fwd(const QmGruFwd& a, int H, int nset, hipStream_t st) {
  XT_REQUIRE(H == 32 || H == 64, "xt_qmix: rnn_hidden_dim = %d (the recurrent kernels take 32 or 64)", H);
  XT_REQUIRE(a.T1 >= 1 && a.S >= 1 && (long long)a.T1 * a.S * 4 * H < (1ll << 31), "xt_qmix_gru_fwd: T1 = %d, S = %d out of range",
             a.T1, a.S);
  for (int s = 0; s < nset; ++s) XT_REQUIRE(a.wg[s] && a.wc[s] && a.xg[s] && a.out[s], "xt_qmix_gru_fwd: null argument");
  const dim3 grid((unsigned)((a.S + 15) / 16), (unsigned)nset);
  if (H == 64) hipLaunchKernelGGL(qmix_gru_fwd_kernel<64>, grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL(qmix_gru_fwd_kernel<32>, grid, dim3(128), 0, st, a);
  XT_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------ the persistent BPTT
// Same tiling, t downward.  The carried dh is elementwise in the accumulator layout: it stays in the lane's registers.  The LDS
// tiles (dc_pre, [dr_pre | du_pre]) alternate between two buffers by the parity of t, which leaves two barriers per step.
struct QmGruBwd {
  const float* wg; const float* wc;
  const float* saved;                    // [T1, S, 4H]
  const float* h0;                       // [S, H] or null
  const float* dout;                     // [T1, S, H]: gradient of `out`
  const float* dhT;                      // [S, H] or null: gradient of the final state
  const int32_t* lens;
  float* dg3;                            // [T1, S, 3H]: dr_pre | du_pre | dc_pre
  float* dh0;                            // [S, H] or null
  int T1, S;
};

template <int H>
__global__ __launch_bounds__(H * 4) void qmix_gru_bwd_kernel(const QmGruBwd a) {
  constexpr int LD = H + 1, LDG = 2 * H + 1, KS = H / 4;
  __shared__ float dcs[2][16 * LD];
  __shared__ float dgs[2][16 * LDG];
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  const int j = l & 15, g = l >> 4, col = 16 * w + j, s0 = blockIdx.x * 16;
  const int T1 = a.T1, S = a.S;
  // transposed fragments: B[k][j] = W[H + col][k]
  float bct[KS], bgt[2 * KS];
#pragma unroll
  for (int kk = 0; kk < KS; ++kk) bct[kk] = a.wc[(H + col) * H + 4 * kk + g];
#pragma unroll
  for (int kk = 0; kk < 2 * KS; ++kk) bgt[kk] = a.wg[(H + col) * 2 * H + 4 * kk + g];
  int row[4], ln[4];
  bool ok[4];
  float dh[4];
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    const int s = s0 + 4 * g + v;
    ok[v] = s < S;
    row[v] = ok[v] ? s : S - 1;
    ln[v] = a.lens ? a.lens[row[v]] : T1;
    dh[v] = a.dhT ? a.dhT[(long long)row[v] * H + col] : 0.f;
  }
  for (int t = T1 - 1; t >= 0; --t) {
    const int p = t & 1;
    float r[4], u[4], hp[4], dt[4], dup[4], dcp[4], drp[4];
    bool valid[4];
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const long long o = (long long)t * S + row[v];
      const float* sv = a.saved + o * 4 * H;
      r[v] = sv[col]; u[v] = sv[H + col];
      const float c = sv[2 * H + col];
      hp[v] = t > 0 ? (sv - (long long)S * 4 * H)[3 * H + col] : (a.h0 ? a.h0[(long long)row[v] * H + col] : 0.f);
      valid[v] = ok[v] && t < ln[v];
      dt[v] = dh[v] + a.dout[o * H + col];
      dup[v] = valid[v] ? dt[v] * (hp[v] - c) * (u[v] * (1.f - u[v])) : 0.f;
      dcp[v] = valid[v] ? dt[v] * (1.f - u[v]) * (1.f - c * c) : 0.f;
      dcs[p][(4 * g + v) * LD + col] = dcp[v];
      dgs[p][(4 * g + v) * LDG + H + col] = dup[v];
    }
    __syncthreads();
    qm_f4 drh = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < KS; ++kk) drh = __builtin_amdgcn_mfma_f32_16x16x4f32(dcs[p][j * LD + 4 * kk + g], bct[kk], drh, 0, 0, 0);
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      drp[v] = valid[v] ? drh[v] * hp[v] * (r[v] * (1.f - r[v])) : 0.f;
      dgs[p][(4 * g + v) * LDG + col] = drp[v];
    }
    __syncthreads();
    qm_f4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < 2 * KS; ++kk) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(dgs[p][j * LDG + 4 * kk + g], bgt[kk], acc, 0, 0, 0);
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      if (valid[v]) dh[v] = dt[v] * u[v] + drh[v] * r[v] + acc[v];
      if (ok[v]) {
        float* d = a.dg3 + ((long long)t * S + row[v]) * 3 * H;
        d[col] = drp[v]; d[H + col] = dup[v]; d[2 * H + col] = dcp[v];
      }
    }
  }
  if (a.dh0) {
#pragma unroll
    for (int v = 0; v < 4; ++v)
      if (ok[v]) a.dh0[(long long)row[v] * H + col] = dh[v];
  }
}

static int launch_gru_bwd(const QmGruBwd& a, int H, hipStream_t st) {
  XT_REQUIRE(H == 32 || H == 64, "xt_qmix: rnn_hidden_dim = %d (the recurrent kernels take 32 or 64)", H);
  XT_REQUIRE(a.T1 >= 1 && a.S >= 1 && (long long)a.T1 * a.S * 4 * H < (1ll << 31), "xt_qmix_gru_bwd: T1 = %d, S = %d out of range",
             a.T1, a.S);
  XT_REQUIRE(a.wg && a.wc && a.saved && a.dout && a.dg3, "xt_qmix_gru_bwd: null argument");
  const dim3 grid((unsigned)((a.S + 15) / 16));
  if (H == 64) hipLaunchKernelGGL(qmix_gru_bwd_kernel<64>, grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL(qmix_gru_bwd_kernel<32>, grid, dim3(128), 0, st, a);
  XT_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------ the recurrent agent: dense (relu) -> GRU -> dense_1
enum { AW1, AB1, AWG, ABG, AWC, ABC, AW2, AB2 };      // its eight tensors, the first eight of a parameter set

struct RnnAgent {
  int obs_dim, H, A, n;
  int64_t off[kQmAgentTensors];          // flat offsets of the tensors in a parameter set (and in the gradient)
  float *x1[2], *xg[2], *out[2], *q[2];  // per parameter set of one forward: [M, H], [M, 3H], [M, H], [M, A], M = T1 S time-major
  float *saved;                          // [M, 4H] of set 0
  float *dq, *dout, *dg3, *dx1, *slabs;  // the backward's: [M, A], [M, H], [M, 3H], [M, H], qm_nslab(M) weight-gradient slabs
};

// the forward of `nset` parameter sets (one recurrent launch) over B episodes of T1 steps: q [T1, S, A] time-major per set (or,
// `q_bt`, one set into a [B, T1, n, A] array)
static int agent_fwd(const RnnAgent& g, const float* const* ps, int nset, const float* obs, int B, int T1, const float* h0,
                     const int32_t* lens, bool save, float* q_bt, float* hT, hipStream_t st) {
  const int H = g.H, A = g.A, S = B * g.n, M = T1 * S;
  QmGruFwd gf{};
  for (int s = 0; s < nset; ++s) {
    const float* p = ps[s];
    DenseGemm a{};
    a.x = obs; a.ldx = g.obs_dim; a.K = g.obs_dim; a.w = p + g.off[AW1]; a.ldw = H; a.M = M; a.N = H; a.bias = p + g.off[AB1];
    a.relu = 1; a.y = g.x1[s]; a.ldy = H; a.imap = 1; a.S = S; a.n = g.n; a.T = T1;
    if (int rc = launch_dense_gemm(a, st)) return rc;
    DenseGemm x{};
    x.x = g.x1[s]; x.ldx = H; x.K = H; x.w = p + g.off[AWG]; x.ldw = 2 * H; x.M = M; x.N = 2 * H; x.bias = p + g.off[ABG];
    x.y = g.xg[s]; x.ldy = 3 * H;
    if (int rc = launch_dense_gemm(x, st)) return rc;
    x.w = p + g.off[AWC]; x.ldw = H; x.N = H; x.bias = p + g.off[ABC]; x.y = g.xg[s] + 2 * H;
    if (int rc = launch_dense_gemm(x, st)) return rc;
    gf.wg[s] = p + g.off[AWG]; gf.wc[s] = p + g.off[AWC]; gf.xg[s] = g.xg[s]; gf.h0[s] = h0;
    gf.saved[s] = save && s == 0 ? g.saved : nullptr; gf.out[s] = g.out[s]; gf.hT[s] = hT;
  }
  gf.lens = lens; gf.T1 = T1; gf.S = S;
  if (int rc = launch_gru_fwd(gf, H, nset, st)) return rc;
  for (int s = 0; s < nset; ++s) {
    const float* p = ps[s];
    DenseGemm a{};
    a.x = g.out[s]; a.ldx = H; a.K = H; a.w = p + g.off[AW2]; a.ldw = A; a.M = M; a.N = A; a.bias = p + g.off[AB2];
    a.y = q_bt ? q_bt : g.q[s]; a.ldy = A; a.omap = q_bt ? 1 : 0; a.S = S; a.n = g.n; a.T = T1;
    if (int rc = launch_dense_gemm(a, st)) return rc;
  }
  return 0;
}

// the backward of parameter set `p` (set 0 of a saving forward) from dq [T1, S, A] into `gr`: dense_1, BPTT, then everything over
// the stacked rows
static int agent_bwd(const RnnAgent& g, const float* p, float* gr, const float* obs, const int32_t* lens, int B, int T1, hipStream_t st) {
  const int H = g.H, A = g.A, S = B * g.n, M = T1 * S;
  const float *x1 = g.x1[0], *saved = g.saved, *dg3 = g.dg3;
  auto wgrad = [&](const DenseWgrad& a, int k, int row0, bool bias) {
    return launch_dense_wgrad(a, gr + g.off[k] + row0 * a.N, bias ? gr + g.off[k + 1] : nullptr, g.slabs, kQmWgradRows, false, st);
  };
  DenseWgrad w2{};
  w2.x = g.out[0]; w2.ldx = H; w2.dy = g.dq; w2.ldy = A; w2.M = M; w2.K = H; w2.N = A;
  if (int rc = wgrad(w2, AW2, 0, true)) return rc;
  DenseGemm dx{};     // d out = dq . W2^T
  dx.x = g.dq; dx.ldx = A; dx.K = A; dx.w = p + g.off[AW2]; dx.ldw = A; dx.wt = 1; dx.M = M; dx.N = H; dx.y = g.dout; dx.ldy = H;
  if (int rc = launch_dense_gemm(dx, st)) return rc;
  QmGruBwd gb{};
  gb.wg = p + g.off[AWG]; gb.wc = p + g.off[AWC]; gb.saved = saved; gb.dout = g.dout; gb.lens = lens; gb.dg3 = g.dg3; gb.T1 = T1; gb.S = S;
  if (int rc = launch_gru_bwd(gb, H, st)) return rc;
  DenseWgrad a{};     // gates kernel, input rows (and the bias); then the recurrent rows: h_{t-1} is the saved state one step up
  a.x = x1; a.ldx = H; a.dy = dg3; a.ldy = 3 * H; a.M = M; a.K = H; a.N = 2 * H;
  if (int rc = wgrad(a, AWG, 0, true)) return rc;
  a.x = saved + 3 * H; a.ldx = 4 * H; a.dy = dg3 + (long long)S * 3 * H; a.M = M - S;
  if (int rc = wgrad(a, AWG, H, false)) return rc;
  DenseWgrad c{};     // candidate kernel: input rows (and the bias), then r o h_{t-1}
  c.x = x1; c.ldx = H; c.dy = dg3 + 2 * H; c.ldy = 3 * H; c.M = M; c.K = H; c.N = H;
  if (int rc = wgrad(c, AWC, 0, true)) return rc;
  c.x = saved + 3 * H; c.ldx = 4 * H; c.xmul = saved + (long long)S * 4 * H; c.ldxm = 4 * H; c.dy = dg3 + (long long)S * 3 * H + 2 * H;
  c.M = M - S;
  if (int rc = wgrad(c, AWC, H, false)) return rc;
  DenseGemm e{};      // d x1 = relu'(x1) * ([dr | du] . Wg[:H]^T + dc . Wc[:H]^T)
  e.x = dg3; e.ldx = 3 * H; e.K = 2 * H; e.w = p + g.off[AWG]; e.ldw = 2 * H; e.wt = 1; e.M = M; e.N = H; e.y = g.dx1; e.ldy = H;
  if (int rc = launch_dense_gemm(e, st)) return rc;
  e.x = dg3 + 2 * H; e.K = H; e.w = p + g.off[AWC]; e.ldw = H; e.add = g.dx1; e.maskx = x1; e.ldm = H;
  if (int rc = launch_dense_gemm(e, st)) return rc;
  DenseWgrad w1{};
  w1.x = obs; w1.ldx = g.obs_dim; w1.dy = g.dx1; w1.ldy = H; w1.M = M; w1.K = g.obs_dim; w1.N = H; w1.imap = 1; w1.S = S; w1.n = g.n;
  w1.T = T1;
  return wgrad(w1, AW1, 0, true);
}

// ------------------------------------------------------------------ centred RMSProp, tf.clip_by_norm per tensor
struct QmSegs {
  int n;
  int off[kQmTensors], cnt[kQmTensors];
};

// norm2[i] = sum of squares of tensor i: thread t takes t, t + 256, ... ascending in float64, then a fixed tree
__global__ __launch_bounds__(256) void qmix_norm_kernel(const float* __restrict__ g, const QmSegs s, double* __restrict__ norm2) {
  const float* p = g + s.off[blockIdx.x];
  const int cnt = s.cnt[blockIdx.x];
  double acc = 0.0;
  for (int i = threadIdx.x; i < cnt; i += 256) acc += (double)p[i] * (double)p[i];
  const double sum = dense_tree_sum(acc);
  if (threadIdx.x == 0) norm2[blockIdx.x] = sum;
}

}  // namespace
}  // namespace xt
