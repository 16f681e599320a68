// Device code shared by the QMIX and SCC learners (xt_qmix.hip, xt_scc.hip): the two persistent GRU kernels and their
// launchers, the plain Dense / weight-gradient kernels over stacked rows, the ordered float64 sum and the per-tensor norm.
// Every translation unit that includes this file gets its own copy (internal linkage).
#pragma once
#include <cmath>

#include "xt_common.h"

namespace xt {
namespace {

typedef float qm_f4 __attribute__((ext_vector_type(4)));
constexpr int kQmWgradRows = 512;       // rows of one weight-gradient slab
constexpr int kQmTensors = XT_QMIX_TENSORS;
constexpr int kQmAgentTensors = 8;

// time-major row r = t * S + b * n + a  ->  row (b * T + t) * n + a of a [B, T, n, .] array
__device__ __forceinline__ long long qm_bt_row(long long r, int S, int n, int T) {
  const int t = (int)(r / S), s = (int)(r % S);
  return ((long long)(s / n) * T + t) * n + s % n;
}

// ------------------------------------------------------------------ y = epilogue(x . w)
struct QmGemm {
  const float* x; int ldx;
  const float* w; int ldw; int wt;       // element (k, n) of the kernel at w[k * ldw + n], or (wt) at w[n * ldw + k]
  int M, K, N;
  const float* bias; int relu;
  const float* add;                      // [M, ldy] or null: y = add + acc (may be y itself)
  const float* maskx; int ldm;           // null, or y = 0 where maskx[m, n] <= 0
  float* y; int ldy;
  int imap, omap, S, n, T;               // imap / omap: x / y rows are [B, T, n, .] rows, m is time-major
};

__global__ __launch_bounds__(256) void qm_gemm_kernel(const QmGemm a) {
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long total = (long long)((a.M + 3) >> 2) * a.N;
  if (gid >= total) return;
  const int n = (int)(gid % a.N);
  const int m0 = (int)(gid / a.N) * 4;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  const float* xr[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const long long m = m0 + r < a.M ? m0 + r : a.M - 1;
    xr[r] = a.x + (a.imap ? qm_bt_row(m, a.S, a.n, a.T) : m) * a.ldx;
  }
  const long long wk = a.wt ? 1 : a.ldw, wn = a.wt ? a.ldw : 1;
  for (int k = 0; k < a.K; ++k) {
    const float wv = a.w[k * wk + n * wn];
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[r] = acc[r] + xr[r][k] * wv;
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int m = m0 + r;
    if (m >= a.M) break;
    float v = acc[r];
    const long long yr = a.omap ? qm_bt_row(m, a.S, a.n, a.T) : m;
    if (a.bias) v = v + a.bias[n];
    if (a.add) v = a.add[yr * a.ldy + n] + v;
    if (a.relu) v = v > 0.f ? v : 0.f;
    if (a.maskx && !(a.maskx[(long long)m * a.ldm + n] > 0.f)) v = 0.f;
    a.y[yr * a.ldy + n] = v;
  }
}

static int launch_qm_gemm(const QmGemm& a, hipStream_t st) {
  XT_REQUIRE(a.M > 0 && a.N > 0 && a.K > 0 && a.x && a.w && a.y, "qmix gemm: bad arguments");
  const long long total = (long long)((a.M + 3) >> 2) * a.N;
  XT_REQUIRE((total + 255) / 256 < (1ll << 31), "qmix gemm: too many outputs");
  hipLaunchKernelGGL(qm_gemm_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, a);
  XT_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------ dW = x^T . dy (+ db) over row slabs, then the slabs
struct QmWgrad {
  const float* x; int ldx;
  const float* xmul; int ldxm;           // null, or the x element is x * xmul (r o h of the candidate kernel)
  const float* dy; int ldy;
  int M, K, N, nslab, bias;
  int imap, S, n, T;
  float* out;                            // [nslab, (K + bias) * N]
};

__global__ __launch_bounds__(256) void qm_wgrad_kernel(const QmWgrad a) {
  const long long count = (long long)(a.K + a.bias) * a.N;
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  if (gid >= count * a.nslab) return;
  const int s = (int)(gid / count);
  const int e = (int)(gid % count);
  const int kk = e / a.N, n = e % a.N;
  const int r0 = s * kQmWgradRows;
  const int r1 = r0 + kQmWgradRows < a.M ? r0 + kQmWgradRows : a.M;
  float acc = 0.f;
  if (kk < a.K) {
    for (int r = r0; r < r1; ++r) {
      const long long xr = a.imap ? qm_bt_row(r, a.S, a.n, a.T) : r;
      float xv = a.x[xr * a.ldx + kk];
      if (a.xmul) xv = xv * a.xmul[(long long)r * a.ldxm + kk];
      acc = acc + xv * a.dy[(long long)r * a.ldy + n];
    }
  } else {
    for (int r = r0; r < r1; ++r) acc = acc + a.dy[(long long)r * a.ldy + n];
  }
  a.out[gid] = acc;
}

// dw[e] (e < nw) / db[e - nw] = sum over ascending s of slabs[s][e]
__global__ __launch_bounds__(256) void qm_slab_sum_kernel(const float* __restrict__ slabs, long long count, long long nw, int nslab,
                                                          float* __restrict__ dw, float* __restrict__ db) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= count) return;
  float acc = 0.f;
  for (int s = 0; s < nslab; ++s) acc = acc + slabs[(long long)s * count + e];
  if (e < nw) dw[e] = acc;
  else db[e - nw] = acc;
}

__global__ __launch_bounds__(256) void qm_fill_kernel(float* __restrict__ p, long long n, float v) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e < n) p[e] = v;
}

static inline int qm_nslab(long long M) { return (int)((M + kQmWgradRows - 1) / kQmWgradRows); }

// dw [K, N] and (db != null) db [N]; `slabs` holds qm_nslab(M) * (K + 1) * N floats.  M == 0: dw (and db) = 0.
static int launch_qm_wgrad(QmWgrad a, float* dw, float* db, float* slabs, hipStream_t st) {
  XT_REQUIRE(dw && slabs && a.K > 0 && a.N > 0 && a.M >= 0, "qmix wgrad: bad arguments");
  a.bias = db ? 1 : 0;
  const long long count = (long long)(a.K + a.bias) * a.N, nw = (long long)a.K * a.N;
  if (a.M == 0) {
    hipLaunchKernelGGL(qm_fill_kernel, dim3((unsigned)((nw + 255) / 256)), dim3(256), 0, st, dw, nw, 0.f);
    if (db) hipLaunchKernelGGL(qm_fill_kernel, dim3((unsigned)((a.N + 255) / 256)), dim3(256), 0, st, db, (long long)a.N, 0.f);
    XT_LAUNCH_CHECK();
    return 0;
  }
  XT_REQUIRE(a.x && a.dy, "qmix wgrad: bad arguments");
  a.nslab = qm_nslab(a.M);
  a.out = slabs;
  XT_REQUIRE((count * a.nslab + 255) / 256 < (1ll << 31), "qmix wgrad: too large");
  hipLaunchKernelGGL(qm_wgrad_kernel, dim3((unsigned)((count * a.nslab + 255) / 256)), dim3(256), 0, st, a);
  XT_LAUNCH_CHECK();
  hipLaunchKernelGGL(qm_slab_sum_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st, slabs, count, nw, a.nslab, dw, db);
  XT_LAUNCH_CHECK();
  return 0;
}

// out[0] = (sum of n values, thread t takes t, t + 256, ... ascending, then a fixed tree) / (div ? div[0] : 1)
template <typename T>
__global__ __launch_bounds__(256) void qm_sum_kernel(const T* __restrict__ src, long long n, const double* __restrict__ div,
                                                     double* __restrict__ out) {
  __shared__ double sh[256];
  double acc = 0.0;
  for (long long i = threadIdx.x; i < n; i += 256) acc += (double)src[i];
  sh[threadIdx.x] = acc;
  __syncthreads();
  for (int o = 128; o; o >>= 1) {
    if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = div ? sh[0] / div[0] : sh[0];
}

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

// ------------------------------------------------------------------ centred RMSProp, tf.clip_by_norm per tensor
struct QmSegs {
  int n;
  int off[kQmTensors], cnt[kQmTensors];
};

// norm2[i] = sum of squares of tensor i: thread t takes t, t + 256, ... ascending in float64, then a fixed tree
__global__ __launch_bounds__(256) void qmix_norm_kernel(const float* __restrict__ g, const QmSegs s, double* __restrict__ norm2) {
  __shared__ double sh[256];
  const float* p = g + s.off[blockIdx.x];
  const int cnt = s.cnt[blockIdx.x];
  double acc = 0.0;
  for (int i = threadIdx.x; i < cnt; i += 256) acc += (double)p[i] * (double)p[i];
  sh[threadIdx.x] = acc;
  __syncthreads();
  for (int o = 128; o; o >>= 1) {
    if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) norm2[blockIdx.x] = sh[0];
}

}  // namespace
}  // namespace xt
