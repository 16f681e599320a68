// MuZero: the K-step unrolled model update (xt_mz_* of include/xt_mi355x.h).
//
// The representation chain (Dense layers on float32 observations) runs on the trunk-layer kernels of xt_igemm.hip
// (launch_fwd, xt_layer_bwd, xt_layer_wgrad_slabs).  Everything behind it is Dense layers of any width (supports of 3, 7, 26, 305 columns, hidden
// states of 4) over the STACKED rows of all unroll steps, on the kernels of this file:
//   mz_gemm_kernel      y = epilogue(x . w): forward (conditioning row + bias + relu) or input gradient (on the transposed
//                       kernel: join term + scale + relu mask)
//   mz_wgrad_kernel     dW / db over row slabs of XT_MZ_WGRAD_ROWS rows, with the gathered rows of the conditioned layer
//   mz_loss_kernel      softmax + two-hot / dense target + cross-entropy + d(logits)
// All of them float32 without contraction (the build's -ffp-contract=off), sums in ascending order: the NumPy twins of the
// tests reproduce them bit for bit.
#include <cmath>
#include <new>

#include "xt_common.h"
#include "xt_launch.h"

namespace xt {

// ------------------------------------------------------------------ y[m, n] = epilogue(sum_k x[m, k] w[k, n])
// One thread owns 4 consecutive rows of one column (the w element is loaded once for the four); consecutive threads own
// consecutive columns, so w loads coalesce and x loads are a few broadcast addresses per wavefront.
struct MzGemm {
  const float* x; int ldx;        // [M, ldx], K columns read
  const float* w;                 // [K (+ A), N]
  int M, K, N;
  // forward epilogue
  const float* bias;              // [N] or null
  const int32_t* actions;         // null, or the conditioning: row r = i * B + b adds w[K + actions[b * a_stride + i]]
  int a_stride, B, A;
  int relu;
  // input-gradient epilogue (MODE 1): y = mask(maskx) * (add + c * acc)
  const float* add;               // [M, N] or null
  float c;
  const float* maskx;             // [M, N] or null: y = 0 where maskx <= 0
  float* y;                       // [M, N]
};

template <int MODE>
__global__ __launch_bounds__(256) void mz_gemm_kernel(const MzGemm a) {
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long total = (long long)((a.M + 3) >> 2) * a.N;
  if (gid >= total) return;
  const int n = (int)(gid % a.N);
  const int m0 = (int)(gid / a.N) * 4;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  const float* xr[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) xr[r] = a.x + (long long)(m0 + r < a.M ? m0 + r : a.M - 1) * a.ldx;
  for (int k = 0; k < a.K; ++k) {
    const float wv = a.w[(long long)k * a.N + n];
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[r] = acc[r] + xr[r][k] * wv;
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int m = m0 + r;
    if (m >= a.M) break;
    float v = acc[r];
    if (MODE == 0) {
      if (a.actions) {
        const int act = a.actions[(long long)(m % a.B) * a.a_stride + m / a.B];
        if (act >= 0 && act < a.A) v = v + a.w[(long long)(a.K + act) * a.N + n];
      }
      if (a.bias) v = v + a.bias[n];
      if (a.relu) v = v > 0.f ? v : 0.f;
    } else {
      v = a.c * v;
      if (a.add) v = a.add[(long long)m * a.N + n] + v;
      if (a.maskx && !(a.maskx[(long long)m * a.N + n] > 0.f)) v = 0.f;
    }
    a.y[(long long)m * a.N + n] = v;
  }
}

template <int MODE>
static int launch_gemm(const MzGemm& a, hipStream_t st) {
  XT_REQUIRE(a.M > 0 && a.N > 0 && a.K >= 0 && a.y && (a.K == 0 || (a.x && a.w)), "mz gemm: bad arguments");
  const long long total = (long long)((a.M + 3) >> 2) * a.N;
  XT_REQUIRE((total + 255) / 256 < (1ll << 31), "mz gemm: too many outputs");
  hipLaunchKernelGGL(mz_gemm_kernel<MODE>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, a);
  XT_LAUNCH_CHECK();
  return 0;
}

// wt[n, k] = w[k, n] for k < K (the first K rows of a [rows, N] kernel): the input gradient then runs as a forward
__global__ __launch_bounds__(256) void mz_transpose_kernel(const float* __restrict__ w, int K, int N, float* __restrict__ wt) {
  const int gid = blockIdx.x * 256 + threadIdx.x;
  if (gid >= K * N) return;
  const int k = gid % K, n = gid / K;
  wt[gid] = w[(long long)k * N + n];
}
static int launch_transpose(const float* w, int K, int N, float* wt, hipStream_t st) {
  XT_REQUIRE(w && wt && K > 0 && N > 0 && (long long)K * N < (1ll << 31), "mz transpose: bad arguments");
  hipLaunchKernelGGL(mz_transpose_kernel, dim3((K * N + 255) / 256), dim3(256), 0, st, w, K, N, wt);
  XT_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------ weight + bias gradient over row slabs
// out[s][kk, n] for kk in [0, K + A]: kk < K: sum_r x[r, kk] dy[r, n]; K <= kk < K + A: sum over the rows whose action is
// kk - K of dy[r, n] (zero when nobody took it); kk == K + A: sum_r dy[r, n].  Rows [s * chunk, (s + 1) * chunk) ascending.
struct MzWgrad {
  const float* x; int ldx;
  const float* dy;
  const int32_t* actions; int a_stride, B, A;
  int M, K, N, nslab;
  float* out;                     // [nslab, (K + A + 1) * N]
};

__global__ __launch_bounds__(256) void mz_wgrad_kernel(const MzWgrad a) {
  const long long count = (long long)(a.K + a.A + 1) * a.N;
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  if (gid >= count * a.nslab) return;
  const int s = (int)(gid / count);
  const int e = (int)(gid % count);
  const int kk = e / a.N, n = e % a.N;
  const int r0 = s * XT_MZ_WGRAD_ROWS;
  const int r1 = r0 + XT_MZ_WGRAD_ROWS < a.M ? r0 + XT_MZ_WGRAD_ROWS : a.M;
  float acc = 0.f;
  if (kk < a.K) {
    int r = r0;
    for (; r + 4 <= r1; r += 4) {      // four rows' loads in flight, added in ascending order
      float xv[4], dv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        xv[u] = a.x[(long long)(r + u) * a.ldx + kk];
        dv[u] = a.dy[(long long)(r + u) * a.N + n];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) acc = acc + xv[u] * dv[u];
    }
    for (; r < r1; ++r) acc = acc + a.x[(long long)r * a.ldx + kk] * a.dy[(long long)r * a.N + n];
  } else if (kk < a.K + a.A) {
    const int want = kk - a.K;
    for (int r = r0; r < r1; ++r)
      if (a.actions[(long long)(r % a.B) * a.a_stride + r / a.B] == want) acc = acc + a.dy[(long long)r * a.N + n];
  } else {
    for (int r = r0; r < r1; ++r) acc = acc + a.dy[(long long)r * a.N + n];
  }
  a.out[gid] = acc;
}

// dwb[e] = sum over ascending s of slabs[s][e]
__global__ __launch_bounds__(256) void mz_slab_sum_kernel(const float* __restrict__ slabs, long long count, int nslab,
                                                          float* __restrict__ dwb) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= count) return;
  float acc = 0.f;
  for (int s = 0; s < nslab; ++s) acc = acc + slabs[(long long)s * count + e];
  dwb[e] = acc;
}

static inline int mz_nslab(int M) { return (M + XT_MZ_WGRAD_ROWS - 1) / XT_MZ_WGRAD_ROWS; }

// a: out is ignored; dwb receives the gradient, `slabs` holds mz_nslab(M) slabs when that is more than one
static int launch_mz_wgrad(MzWgrad a, float* dwb, float* slabs, hipStream_t st) {
  XT_REQUIRE(a.x && a.dy && dwb && a.M > 0 && a.K > 0 && a.N > 0 && a.A >= 0 && (a.A == 0 || (a.actions && a.B > 0)),
             "mz wgrad: bad arguments");
  a.nslab = mz_nslab(a.M);
  XT_REQUIRE(a.nslab == 1 || slabs, "mz wgrad: %d rows need a slab buffer", a.M);
  const long long count = (long long)(a.K + a.A + 1) * a.N;
  XT_REQUIRE((count * a.nslab + 255) / 256 < (1ll << 31), "mz wgrad: too large");
  a.out = a.nslab == 1 ? dwb : slabs;
  hipLaunchKernelGGL(mz_wgrad_kernel, dim3((unsigned)((count * a.nslab + 255) / 256)), dim3(256), 0, st, a);
  XT_LAUNCH_CHECK();
  if (a.nslab > 1) {
    hipLaunchKernelGGL(mz_slab_sum_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st, slabs, count, a.nslab, dwb);
    XT_LAUNCH_CHECK();
  }
  return 0;
}

// ------------------------------------------------------------------ the loss head
struct MzLoss {
  const float* logits;
  int nblk, B, N, S;
  const float* target_dense;      // [B, S, N] or null
  const double* target_scalar;    // [B, S]
  double tmin, tmax;
  float scale0, scale_rest;
  float* probs;                   // may be null
  float* dz;                      // may be null
  double* rowloss;                // may be null (probabilities only)
};

template <bool WIDE>
__device__ __forceinline__ float mz_red_max(float v, float* sh) {
  for (int o = 32; o; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  if (WIDE) {
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    v = fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3]));
  }
  return v;
}
template <bool WIDE>
__device__ __forceinline__ double mz_red_sum(double v, double* sh) {
  for (int o = 32; o; o >>= 1) v = v + __shfl_xor(v, o);      // (a butterfly: every lane ends with the same bits)
  if (WIDE) {
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    v = ((sh[0] + sh[1]) + sh[2]) + sh[3];
  }
  return v;
}

// WIDE = false: 4 rows per workgroup, one wavefront each (N <= 64); true: one row per workgroup, lanes stride the row
template <bool WIDE>
__global__ __launch_bounds__(256) void mz_loss_kernel(const MzLoss a) {
  __shared__ float shf[4];
  __shared__ double shd[4];
  const int T = WIDE ? 256 : 64;
  const int t = WIDE ? threadIdx.x : (threadIdx.x & 63);
  const long long rows = (long long)a.nblk * a.B;
  const long long r = WIDE ? (long long)blockIdx.x : (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;          // (WIDE: never; else a whole wavefront leaves, and no barrier follows)
  const int k = (int)(r / a.B), b = (int)(r % a.B);
  const float* z = a.logits + r * a.N;
  float mx = -INFINITY;
  for (int j = t; j < a.N; j += T) mx = fmaxf(mx, z[j]);
  mx = mz_red_max<WIDE>(mx, shf);
  double se = 0.0;
  for (int j = t; j < a.N; j += T) se += (double)expf(z[j] - mx);
  const float sum = (float)mz_red_sum<WIDE>(se, shd);
  if (!a.rowloss) {
    for (int j = t; j < a.N; j += T) a.probs[r * a.N + j] = expf(z[j] - mx) / sum;
    return;
  }
  // the target row: dense, or the two-hot of the compressed scalar
  int i0 = -1;
  float t_lo = 0.f, t_hi = 0.f;
  const float* td = nullptr;
  if (a.target_dense) {
    td = a.target_dense + ((long long)b * a.S + k) * a.N;
  } else {
    double x = a.target_scalar[(long long)b * a.S + k];
    x = fmin(fmax(x, a.tmin), a.tmax) - a.tmin;
    const double sg = x > 0.0 ? 1.0 : (x < 0.0 ? -1.0 : 0.0);
    const double c = sg * (sqrt(fabs(x) + 1.0) - 1.0) + 0.001 * x;
    const double fl = floor(c);
    const double rest = c - fl;
    i0 = fl >= (double)(a.N - 1) ? a.N - 1 : (fl >= 0.0 ? (int)fl : 0);      // (NaN lands on bin 0)
    if (i0 >= a.N - 1) { t_lo = 1.f; t_hi = 0.f; }                           // the top of the range: the whole mass on the last bin
    else { t_lo = (float)(1.0 - rest); t_hi = (float)rest; }
  }
  double swp = 0.0, sl = 0.0;
  for (int j = t; j < a.N; j += T) {
    const float p = expf(z[j] - mx) / sum;
    const float tj = td ? td[j] : (j == i0 ? t_lo : (j == i0 + 1 ? t_hi : 0.f));
    const double pe = (double)p + 1e-10;
    swp += ((double)tj / pe) * (double)p;
    sl += (double)tj * log(pe);
  }
  swp = mz_red_sum<WIDE>(swp, shd);
  sl = mz_red_sum<WIDE>(sl, shd);
  const double bn = (double)a.B * (double)a.N;
  const double s = (double)(k == 0 ? a.scale0 : a.scale_rest) / bn;
  for (int j = t; j < a.N; j += T) {
    const float p = expf(z[j] - mx) / sum;
    const float tj = td ? td[j] : (j == i0 ? t_lo : (j == i0 + 1 ? t_hi : 0.f));
    const double pe = (double)p + 1e-10;
    if (a.probs) a.probs[r * a.N + j] = p;
    if (a.dz) a.dz[r * a.N + j] = (float)(s * (double)p * (swp - (double)tj / pe));
  }
  if (t == 0) a.rowloss[r] = -sl / bn;
}

// out[0] = the sum of n doubles: thread t takes t, t + 256, ... ascending, then a fixed tree
__global__ __launch_bounds__(256) void mz_loss_sum_kernel(const double* __restrict__ rowloss, long long n, double* __restrict__ out) {
  __shared__ double sh[256];
  double acc = 0.0;
  for (long long i = threadIdx.x; i < n; i += 256) acc += rowloss[i];
  sh[threadIdx.x] = acc;
  __syncthreads();
  for (int o = 128; o; o >>= 1) {
    if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = sh[0];
}

static int launch_mz_loss(const MzLoss& a, hipStream_t st) {
  XT_REQUIRE(a.logits && a.nblk > 0 && a.B > 0 && a.N >= 2 && a.N <= 65536, "xt_mz_loss: nblk %d, B %d, N %d out of range",
             a.nblk, a.B, a.N);
  XT_REQUIRE(a.rowloss ? (a.S >= a.nblk && (a.target_dense || a.target_scalar)) : a.probs != nullptr,
             "xt_mz_loss: needs a target with at least nblk = %d columns (S = %d), or a probability output", a.nblk, a.S);
  XT_REQUIRE(a.target_dense || !a.rowloss || a.tmax > a.tmin, "xt_mz_loss: tmax %g <= tmin %g", a.tmax, a.tmin);
  const long long rows = (long long)a.nblk * a.B;
  XT_REQUIRE(rows < (1ll << 31), "xt_mz_loss: too many rows");
  if (a.N <= 64) hipLaunchKernelGGL(mz_loss_kernel<false>, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, a);
  else hipLaunchKernelGGL(mz_loss_kernel<true>, dim3((unsigned)rows), dim3(256), 0, st, a);
  XT_LAUNCH_CHECK();
  return 0;
}

}  // namespace xt

// ------------------------------------------------------------------ the handle
struct xt_mz {
  xt_mz_desc d;
  xt_layer_desc rep[XT_MZ_MAX_CHAIN], dyn[XT_MZ_MAX_CHAIN], pred[XT_MZ_MAX_CHAIN];
  int max_batch;
  int nt, nq;                       // trunk layers of dyn / pred
  float *params, *grads, *m, *v, *state;
  float* ws;
  int64_t ws_floats;
  // workspace offsets (floats)
  int64_t o_rep_act[XT_MZ_MAX_CHAIN], o_rep_dpre[XT_MZ_MAX_CHAIN], o_rep_slabs;
  int rep_slab_cap[XT_MZ_MAX_CHAIN];
  int64_t o_h, o_dh, o_gpred;       // [(U + 1) Bm, H]: hidden stack, joined d(pre-activation), prediction gradient
  int64_t o_t[XT_MZ_MAX_CHAIN], o_dt[XT_MZ_MAX_CHAIN], o_tr;   // dyn trunk: activations, d(pre), the reward head's gradient [U Bm, Nt]
  int64_t o_q[XT_MZ_MAX_CHAIN], o_dq[XT_MZ_MAX_CHAIN], o_qv;   // pred trunk
  int64_t o_zr, o_dr, o_zp, o_dp, o_zv, o_dv;                  // logits and d(logits)
  int64_t o_wt_dyn[XT_MZ_MAX_CHAIN], o_wt_pred[XT_MZ_MAX_CHAIN];      // every Dense kernel transposed, once per step
  int64_t o_slabs, o_rowloss, o_scratch;
};

namespace xt {

static int mz_dense_ok(const xt_layer_desc& l, const char* who, int i) {
  const xt_conv_geom& g = l.g;
  XT_REQUIRE(g.H == 1 && g.W == 1 && g.KH == 1 && g.KW == 1 && g.S == 1 && g.OH == 1 && g.OW == 1 && g.PT == 0 && g.PL == 0 &&
             g.C >= 1 && g.N >= 1, "xt_mz_create: %s layer %d is not a Dense layer", who, i);
  XT_REQUIRE(g.act == XT_ACT_RELU || g.act == XT_ACT_NONE, "xt_mz_create: %s layer %d: activation %d (relu or none)", who, i, g.act);
  XT_REQUIRE(l.param_off >= 0, "xt_mz_create: %s layer %d: negative offset", who, i);
  return 0;
}

static inline int64_t al4(int64_t x) { return (x + 3) & ~(int64_t)3; }

static int rep_msplit(const xt_conv_geom& g, int B, int cap) {
  const long long M = (long long)B * g.OH * g.OW;
  long long s = M / 1024;
  if (s < 1) s = 1;
  if (s > cap) s = cap;
  return (int)s;
}

static int mz_plan(xt_mz* z) {
  const xt_mz_desc& d = z->d;
  const int64_t Bm = z->max_batch, U = d.unroll, S = U + 1, H = d.hidden;
  int64_t off = 0;
  auto take = [&](int64_t n) { const int64_t o = off; off += al4(n); return o; };
  z->o_h = take(S * Bm * H);
  z->o_dh = take(S * Bm * H);
  z->o_gpred = take(S * Bm * H);
  int64_t rep_slab = 4;
  for (int l = 0; l < d.n_rep; ++l) {
    const xt_conv_geom& g = z->rep[l].g;
    const int64_t out = Bm * g.OH * g.OW * g.N;
    const bool last = l == d.n_rep - 1;
    z->o_rep_act[l] = last ? z->o_h : take(out);
    z->o_rep_dpre[l] = last ? z->o_dh : take(out);
    const int64_t count = (int64_t)(g.KH * g.KW * g.C + 1) * g.N;
    int64_t cap = (16ll << 20) / count;
    if (cap > 64) cap = 64;
    if (cap < 1) cap = 1;
    z->rep_slab_cap[l] = (int)cap;
    const int64_t need = (int64_t)rep_msplit(g, (int)Bm, (int)cap) * count;
    if (need > rep_slab) rep_slab = need;
  }
  z->o_rep_slabs = take(rep_slab);
  int64_t slab = 4;
  auto dense = [&](const xt_layer_desc& l, int64_t rows) {
    const int64_t need = (int64_t)mz_nslab((int)rows) * (l.g.C + 1) * l.g.N;
    if (need > slab) slab = need;
  };
  for (int l = 0; l < z->nt; ++l) {
    z->o_t[l] = take(U * Bm * z->dyn[l].g.N);
    z->o_dt[l] = take(U * Bm * z->dyn[l].g.N);
    dense(z->dyn[l], U * Bm);
  }
  z->o_tr = take(U * Bm * z->dyn[z->nt - 1].g.N);
  dense(z->dyn[z->nt], U * Bm);
  dense(z->dyn[z->nt + 1], U * Bm);
  for (int l = 0; l < z->nq; ++l) {
    z->o_q[l] = take(S * Bm * z->pred[l].g.N);
    z->o_dq[l] = take(S * Bm * z->pred[l].g.N);
    dense(z->pred[l], S * Bm);
  }
  z->o_qv = take(S * Bm * z->pred[z->nq - 1].g.N);
  dense(z->pred[z->nq], S * Bm);
  dense(z->pred[z->nq + 1], S * Bm);
  z->o_zr = take(U * Bm * d.reward_support);
  z->o_dr = take(U * Bm * d.reward_support);
  z->o_zp = take(S * Bm * d.action_dim);
  z->o_dp = take(S * Bm * d.action_dim);
  z->o_zv = take(S * Bm * d.value_support);
  z->o_dv = take(S * Bm * d.value_support);
  for (int l = 0; l < d.n_dyn; ++l) z->o_wt_dyn[l] = take((int64_t)z->dyn[l].g.C * z->dyn[l].g.N);
  for (int l = 0; l < d.n_pred; ++l) z->o_wt_pred[l] = take((int64_t)z->pred[l].g.C * z->pred[l].g.N);
  z->o_slabs = take(slab);
  z->o_rowloss = take(2 * (2 * S + U) * Bm + 4);      // doubles
  z->o_scratch = take(4096);
  z->ws_floats = off;
  return 0;
}

static const float* wof(const xt_mz* z, const xt_layer_desc& l) { return z->params + l.param_off; }
static const float* bof(const xt_mz* z, const xt_layer_desc& l) { return z->params + l.param_off + (int64_t)l.g.C * l.g.N; }
static float* gof(const xt_mz* z, const xt_layer_desc& l) { return z->grads + l.param_off; }

// y = act(x . w + b) of one Dense layer over M rows; actions != null: the conditioned layer (w has A more rows)
static int mz_fwd(const xt_mz* z, const xt_layer_desc& l, const float* x, int M, float* y, const int32_t* actions, int a_stride,
                  int B, hipStream_t st) {
  MzGemm a{};
  const int A = actions ? z->d.action_dim : 0;
  a.x = x; a.K = l.g.C - A; a.ldx = a.K; a.w = wof(z, l); a.M = M; a.N = l.g.N; a.bias = bof(z, l);
  a.actions = actions; a.a_stride = a_stride; a.B = B > 0 ? B : 1; a.A = A; a.relu = l.g.act == XT_ACT_RELU; a.y = y;
  return launch_gemm<0>(a, st);
}

// the transposed kernels the step's input gradients read: [N, Kuse] per layer, Kuse = hidden for the conditioned layer
// (its action rows have no input gradient), else C.  Once per step: the weights do not change inside it.
static int mz_transpose_all(const xt_mz* z, hipStream_t st) {
  for (int l = 0; l < z->d.n_dyn; ++l)
    if (int rc = launch_transpose(wof(z, z->dyn[l]), l == 0 ? z->d.hidden : z->dyn[l].g.C, z->dyn[l].g.N, z->ws + z->o_wt_dyn[l], st))
      return rc;
  for (int l = 0; l < z->d.n_pred; ++l)
    if (int rc = launch_transpose(wof(z, z->pred[l]), z->pred[l].g.C, z->pred[l].g.N, z->ws + z->o_wt_pred[l], st)) return rc;
  return 0;
}

// dx [M, Kuse] = mask(maskx) * (add + c * dy . w[:Kuse]^T), wt = the layer's transposed kernel [N, Kuse]
static int mz_dgrad(const xt_mz* z, const xt_layer_desc& l, const float* wt, int Kuse, const float* dy, int M, const float* add,
                    float c, const float* maskx, float* dx, hipStream_t st) {
  MzGemm a{};
  a.x = dy; a.ldx = l.g.N; a.K = l.g.N; a.w = wt; a.M = M; a.N = Kuse; a.add = add; a.c = c; a.maskx = maskx; a.y = dx;
  return launch_gemm<1>(a, st);
}

static int mz_wgrad(const xt_mz* z, const xt_layer_desc& l, const float* x, const float* dy, int M, const int32_t* actions,
                    int a_stride, int B, hipStream_t st) {
  MzWgrad a{};
  const int A = actions ? z->d.action_dim : 0;
  a.x = x; a.K = l.g.C - A; a.ldx = a.K; a.dy = dy; a.actions = actions; a.a_stride = a_stride; a.B = B > 0 ? B : 1; a.A = A;
  a.M = M; a.N = l.g.N;
  return launch_mz_wgrad(a, gof(z, l), z->ws + z->o_slabs, st);
}

static int mz_check_bound(const xt_mz* z, int B, const char* who) {
  XT_REQUIRE(z && z->params && z->ws, "%s: the handle is not bound", who);
  XT_REQUIRE(B >= 1 && B <= z->max_batch, "%s: B = %d outside [1, %d]", who, B, z->max_batch);
  return 0;
}

// float32 observations [., obs_dim] (sample b = row idx[b], or row b) -> hstack rows [0, B)
static int mz_rep_fwd(const xt_mz* z, const void* obs, const int32_t* idx, int B, hipStream_t st) {
  const xt_input_xform xf = {0, 0.f, 1.f};
  const void* x = obs;
  for (int l = 0; l < z->d.n_rep; ++l) {
    const xt_layer_desc& L = z->rep[l];
    float* y = z->ws + z->o_rep_act[l];
    if (int rc = launch_fwd(&L.g, l == 0 ? &xf : nullptr, B, x, l == 0 ? idx : nullptr, wof(z, L), bof(z, L), y, nullptr, 1, st))
      return rc;
    x = y;
  }
  return 0;
}

// one dynamics step on B rows: h_in -> trunk (stored at row offset `row0` of the trunk buffers) -> h_out
static int mz_dyn_fwd(const xt_mz* z, const float* h_in, const int32_t* actions, int a_stride, int step, int B, int64_t row0,
                      float* h_out, hipStream_t st) {
  const float* x = h_in;
  for (int l = 0; l < z->nt; ++l) {
    float* y = z->ws + z->o_t[l] + row0 * z->dyn[l].g.N;
    // (the action of row b is actions[b * a_stride + step]: the pointer is moved, the block index inside stays 0)
    if (int rc = mz_fwd(z, z->dyn[l], x, B, y, l == 0 ? actions + step : nullptr, a_stride, B, st)) return rc;
    x = y;
  }
  return mz_fwd(z, z->dyn[z->nt], x, B, h_out, nullptr, 0, 0, st);
}

// the prediction chain on M stacked rows of the hidden stack: logits into o_zp / o_zv
static int mz_pred_fwd(const xt_mz* z, const float* h, int M, hipStream_t st) {
  const float* x = h;
  for (int l = 0; l < z->nq; ++l) {
    float* y = z->ws + z->o_q[l];
    if (int rc = mz_fwd(z, z->pred[l], x, M, y, nullptr, 0, 0, st)) return rc;
    x = y;
  }
  if (int rc = mz_fwd(z, z->pred[z->nq], x, M, z->ws + z->o_zv, nullptr, 0, 0, st)) return rc;
  return mz_fwd(z, z->pred[z->nq + 1], x, M, z->ws + z->o_zp, nullptr, 0, 0, st);
}

static int mz_softmax(const float* logits, int rows, int N, float* probs, hipStream_t st) {
  MzLoss a{};
  a.logits = logits; a.nblk = 1; a.B = rows; a.N = N; a.S = 1; a.probs = probs;
  return launch_mz_loss(a, st);
}

}  // namespace xt

extern "C" {

int xt_mz_create(const xt_mz_desc* desc, int32_t max_batch, xt_mz** out) {
  using namespace xt;
  XT_REQUIRE(desc && out, "xt_mz_create: null argument");
  *out = nullptr;
  const xt_mz_desc& d = *desc;
  XT_REQUIRE(max_batch >= 1 && max_batch <= (1 << 20), "xt_mz_create: max_batch = %d outside [1, 2^20]", max_batch);
  XT_REQUIRE(d.unroll >= 1 && d.unroll <= XT_MZ_MAX_UNROLL, "xt_mz_create: unroll (td_step) = %d outside [1, %d]", d.unroll,
             XT_MZ_MAX_UNROLL);
  XT_REQUIRE(d.value_support >= 2 && d.reward_support >= 2, "xt_mz_create: support sizes %d / %d (value / reward) below 2",
             d.value_support, d.reward_support);
  XT_REQUIRE(d.action_dim >= 1, "xt_mz_create: action_dim = %d below 1", d.action_dim);
  XT_REQUIRE(d.value_max > d.value_min && d.reward_max > d.reward_min, "xt_mz_create: max <= min (value [%g, %g], reward [%g, %g])",
             d.value_min, d.value_max, d.reward_min, d.reward_max);
  XT_REQUIRE(d.hidden >= 1, "xt_mz_create: hidden = %d below 1", d.hidden);
  XT_REQUIRE(d.rep && d.dyn && d.pred && d.n_rep >= 1 && d.n_rep <= XT_MZ_MAX_CHAIN && d.n_dyn >= 3 && d.n_dyn <= XT_MZ_MAX_CHAIN &&
             d.n_pred >= 3 && d.n_pred <= XT_MZ_MAX_CHAIN,
             "xt_mz_create: chain lengths %d / %d / %d (rep 1..%d, dyn and pred 3..%d)", d.n_rep, d.n_dyn, d.n_pred, XT_MZ_MAX_CHAIN,
             XT_MZ_MAX_CHAIN);
  XT_REQUIRE(d.n_params > 0 && d.n_params % 4 == 0, "xt_mz_create: n_params = %lld is not a positive multiple of 4",
             (long long)d.n_params);
  XT_REQUIRE(d.obs_dim >= 1, "xt_mz_create: obs_dim = %d below 1", d.obs_dim);
  // the rep chain: Dense layers whose widths meet
  int h = 1, w = 1, c = d.obs_dim;
  for (int l = 0; l < d.n_rep; ++l) {
    const xt_conv_geom& g = d.rep[l].g;
    XT_REQUIRE(g.H == 1 && g.W == 1 && g.KH == 1 && g.KW == 1 && g.S == 1 && g.OH == 1 && g.OW == 1 && g.PT == 0 && g.PL == 0,
               "xt_mz_create: rep layer %d is not a Dense layer: the representation chain takes Dense layers only (MuzeroMlp)", l);
    XT_REQUIRE((long long)g.H * g.W * g.C == (long long)h * w * c, "xt_mz_create: rep layer %d reads %dx%dx%d, its producer "
               "writes %dx%dx%d", l, g.H, g.W, g.C, h, w, c);
    XT_REQUIRE(g.C % 4 == 0 && g.N % 4 == 0 && d.rep[l].param_off % 4 == 0, "xt_mz_create: rep layer %d: C = %d, N = %d and its "
               "offset must be multiples of 4", l, g.C, g.N);
    XT_REQUIRE(g.act == XT_ACT_RELU, "xt_mz_create: rep layer %d: activation %d (relu only)", l, g.act);
    XT_REQUIRE(d.rep[l].param_off >= 0 && d.rep[l].param_off + (int64_t)(g.KH * g.KW * g.C + 1) * g.N <= d.n_params,
               "xt_mz_create: rep layer %d leaves the parameter buffer", l);
    h = g.OH; w = g.OW; c = g.N;
  }
  XT_REQUIRE(h == 1 && w == 1 && c == d.hidden, "xt_mz_create: the rep chain ends in %dx%dx%d, hidden = %d", h, w, c, d.hidden);
  const int nt = d.n_dyn - 2, nq = d.n_pred - 2;
  for (int l = 0; l < d.n_dyn; ++l) {
    if (int rc = mz_dense_ok(d.dyn[l], "dyn", l)) return rc;
    const int want_c = l == 0 ? d.hidden + d.action_dim : d.dyn[l < nt ? l - 1 : nt - 1].g.N;
    const int want_n = l == nt ? d.hidden : (l == nt + 1 ? d.reward_support : d.dyn[l].g.N);
    XT_REQUIRE(d.dyn[l].g.C == want_c && d.dyn[l].g.N == want_n, "xt_mz_create: dyn layer %d is %d -> %d, expected %d -> %d", l,
               d.dyn[l].g.C, d.dyn[l].g.N, want_c, want_n);
    XT_REQUIRE(d.dyn[l].g.act == (l <= nt ? XT_ACT_RELU : XT_ACT_NONE), "xt_mz_create: dyn layer %d: activation %d", l, d.dyn[l].g.act);
    XT_REQUIRE(d.dyn[l].param_off + (int64_t)(d.dyn[l].g.C + 1) * d.dyn[l].g.N <= d.n_params,
               "xt_mz_create: dyn layer %d leaves the parameter buffer", l);
  }
  for (int l = 0; l < d.n_pred; ++l) {
    if (int rc = mz_dense_ok(d.pred[l], "pred", l)) return rc;
    const int want_c = l == 0 ? d.hidden : d.pred[l < nq ? l - 1 : nq - 1].g.N;
    const int want_n = l == nq ? d.value_support : (l == nq + 1 ? d.action_dim : d.pred[l].g.N);
    XT_REQUIRE(d.pred[l].g.C == want_c && d.pred[l].g.N == want_n, "xt_mz_create: pred layer %d is %d -> %d, expected %d -> %d", l,
               d.pred[l].g.C, d.pred[l].g.N, want_c, want_n);
    XT_REQUIRE(d.pred[l].g.act == (l < nq ? XT_ACT_RELU : XT_ACT_NONE), "xt_mz_create: pred layer %d: activation %d", l,
               d.pred[l].g.act);
    XT_REQUIRE(d.pred[l].param_off + (int64_t)(d.pred[l].g.C + 1) * d.pred[l].g.N <= d.n_params,
               "xt_mz_create: pred layer %d leaves the parameter buffer", l);
  }
  // the widest stacked tensor stays inside the 32-bit element range of the kernels' row arithmetic
  long long widest = d.value_support;
  for (int l = 0; l < nt; ++l) widest = d.dyn[l].g.N > widest ? d.dyn[l].g.N : widest;
  for (int l = 0; l < nq; ++l) widest = d.pred[l].g.N > widest ? d.pred[l].g.N : widest;
  XT_REQUIRE((long long)(d.unroll + 1) * max_batch * widest < (1ll << 31), "xt_mz_create: (unroll + 1) * max_batch * %lld "
             "elements exceed 2^31", widest);
  xt_mz* z = new (std::nothrow) xt_mz();
  XT_REQUIRE(z, "xt_mz_create: out of memory");
  z->d = d;
  for (int l = 0; l < d.n_rep; ++l) z->rep[l] = d.rep[l];
  for (int l = 0; l < d.n_dyn; ++l) z->dyn[l] = d.dyn[l];
  for (int l = 0; l < d.n_pred; ++l) z->pred[l] = d.pred[l];
  z->d.rep = z->rep; z->d.dyn = z->dyn; z->d.pred = z->pred;
  z->max_batch = max_batch; z->nt = nt; z->nq = nq;
  if (int rc = mz_plan(z)) { delete z; return rc; }
  *out = z;
  return 0;
}

void xt_mz_destroy(xt_mz* mz) { delete mz; }

int64_t xt_mz_workspace_bytes(const xt_mz* mz) { return mz ? mz->ws_floats * 4 : 0; }

int xt_mz_bind(xt_mz* mz, float* params, float* grads, float* adam_m, float* adam_v, float* adam_state, void* workspace,
               int64_t workspace_bytes) {
  XT_REQUIRE(mz && params && grads && adam_m && adam_v && adam_state && workspace, "xt_mz_bind: null argument");
  XT_REQUIRE(workspace_bytes >= mz->ws_floats * 4, "xt_mz_bind: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
             (long long)mz->ws_floats * 4);
  XT_REQUIRE((((uintptr_t)params | (uintptr_t)grads | (uintptr_t)adam_m | (uintptr_t)adam_v | (uintptr_t)workspace) & 15) == 0,
             "xt_mz_bind: buffers must be 16-byte aligned");
  mz->params = params; mz->grads = grads; mz->m = adam_m; mz->v = adam_v; mz->state = adam_state;
  mz->ws = static_cast<float*>(workspace);
  return 0;
}

int xt_mz_step(xt_mz* mz, const void* obs, const int32_t* idx, int32_t B, const int32_t* actions, const double* target_value,
               const double* target_reward, const float* target_policy, const xt_mz_cfg* cfg, double* loss_out, void* stream) {
  using namespace xt;
  if (int rc = mz_check_bound(mz, B, "xt_mz_step")) return rc;
  XT_REQUIRE(obs && actions && target_value && target_reward && target_policy && cfg && loss_out, "xt_mz_step: null argument");
  const xt_mz* z = mz;
  const xt_mz_desc& d = z->d;
  const hipStream_t st = as_stream(stream);
  const int U = d.unroll, S = U + 1, H = d.hidden, nt = z->nt, nq = z->nq;
  const int MS = S * B, MU = U * B;
  float* ws = z->ws;
  float* hs = ws + z->o_h;
  float* dh = ws + z->o_dh;
  float* gp = ws + z->o_gpred;

  // ---- forward
  if (int rc = mz_rep_fwd(z, obs, idx, B, st)) return rc;
  for (int i = 0; i < U; ++i)
    if (int rc = mz_dyn_fwd(z, hs + (int64_t)i * B * H, actions, U, i, B, (int64_t)i * B, hs + (int64_t)(i + 1) * B * H, st)) return rc;
  const float* tl = ws + z->o_t[nt - 1];                      // the trunk's output of all steps, [U B, Nt]
  if (int rc = mz_fwd(z, z->dyn[nt + 1], tl, MU, ws + z->o_zr, nullptr, 0, 0, st)) return rc;
  if (int rc = mz_pred_fwd(z, hs, MS, st)) return rc;

  // ---- the three heads: d(logits) and the rows' losses
  double* rowloss = reinterpret_cast<double*>(ws + z->o_rowloss);
  const float inv_u = 1.f / (float)U;
  {
    MzLoss a{};
    a.logits = ws + z->o_zp; a.nblk = S; a.B = B; a.N = d.action_dim; a.S = S; a.target_dense = target_policy;
    a.scale0 = 1.f; a.scale_rest = inv_u; a.dz = ws + z->o_dp; a.rowloss = rowloss;
    if (int rc = launch_mz_loss(a, st)) return rc;
    a.logits = ws + z->o_zv; a.N = d.value_support; a.target_dense = nullptr; a.target_scalar = target_value;
    a.tmin = d.value_min; a.tmax = d.value_max; a.dz = ws + z->o_dv; a.rowloss = rowloss + MS;
    if (int rc = launch_mz_loss(a, st)) return rc;
    // (the reward target of dynamics step i is column i: block i of the U blocks reads column i)
    a.logits = ws + z->o_zr; a.nblk = U; a.N = d.reward_support; a.target_scalar = target_reward;
    a.tmin = d.reward_min; a.tmax = d.reward_max; a.scale0 = inv_u; a.dz = ws + z->o_dr; a.rowloss = rowloss + 2 * MS;
    if (int rc = launch_mz_loss(a, st)) return rc;
    hipLaunchKernelGGL(mz_loss_sum_kernel, dim3(1), dim3(256), 0, st, rowloss, (long long)(2 * MS + MU), loss_out);
    XT_LAUNCH_CHECK();
  }

  // ---- the prediction chain's backward, once over the stack
  if (int rc = mz_transpose_all(z, st)) return rc;
  const xt_layer_desc& Lv = z->pred[nq];
  const xt_layer_desc& Lp = z->pred[nq + 1];
  const float* ql = ws + z->o_q[nq - 1];
  if (int rc = mz_dgrad(z, Lv, ws + z->o_wt_pred[nq], Lv.g.C, ws + z->o_dv, MS, nullptr, 1.f, nullptr, ws + z->o_qv, st)) return rc;
  if (int rc = mz_dgrad(z, Lp, ws + z->o_wt_pred[nq + 1], Lp.g.C, ws + z->o_dp, MS, ws + z->o_qv, 1.f, ql, ws + z->o_dq[nq - 1], st)) return rc;
  if (int rc = mz_wgrad(z, Lv, ql, ws + z->o_dv, MS, nullptr, 0, 0, st)) return rc;
  if (int rc = mz_wgrad(z, Lp, ql, ws + z->o_dp, MS, nullptr, 0, 0, st)) return rc;
  for (int l = nq - 1; l >= 0; --l) {
    const float* xin = l == 0 ? hs : ws + z->o_q[l - 1];
    if (int rc = mz_wgrad(z, z->pred[l], xin, ws + z->o_dq[l], MS, nullptr, 0, 0, st)) return rc;
    if (l > 0) {
      if (int rc = mz_dgrad(z, z->pred[l], ws + z->o_wt_pred[l], z->pred[l].g.C, ws + z->o_dq[l], MS, nullptr, 1.f, xin, ws + z->o_dq[l - 1], st)) return rc;
    } else {
      if (int rc = mz_dgrad(z, z->pred[0], ws + z->o_wt_pred[0], H, ws + z->o_dq[0], MS, nullptr, 1.f, nullptr, gp, st)) return rc;
    }
  }

  // ---- the reward head, once over the U B dynamics rows
  const xt_layer_desc& Lr = z->dyn[nt + 1];
  const xt_layer_desc& Lh = z->dyn[nt];
  if (int rc = mz_dgrad(z, Lr, ws + z->o_wt_dyn[nt + 1], Lr.g.C, ws + z->o_dr, MU, nullptr, 1.f, nullptr, ws + z->o_tr, st)) return rc;
  if (int rc = mz_wgrad(z, Lr, tl, ws + z->o_dr, MU, nullptr, 0, 0, st)) return rc;

  // ---- the dynamics chain backwards: the only sequential part
  {   // step U has no consumer but the prediction net: d(pre) = relu'(h_U) * g_pred
    MzGemm a{};
    a.M = B; a.N = H; a.K = 0; a.add = gp + (int64_t)U * B * H; a.c = 0.f; a.maskx = hs + (int64_t)U * B * H;
    a.y = dh + (int64_t)U * B * H;
    if (int rc = launch_gemm<1>(a, st)) return rc;
  }
  for (int i = U - 1; i >= 0; --i) {
    const int64_t r0 = (int64_t)i * B;
    const int Nt = z->dyn[nt - 1].g.N;
    // t_i: the reward head's gradient + Dense_h's, through the trunk's relu
    if (int rc = mz_dgrad(z, Lh, ws + z->o_wt_dyn[nt], Lh.g.C, dh + (r0 + B) * H, B, ws + z->o_tr + r0 * Nt, 1.f, ws + z->o_t[nt - 1] + r0 * Nt,
                          ws + z->o_dt[nt - 1] + r0 * Nt, st))
      return rc;
    for (int l = nt - 1; l >= 1; --l) {
      const int Np = z->dyn[l - 1].g.N, Nl = z->dyn[l].g.N;
      if (int rc = mz_dgrad(z, z->dyn[l], ws + z->o_wt_dyn[l], z->dyn[l].g.C, ws + z->o_dt[l] + r0 * Nl, B, nullptr, 1.f, ws + z->o_t[l - 1] + r0 * Np,
                            ws + z->o_dt[l - 1] + r0 * Np, st))
        return rc;
    }
    // the hidden-state join: g(h_i) = g_pred(h_i) + c * dh, c = 0.5 behind scale_gradient (i >= 1), 1 for h_0
    if (int rc = mz_dgrad(z, z->dyn[0], ws + z->o_wt_dyn[0], H, ws + z->o_dt[0] + r0 * z->dyn[0].g.N, B, gp + r0 * H, i >= 1 ? 0.5f : 1.f, hs + r0 * H,
                          dh + r0 * H, st))
      return rc;
  }

  // ---- the dynamics layers' weight gradients, once over the stacked rows the backward chain has filled
  if (int rc = mz_wgrad(z, Lh, tl, dh + (int64_t)B * H, MU, nullptr, 0, 0, st)) return rc;
  for (int l = nt - 1; l >= 1; --l)
    if (int rc = mz_wgrad(z, z->dyn[l], ws + z->o_t[l - 1], ws + z->o_dt[l], MU, nullptr, 0, 0, st)) return rc;
  if (int rc = mz_wgrad(z, z->dyn[0], hs, ws + z->o_dt[0], MU, actions, U, B, st)) return rc;

  // ---- the representation chain's backward from d(pre) of its last layer = rows [0, B) of the joined gradient
  for (int l = d.n_rep - 1; l >= 0; --l) {
    const xt_layer_desc& L = z->rep[l];
    const int cap = z->rep_slab_cap[l], ms = rep_msplit(L.g, B, cap);
    float* slabs = ws + z->o_rep_slabs;
    if (l > 0) {
      if (int rc = xt_layer_bwd(&L.g, B, ws + z->o_rep_act[l - 1], nullptr, ws + z->o_rep_dpre[l], wof(z, L), XT_ACT_RELU, nullptr,
                                ws + z->o_rep_dpre[l - 1], gof(z, L), slabs, ms, ms, stream, nullptr))
        return rc;
    } else {
      const xt_input_xform xf0 = {0, 0.f, 1.f};
      if (int rc = xt_layer_wgrad_slabs(&L.g, &xf0, B, obs, idx, ws + z->o_rep_dpre[0], gof(z, L), slabs, ms, ms, stream, nullptr))
        return rc;
    }
  }
  return 0;
}

int xt_mz_apply(xt_mz* mz, const xt_mz_cfg* cfg, void* stream) {
  XT_REQUIRE(mz && mz->params && cfg, "xt_mz_apply: the handle is not bound");
  // 2^100 * min(1 / norm, 2^-100) == 1.0f exactly for every norm below 2^100: tf.train.AdamOptimizer without clipping
  const float no_clip = 1.2676506002282294e30f;
  return xt_adam_tf_clip(mz->params, mz->grads, mz->m, mz->v, mz->d.n_params, cfg->lr, cfg->beta1, cfg->beta2, cfg->eps, no_clip,
                         1.f, mz->state, mz->ws + mz->o_scratch, stream);
}

int xt_mz_initial(xt_mz* mz, const void* obs, const int32_t* idx, int32_t B, float* policy, float* value, float* hidden,
                  void* stream) {
  using namespace xt;
  if (int rc = mz_check_bound(mz, B, "xt_mz_initial")) return rc;
  XT_REQUIRE(obs && policy && value && hidden, "xt_mz_initial: null argument");
  const hipStream_t st = as_stream(stream);
  float* hs = mz->ws + mz->o_h;
  if (int rc = mz_rep_fwd(mz, obs, idx, B, st)) return rc;
  if (int rc = mz_pred_fwd(mz, hs, B, st)) return rc;
  if (int rc = mz_softmax(mz->ws + mz->o_zp, B, mz->d.action_dim, policy, st)) return rc;
  if (int rc = mz_softmax(mz->ws + mz->o_zv, B, mz->d.value_support, value, st)) return rc;
  XT_CHECK_HIP(hipMemcpyAsync(hidden, hs, (size_t)B * mz->d.hidden * 4, hipMemcpyDeviceToDevice, st));
  return 0;
}

int xt_mz_recurrent(xt_mz* mz, const float* hidden_in, const int32_t* action, int32_t B, float* hidden_out, float* reward,
                    float* policy, float* value, void* stream) {
  using namespace xt;
  if (int rc = mz_check_bound(mz, B, "xt_mz_recurrent")) return rc;
  XT_REQUIRE(hidden_in && action && hidden_out && reward && policy && value, "xt_mz_recurrent: null argument");
  const hipStream_t st = as_stream(stream);
  float* hs = mz->ws + mz->o_h;
  if (int rc = mz_dyn_fwd(mz, hidden_in, action, 1, 0, B, 0, hs, st)) return rc;
  if (int rc = mz_fwd(mz, mz->dyn[mz->nt + 1], mz->ws + mz->o_t[mz->nt - 1], B, mz->ws + mz->o_zr, nullptr, 0, 0, st)) return rc;
  if (int rc = mz_pred_fwd(mz, hs, B, st)) return rc;
  if (int rc = mz_softmax(mz->ws + mz->o_zr, B, mz->d.reward_support, reward, st)) return rc;
  if (int rc = mz_softmax(mz->ws + mz->o_zp, B, mz->d.action_dim, policy, st)) return rc;
  if (int rc = mz_softmax(mz->ws + mz->o_zv, B, mz->d.value_support, value, st)) return rc;
  XT_CHECK_HIP(hipMemcpyAsync(hidden_out, hs, (size_t)B * mz->d.hidden * 4, hipMemcpyDeviceToDevice, st));
  return 0;
}

int xt_mz_loss(const float* logits, int32_t nblk, int32_t B, int32_t N, int32_t S, const float* target_dense,
               const double* target_scalar, double tmin, double tmax, float scale0, float scale_rest, float* probs, float* dz,
               double* rowloss, double* loss_out, void* stream) {
  using namespace xt;
  XT_REQUIRE(rowloss, "xt_mz_loss: rowloss is null");
  MzLoss a{};
  a.logits = logits; a.nblk = nblk; a.B = B; a.N = N; a.S = S; a.target_dense = target_dense; a.target_scalar = target_scalar;
  a.tmin = tmin; a.tmax = tmax; a.scale0 = scale0; a.scale_rest = scale_rest; a.probs = probs; a.dz = dz; a.rowloss = rowloss;
  const hipStream_t st = as_stream(stream);
  if (int rc = launch_mz_loss(a, st)) return rc;
  if (loss_out) {
    hipLaunchKernelGGL(mz_loss_sum_kernel, dim3(1), dim3(256), 0, st, rowloss, (long long)nblk * B, loss_out);
    XT_LAUNCH_CHECK();
  }
  return 0;
}

int xt_mz_cond_fwd(const float* h, const int32_t* actions, int32_t a_stride, int32_t nblk, int32_t B, int32_t hidden, int32_t A,
                   int32_t N, const float* w, const float* bias, int32_t act, float* y, void* stream) {
  using namespace xt;
  XT_REQUIRE(h && actions && w && bias && y && nblk >= 1 && B >= 1 && hidden >= 1 && A >= 1 && N >= 1 && a_stride >= nblk &&
             (long long)nblk * B * (N > hidden ? N : hidden) < (1ll << 31), "xt_mz_cond_fwd: bad arguments");
  XT_REQUIRE(act == XT_ACT_RELU || act == XT_ACT_NONE, "xt_mz_cond_fwd: activation %d (relu or none)", act);
  MzGemm a{};
  a.x = h; a.ldx = hidden; a.K = hidden; a.w = w; a.M = nblk * B; a.N = N; a.bias = bias; a.actions = actions; a.a_stride = a_stride;
  a.B = B; a.A = A; a.relu = act == XT_ACT_RELU; a.y = y;
  return launch_gemm<0>(a, as_stream(stream));
}

int xt_mz_cond_bwd(const float* h, const int32_t* actions, int32_t a_stride, int32_t nblk, int32_t B, int32_t hidden, int32_t A,
                   int32_t N, const float* w, const float* dy, const float* g_pred, float c, float* g, float* dwb, float* slabs,
                   float* wt, void* stream) {
  using namespace xt;
  XT_REQUIRE(h && actions && w && dy && g && dwb && wt && nblk >= 1 && B >= 1 && hidden >= 1 && A >= 1 && N >= 1 &&
             a_stride >= nblk && (long long)nblk * B * (N > hidden ? N : hidden) < (1ll << 31), "xt_mz_cond_bwd: bad arguments");
  const hipStream_t st = as_stream(stream);
  const int M = nblk * B;
  MzWgrad wg{};
  wg.x = h; wg.ldx = hidden; wg.K = hidden; wg.dy = dy; wg.actions = actions; wg.a_stride = a_stride; wg.B = B; wg.A = A; wg.M = M;
  wg.N = N;
  if (int rc = launch_mz_wgrad(wg, dwb, slabs, st)) return rc;
  if (int rc = launch_transpose(w, hidden, N, wt, st)) return rc;
  MzGemm a{};
  a.x = dy; a.ldx = N; a.K = N; a.w = wt; a.M = M; a.N = hidden; a.add = g_pred; a.c = c; a.maskx = h; a.y = g;
  return launch_gemm<1>(a, st);
}

}  // extern "C"
