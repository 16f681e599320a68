// The plain Dense kernels over stacked rows that the MuZero, QMIX and SCC learners share (xt_muzero.hip, xt_qmix.hip,
// xt_scc.hip): y = epilogue(x . w), the slab-ordered weight gradient with its slab sum, a fill and the ordered float64 sum.
// All of them float32 without contraction (the build's -ffp-contract=off), no atomics, every sum in ascending order: the
// NumPy twins of the tests reproduce them bit for bit, and a train is bit-identical from run to run.
// Every translation unit that includes this file gets its own copy (internal linkage), compiled with that object's flags:
// xt_qmix.o and xt_scc.o keep the packed-fp32 VALU forms off, xt_muzero.o keeps the default (see the Makefile).
#pragma once
#include "xt_common.h"

namespace xt {
namespace {

// time-major row r = t * S + b * n + a  ->  row (b * T + t) * n + a of a [B, T, n, .] array
__device__ __forceinline__ long long dense_bt_row(long long r, int S, int n, int T) {
  const int t = (int)(r / S), s = (int)(r % S);
  return ((long long)(s / n) * T + t) * n + s % n;
}

// ------------------------------------------------------------------ y[m, n] = epilogue(sum_k x[m, k] w[k, n])
// One thread owns 4 consecutive rows of one column (the w element is loaded once for the four); consecutive threads own
// consecutive columns, so w loads coalesce and x loads are a few broadcast addresses per wavefront.
// The epilogue, in this order: v = c * acc; + the conditioning row; + bias; add + v; relu; mask.  Every layer is either a
// forward (conditioning row, bias, relu) or an input gradient (c, add, mask): the kernel is instantiated for the two halves.
struct DenseGemm {
  const float* x; int ldx;               // [M, ldx], K columns read; K == 0: x and w may be null (y = mask * add)
  const float* w; int ldw; int wt;       // element (k, n) of the kernel at w[k * ldw + n], or (wt) at w[n * ldw + k]
  int M, K, N;
  float c = 1.f;                         // scale of the product (the join of an input gradient)
  const int32_t* actions;                // null, or the conditioning: row r = i * B + b adds w[K + actions[b * a_stride + i]]
  int a_stride, B, A;                    // (wt == 0; w has A more rows)
  const float* bias; int relu;
  const float* add;                      // [M, ldy] or null: y = add + v (may be y itself)
  const float* maskx; int ldm;           // null, or y = 0 where maskx[m, n] <= 0
  float* y; int ldy;
  int imap, omap, S, n, T;               // imap / omap: x / y rows are [B, T, n, .] rows, m is time-major
};

// MAPPED: the row maps and the transposed kernel are looked at (the recurrent agent's layers and every input gradient of QMIX /
// SCC); else imap = omap = wt = 0.  GRAD: the input gradient's half of the epilogue; else the forward's
template <bool MAPPED, bool GRAD>
__global__ __launch_bounds__(256) void dense_gemm_kernel(const DenseGemm a) {
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
    xr[r] = a.x + (MAPPED && a.imap ? dense_bt_row(m, a.S, a.n, a.T) : m) * a.ldx;
  }
  const long long wk = MAPPED && a.wt ? 1 : a.ldw, wn = MAPPED && a.wt ? a.ldw : 1;
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
    const long long yr = MAPPED && a.omap ? dense_bt_row(m, a.S, a.n, a.T) : m;
    if (!GRAD) {
      if (a.actions) {
        const int act = a.actions[(long long)(m % a.B) * a.a_stride + m / a.B];
        if (act >= 0 && act < a.A) v = v + a.w[(long long)(a.K + act) * a.ldw + n];
      }
      if (a.bias) v = v + a.bias[n];
      if (a.relu) v = v > 0.f ? v : 0.f;
    } else {
      v = a.c * v;
      if (a.add) v = a.add[yr * a.ldy + n] + v;
      if (a.maskx && !(a.maskx[(long long)m * a.ldm + n] > 0.f)) v = 0.f;
    }
    a.y[yr * a.ldy + n] = v;
  }
}

static int launch_dense_gemm(const DenseGemm& a, hipStream_t st) {
  XT_REQUIRE(a.M > 0 && a.N > 0 && a.K >= 0 && a.y && (a.K == 0 || (a.x && a.w)) && (!a.actions || (a.B > 0 && !a.wt)),
             "dense gemm: bad arguments");
  const long long total = (long long)((a.M + 3) >> 2) * a.N;
  XT_REQUIRE((total + 255) / 256 < (1ll << 31), "dense gemm: too many outputs");
  const bool mapped = a.imap || a.omap || a.wt, grad = a.add || a.maskx || a.c != 1.f;
  XT_REQUIRE(!grad || !(a.actions || a.bias || a.relu), "dense gemm: a forward's and an input gradient's epilogue in one launch");
  const dim3 grid((unsigned)((total + 255) / 256));
  auto kernel = mapped ? (grad ? dense_gemm_kernel<true, true> : dense_gemm_kernel<true, false>)
                       : (grad ? dense_gemm_kernel<false, true> : dense_gemm_kernel<false, false>);
  hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, a);
  XT_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------ dW = x^T . dy (+ db) over row slabs, then the slabs
// out[s][kk, n] over the rows [s * rows, (s + 1) * rows) ascending: kk < K: sum_r x[r, kk] dy[r, n]; K <= kk < K + A: the sum
// over the rows whose action is kk - K of dy[r, n] (zero when nobody took it); kk == K + A (bias): sum_r dy[r, n].
struct DenseWgrad {
  const float* x; int ldx;
  const float* xmul; int ldxm;           // null, or the x element is x * xmul (r o h of the candidate kernel)
  const float* dy; int ldy;
  const int32_t* actions;                // null (A == 0), or the gathered rows of the conditioned layer: row r = i * B + b took
  int a_stride, B, A;                    // actions[b * a_stride + i]
  int M, K, N, rows, nslab, bias;        // rows: the slab height (the bits depend on it)
  int imap, S, n, T;
  float* out;                            // [nslab, (K + A + bias) * N]
};

// MAPPED: the x element goes through imap / xmul (the recurrent agent's layers); else it is x[r, kk] itself
template <bool MAPPED>
__global__ __launch_bounds__(256) void dense_wgrad_kernel(const DenseWgrad a) {
  const long long count = (long long)(a.K + a.A + a.bias) * a.N;
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  if (gid >= count * a.nslab) return;
  const int s = (int)(gid / count);
  const int e = (int)(gid % count);
  const int kk = e / a.N, n = e % a.N;
  const int r0 = s * a.rows;
  const int r1 = r0 + a.rows < a.M ? r0 + a.rows : a.M;
  float acc = 0.f;
  if (kk < a.K) {
    auto xel = [&](int r) {
      const long long xr = MAPPED && a.imap ? dense_bt_row(r, a.S, a.n, a.T) : r;
      const float xv = a.x[xr * a.ldx + kk];
      return MAPPED && a.xmul ? xv * a.xmul[(long long)r * a.ldxm + kk] : xv;
    };
    int r = r0;
    for (; r + 4 <= r1; r += 4) {        // four rows' loads in flight, added in ascending order
      float xv[4], dv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        xv[u] = xel(r + u);
        dv[u] = a.dy[(long long)(r + u) * a.ldy + n];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) acc = acc + xv[u] * dv[u];
    }
    for (; r < r1; ++r) acc = acc + xel(r) * a.dy[(long long)r * a.ldy + n];
  } else if (kk < a.K + a.A) {
    const int want = kk - a.K;
    for (int r = r0; r < r1; ++r)
      if (a.actions[(long long)(r % a.B) * a.a_stride + r / a.B] == want) acc = acc + a.dy[(long long)r * a.ldy + n];
  } else {
    for (int r = r0; r < r1; ++r) acc = acc + a.dy[(long long)r * a.ldy + n];
  }
  a.out[gid] = acc;
}

// dw[e] (e < nw) / db[e - nw] = sum over ascending s of slabs[s][e]
__global__ __launch_bounds__(256) void dense_slab_sum_kernel(const float* __restrict__ slabs, long long count, long long nw, int nslab,
                                                          float* __restrict__ dw, float* __restrict__ db) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= count) return;
  float acc = 0.f;
  for (int s = 0; s < nslab; ++s) acc = acc + slabs[(long long)s * count + e];
  if (e < nw) dw[e] = acc;
  else db[e - nw] = acc;
}

__global__ __launch_bounds__(256) void dense_fill_kernel(float* __restrict__ p, long long n, float v) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e < n) p[e] = v;
}

static inline int dense_nslab(long long M, int rows) { return (int)((M + rows - 1) / rows); }

static int launch_slab_sum(const float* slabs, long long count, long long nw, int nslab, float* dw, float* db, hipStream_t st) {
  hipLaunchKernelGGL(dense_slab_sum_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st, slabs, count, nw, nslab, dw, db);
  XT_LAUNCH_CHECK();
  return 0;
}

// dw [K + A, N] and (db != null) db [N], over slabs of `rows` rows; `slabs` holds dense_nslab(M, rows) * (K + A + 1) * N floats.
// `direct`: one slab is written straight to dw (db == dw + (K + A) * N), without the slab sum -- not the same bits as the sum:
// 0.f + (-0.f) is +0.f.  M == 0: dw (and db) = 0.
static int launch_dense_wgrad(DenseWgrad a, float* dw, float* db, float* slabs, int rows, bool direct, hipStream_t st) {
  XT_REQUIRE(dw && a.K > 0 && a.N > 0 && a.M >= 0 && rows > 0 && a.A >= 0 && (a.A == 0 || (a.actions && a.B > 0)),
             "dense wgrad: bad arguments");
  a.bias = db ? 1 : 0;
  const long long nw = (long long)(a.K + a.A) * a.N, count = nw + (long long)a.bias * a.N;
  if (a.M == 0) {
    hipLaunchKernelGGL(dense_fill_kernel, dim3((unsigned)((nw + 255) / 256)), dim3(256), 0, st, dw, nw, 0.f);
    if (db) hipLaunchKernelGGL(dense_fill_kernel, dim3((unsigned)((a.N + 255) / 256)), dim3(256), 0, st, db, (long long)a.N, 0.f);
    XT_LAUNCH_CHECK();
    return 0;
  }
  XT_REQUIRE(a.x && a.dy, "dense wgrad: bad arguments");
  a.rows = rows;
  a.nslab = dense_nslab(a.M, rows);
  direct = direct && a.nslab == 1;
  XT_REQUIRE(direct ? (!db || db == dw + nw) : slabs != nullptr, "dense wgrad: %d rows need a slab buffer", a.M);
  XT_REQUIRE((count * a.nslab + 255) / 256 < (1ll << 31), "dense wgrad: too large");
  a.out = direct ? dw : slabs;
  const dim3 grid((unsigned)((count * a.nslab + 255) / 256));
  if (a.imap || a.xmul) hipLaunchKernelGGL(dense_wgrad_kernel<true>, grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL(dense_wgrad_kernel<false>, grid, dim3(256), 0, st, a);
  XT_LAUNCH_CHECK();
  return direct ? 0 : launch_slab_sum(slabs, count, nw, a.nslab, dw, db, st);
}

// ------------------------------------------------------------------ ordered float64 sums
// the workgroup's 256 partial sums in a fixed tree; every thread calls it, thread 0's return value is the sum
__device__ __forceinline__ double dense_tree_sum(double acc) {
  __shared__ double sh[256];
  sh[threadIdx.x] = acc;
  __syncthreads();
  for (int o = 128; o; o >>= 1) {
    if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
    __syncthreads();
  }
  return sh[0];
}

// out[0] = (sum of n values, thread t takes t, t + 256, ... ascending, then the fixed tree) / (div ? div[0] : 1)
template <typename T>
__global__ __launch_bounds__(256) void dense_sum_kernel(const T* __restrict__ src, long long n, const double* __restrict__ div,
                                                        double* __restrict__ out) {
  double acc = 0.0;
  for (long long i = threadIdx.x; i < n; i += 256) acc += (double)src[i];
  const double sum = dense_tree_sum(acc);
  if (threadIdx.x == 0) out[0] = div ? sum / div[0] : sum;
}

template <typename T>
static int launch_dense_sum(const T* src, long long n, const double* div, double* out, hipStream_t st) {
  hipLaunchKernelGGL(dense_sum_kernel<T>, dim3(1), dim3(256), 0, st, src, n, div, out);
  XT_LAUNCH_CHECK();
  return 0;
}

}  // namespace
}  // namespace xt
