// SCC: the multi-channel critic, the counterfactual credits and the two optimisers (xt_scc_* of include/xt_mi355x.h, DESIGN
// section 10).  The GRU agent is QMIX's: agent_fwd / agent_bwd and the recurrent kernels come from xt_qmix_dev.h, the plain Dense
// kernels (dense_gemm_kernel, dense_wgrad_kernel, the slab sum, the ordered sum) from xt_dense_dev.h.
//
//   scc_critic_fwd_kernel   one pass over the (row, agent) items, agent-major: a workgroup stages its group's L2 in LDS once and
//                           walks 16-item tiles; one first-layer product (fp32 MFMA 16x16x4, the one-hot column added as a weight
//                           row in the epilogue) feeds the full and the counterfactual epilogue, the second layer runs from LDS,
//                           the dot with the final kernel's slice is a fixed-order reduction.  The critic is additive over the
//                           agents, so credit i = s_full(i) - s_alt(i): no masked copies, no further passes, no random draws.
//   scc_td_kernel           v, y, the masked TD error, the row's loss, dv and the credits
//   scc_critic_bwd_kernel   dh2 and dh1 = (dh2 . L2^T) o [h1 > 0] on the same tiling, L2^T in LDS
//   scc_wgrad1_kernel / scc_vgrad_kernel   slab-ordered weight gradients; the first layer's loader makes the one-hot columns
//   scc_actor_head_kernel   the gather of the chosen q, the actor loss and dq as whole rows
//   scc_adam_kernel / scc_rmsprop_kernel   TF1 Adam (critic) and plain RMSProp (agent) on g clip / max(||g||, clip)
// The 16-row MFMA, as in the GRU kernels: the example's batch has 2 agents x 32 x 300 rows = 1200 tiles of 16, enough to fill the
// machine, and a 16-row tile keeps the per-tile LDS (x chunk, two h1 variants) at 5 KB next to the 72 KB of L2 at U = 128.
// Float32 without contraction, no atomics, every sum in a fixed order.
#include <cmath>
#include <new>

#include "xt_common.h"
#include "xt_qmix_dev.h"

namespace xt {

constexpr int kSccKC = 64;               // first-layer K chunk staged in LDS
constexpr int kSccMaxAgents = 32;
constexpr int kSccAgentTensors = 8;
__device__ __forceinline__ int scc_dal4(int x) { return (x + 3) & ~3; }

// where agent i's critic weights are in a parameter set, and how an item finds its source row
struct SccNet {
  int l1[kSccMaxAgents];                 // offset of L1 of agent i's group; b1, L2, b2 follow, each on a 16-byte boundary
  int wv;                                // offset of the final kernel ([n U, 1] or [U, 1]); its bias follows
  int merge_add, KA, n;                  // KA = o + A rows of L1
};
struct SccSrc {
  const float* x; int ldx;               // [B, Tsrc, n, ldx]; columns [0, K) are multiplied by L1[:K]
  const int32_t* actions;                // [B, T, n] or null (no row of L1 is added)
  int K, A, B, T, Tsrc, shift;           // shift: row t reads t' = min(t + 1, T - 1) (the reference's aliased placeholders)
};

__device__ __forceinline__ int scc_src_t(const SccSrc& s, int t) { return s.shift ? (t + 1 < s.T ? t + 1 : s.T - 1) : t; }

// ------------------------------------------------------------------ the critic's forward
struct SccCriticFwd {
  const float* p[2];                     // eval, target (grid z)
  SccNet net; SccSrc src;
  int alt_zero;                          // the alternative is h(0) (n <= 2: the whole slice zeroed), else the action part zeroed
  float* sc;                             // [3, n R]: s_eval_full | s_eval_alt | s_target_full
  float *h1, *h2;                        // [n R, U] of the eval set's full variant, or null
};

template <int U>
__global__ __launch_bounds__(U * 4) void scc_critic_fwd_kernel(const SccCriticFwd a) {
  constexpr int NW = U / 16, LDB = U + 16, LDH = U + 1, LDX = kSccKC + 1, NT = U * 4;
  extern __shared__ float lds[];
  float* l2s = lds;                      // [U][LDB]
  float* xs = l2s + U * LDB;             // [16][LDX]
  float* h1s = xs + 16 * LDX;            // [2][16][LDH]
  float* red = h1s + 2 * 16 * LDH;       // [2][NW][16]
  int* srow = reinterpret_cast<int*>(red + 2 * NW * 16);      // [16] element offset of the item's source row
  int* acts = srow + 16;                 // [16] action, -1: none
  const int set = blockIdx.z, i = blockIdx.y, tid = threadIdx.x;
  const int w = tid >> 6, l = tid & 63, j = l & 15, g = l >> 4, col = 16 * w + j;
  const SccSrc& s = a.src;
  const int R = s.B * s.T, K = s.K, nvar = set == 0 ? 2 : 1;
  const float* __restrict__ p = a.p[set];
  const float* __restrict__ L1 = p + a.net.l1[i];
  const float* __restrict__ b1 = L1 + scc_dal4(a.net.KA * U);
  const float* __restrict__ L2 = b1 + scc_dal4(U);
  const float* __restrict__ b2 = L2 + U * U;
  const float* __restrict__ wv = p + a.net.wv + (a.net.merge_add ? 0 : i * U);
  for (int e = tid; e < U * U; e += NT) l2s[(e / U) * LDB + e % U] = L2[e];
  const float bias1 = b1[col], bias2 = b2[col], wcol = wv[col];
  const int ntile = (R + 15) >> 4;
  for (int tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
    const int r0 = tile * 16;
    __syncthreads();                     // the last tile's readers are done (first pass: L2 is staged)
    if (tid < 16) {
      const int r = r0 + tid < R ? r0 + tid : R - 1;
      const int b = r / s.T, t = scc_src_t(s, r % s.T);
      srow[tid] = ((b * s.Tsrc + t) * a.net.n + i) * s.ldx;
      const int act = s.actions ? s.actions[(b * s.T + t) * a.net.n + i] : -1;
      acts[tid] = act >= 0 && act < s.A ? act : -1;
    }
    __syncthreads();
    qm_f4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < K; k0 += kSccKC) {
      for (int e = tid; e < 16 * kSccKC; e += NT) {
        const int rr = e / kSccKC, kk = e % kSccKC;
        xs[rr * LDX + kk] = k0 + kk < K ? s.x[srow[rr] + k0 + kk] : 0.f;
      }
      __syncthreads();
      const int left = K - k0 < kSccKC ? K - k0 : kSccKC;
      for (int kk = 0; kk < (left + 3) >> 2; ++kk) {
        const int k = k0 + 4 * kk + g;
        const float bv = k < K ? L1[k * U + col] : 0.f;
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(xs[j * LDX + 4 * kk + g], bv, acc, 0, 0, 0);
      }
      __syncthreads();
    }
    // two epilogues of the one product: + b1 + L1[o + a] (full) and + b1 alone (the action part zeroed) or b1 (h(0))
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int row = 4 * g + v, act = acts[row];
      float full = acc[v] + bias1;
      if (act >= 0) full = full + L1[(K + act) * U + col];
      const float alt = a.alt_zero ? bias1 : acc[v] + bias1;
      full = full > 0.f ? full : 0.f;
      h1s[row * LDH + col] = full;
      if (nvar == 2) h1s[(16 + row) * LDH + col] = alt > 0.f ? alt : 0.f;
      if (set == 0 && a.h1 && r0 + row < R) a.h1[((long long)i * R + r0 + row) * U + col] = full;
    }
    __syncthreads();
    for (int var = 0; var < nvar; ++var) {
      const float* hs = h1s + var * 16 * LDH;
      qm_f4 c2 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
      for (int kk = 0; kk < U / 4; ++kk)
        c2 = __builtin_amdgcn_mfma_f32_16x16x4f32(hs[j * LDH + 4 * kk + g], l2s[(4 * kk + g) * LDB + col], c2, 0, 0, 0);
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int row = 4 * g + v;
        float h2 = c2[v] + bias2;
        h2 = h2 > 0.f ? h2 : 0.f;
        if (var == 0 && set == 0 && a.h2 && r0 + row < R) a.h2[((long long)i * R + r0 + row) * U + col] = h2;
        float pv = h2 * wcol;
        for (int o = 8; o; o >>= 1) pv = pv + __shfl_xor(pv, o);      // the 16 columns of this wavefront (a butterfly: one order)
        if (j == 0) red[(var * NW + w) * 16 + row] = pv;
      }
    }
    __syncthreads();
    if (tid < 16 * nvar) {
      const int var = tid >> 4, row = tid & 15;
      float sum = 0.f;
      for (int ww = 0; ww < NW; ++ww) sum = sum + red[(var * NW + ww) * 16 + row];
      if (r0 + row < R) a.sc[(long long)(set == 0 ? var : 2) * a.net.n * R + (long long)i * R + r0 + row] = sum;
    }
  }
}

template <int U>
static constexpr int scc_fwd_lds() { return (U * (U + 16) + 16 * (kSccKC + 1) + 2 * 16 * (U + 1) + 2 * (U / 16) * 16 + 32) * 4; }
template <int U>
static constexpr int scc_bwd_lds() { return (U * (U + 16) + 16 * (U + 1)) * 4; }

template <int U>
static int launch_scc_fwd_u(const SccCriticFwd& a, int nset, int blocks, hipStream_t st) {
  static PerDeviceOnce attr_once;
  attr_once.run([] {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(scc_critic_fwd_kernel<U>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              scc_fwd_lds<U>());
    (void)hipGetLastError();
  });
  hipLaunchKernelGGL(scc_critic_fwd_kernel<U>, dim3((unsigned)blocks, (unsigned)a.net.n, (unsigned)nset), dim3(U * 4), scc_fwd_lds<U>(), st, a);
  XT_LAUNCH_CHECK();
  return 0;
}

// workgroups per (agent, set): enough tiles each that staging L2 is paid back, at most one per tile
static int scc_blocks(int R) {
  const int ntile = (R + 15) / 16;
  const int b = (ntile + 3) / 4;
  return b < 1 ? 1 : (b > 256 ? 256 : b);
}

static int launch_scc_fwd(const SccCriticFwd& a, int U, int nset, hipStream_t st) {
  const int blocks = scc_blocks(a.src.B * a.src.T);
  if (U == 128) return launch_scc_fwd_u<128>(a, nset, blocks, st);
  if (U == 64) return launch_scc_fwd_u<64>(a, nset, blocks, st);
  return launch_scc_fwd_u<32>(a, nset, blocks, st);
}

// ------------------------------------------------------------------ TD error, dv and the credits, one thread per row
struct SccTd {
  const float* sc;                       // [3, n R]
  const float *bv_e, *bv_t;              // the final Dense's bias of the eval / target set
  const float *rewards, *terminated, *mask;      // [R] or null (then only v and the credits are formed)
  const double* masksum;
  float gamma;
  int R, n;
  float* credits;                        // [R, n]
  float* dv;                             // [R] or null
  double* rowloss;                       // [R] or null
  float* v;                              // [R] v_eval, or null
  double* alivesum;                      // 1 double = n sum(mask), or null
};

__global__ __launch_bounds__(256) void scc_td_kernel(const SccTd a) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r == 0 && a.alivesum) a.alivesum[0] = (double)a.n * a.masksum[0];
  if (r >= a.R) return;
  const long long NR = (long long)a.n * a.R;
  float ve = a.bv_e[0], vt = a.bv_t ? a.bv_t[0] : 0.f;
  for (int i = 0; i < a.n; ++i) {
    const float full = a.sc[(long long)i * a.R + r];
    ve = ve + full;
    if (a.bv_t) vt = vt + a.sc[2 * NR + (long long)i * a.R + r];
    a.credits[(long long)r * a.n + i] = full - a.sc[NR + (long long)i * a.R + r];
  }
  if (a.rewards) {
    const float y = a.rewards[r] + a.gamma * (1.f - a.terminated[r]) * vt;
    const float mk = a.mask[r];
    const float mtd = (ve - y) * mk;
    a.rowloss[r] = (double)mtd * (double)mtd;
    a.dv[r] = (float)(2.0 * (double)(mtd * mk) / a.masksum[0]);
  }
  if (a.v) a.v[r] = ve;
}

// ------------------------------------------------------------------ the critic's backward
struct SccCriticBwd {
  const float* p;
  SccNet net;
  const float *dv, *h1, *h2;
  float *dh1, *dh2;                      // [n R, U]
  int R;
};

template <int U>
__global__ __launch_bounds__(U * 4) void scc_critic_bwd_kernel(const SccCriticBwd a) {
  constexpr int LDB = U + 16, LDH = U + 1, NT = U * 4;
  extern __shared__ float lds[];
  float* l2t = lds;                      // [U][LDB]: l2t[k][c] = L2[c][k]
  float* ds = l2t + U * LDB;             // [16][LDH]
  const int i = blockIdx.y, tid = threadIdx.x;
  const int w = tid >> 6, l = tid & 63, j = l & 15, g = l >> 4, col = 16 * w + j;
  const int R = a.R;
  const float* __restrict__ L2 = a.p + a.net.l1[i] + scc_dal4(a.net.KA * U) + scc_dal4(U);
  const float* __restrict__ wv = a.p + a.net.wv + (a.net.merge_add ? 0 : i * U);
  for (int e = tid; e < U * U; e += NT) l2t[(e % U) * LDB + e / U] = L2[e];
  const int ntile = (R + 15) >> 4;
  for (int tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
    const int r0 = tile * 16;
    __syncthreads();
    for (int e = tid; e < 16 * U; e += NT) {
      const int row = e / U, k = e % U, r = r0 + row;
      float d = 0.f;
      if (r < R) {
        const long long idx = ((long long)i * R + r) * U + k;
        d = a.h2[idx] > 0.f ? a.dv[r] * wv[k] : 0.f;
        a.dh2[idx] = d;
      }
      ds[row * LDH + k] = d;
    }
    __syncthreads();
    qm_f4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
    for (int kk = 0; kk < U / 4; ++kk)
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(ds[j * LDH + 4 * kk + g], l2t[(4 * kk + g) * LDB + col], acc, 0, 0, 0);
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int r = r0 + 4 * g + v;
      if (r < R) {
        const long long idx = ((long long)i * R + r) * U + col;
        a.dh1[idx] = a.h1[idx] > 0.f ? acc[v] : 0.f;
      }
    }
  }
}

template <int U>
static int launch_scc_bwd_u(const SccCriticBwd& a, hipStream_t st) {
  static PerDeviceOnce attr_once;
  attr_once.run([] {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(scc_critic_bwd_kernel<U>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              scc_bwd_lds<U>());
    (void)hipGetLastError();
  });
  hipLaunchKernelGGL(scc_critic_bwd_kernel<U>, dim3((unsigned)scc_blocks(a.R), (unsigned)a.net.n), dim3(U * 4), scc_bwd_lds<U>(), st, a);
  XT_LAUNCH_CHECK();
  return 0;
}

static int launch_scc_bwd(const SccCriticBwd& a, int U, hipStream_t st) {
  if (U == 128) return launch_scc_bwd_u<128>(a, st);
  if (U == 64) return launch_scc_bwd_u<64>(a, st);
  return launch_scc_bwd_u<32>(a, st);
}

// ------------------------------------------------------------------ weight gradients, slab-ordered as dense_wgrad_kernel
// dL1 [o + A, U] | db1 [U] of one group: the rows are the group's items (agent-major), the x element is the observation below o,
// the one-hot of the action from o to o + A (made here, never stored), 1 for the bias
struct SccWgrad1 {
  SccSrc src;
  const float* dy;                       // dh1 of the group's first item
  int U, n, i0, M, nslab;                // M = agents of the group * R
  float* out;                            // [nslab, (o + A + 1) * U]
};

__global__ __launch_bounds__(256) void scc_wgrad1_kernel(const SccWgrad1 a) {
  const SccSrc& s = a.src;
  const long long count = (long long)(s.K + s.A + 1) * a.U;
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  if (gid >= count * a.nslab) return;
  const int sl = (int)(gid / count), e = (int)(gid % count);
  const int kk = e / a.U, c = e % a.U, R = s.B * s.T;
  const int m0 = sl * kQmWgradRows, m1 = m0 + kQmWgradRows < a.M ? m0 + kQmWgradRows : a.M;
  float acc = 0.f;
  for (int m = m0; m < m1; ++m) {
    const float dy = a.dy[(long long)m * a.U + c];
    if (kk < s.K + s.A) {
      const int ia = a.i0 + m / R, r = m % R, b = r / s.T, t = scc_src_t(s, r % s.T);
      if (kk < s.K) acc = acc + s.x[((long long)(b * s.Tsrc + t) * a.n + ia) * s.ldx + kk] * dy;
      else if (s.actions[(b * s.T + t) * a.n + ia] == kk - s.K) acc = acc + dy;
    } else {
      acc = acc + dy;
    }
  }
  a.out[gid] = acc;
}

// the final Dense: dw[i U + k] = sum_r dv_r h2[i, r, k] (concat) or dw[k] = sum_i sum_r (add); db = sum_r dv_r
struct SccVgrad {
  const float *h2, *dv;
  int U, R, n, per_agent, nslab;
  float* out;                            // [nslab, nW + 1]
};

__global__ __launch_bounds__(256) void scc_vgrad_kernel(const SccVgrad a) {
  const int nW = a.per_agent ? a.n * a.U : a.U;
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  if (gid >= (long long)(nW + 1) * a.nslab) return;
  const int sl = (int)(gid / (nW + 1)), e = (int)(gid % (nW + 1));
  const int M = e == nW || a.per_agent ? a.R : a.n * a.R;
  const int m0 = sl * kQmWgradRows, m1 = m0 + kQmWgradRows < M ? m0 + kQmWgradRows : M;
  const long long base = e < nW && a.per_agent ? (long long)(e / a.U) * a.R : 0;
  const int k = e % a.U;
  float acc = 0.f;
  for (int m = m0; m < m1; ++m) {
    const float dv = a.dv[m % a.R];
    acc = e == nW ? acc + dv : acc + a.h2[(base + m) * a.U + k] * dv;
  }
  a.out[gid] = acc;
}

// ------------------------------------------------------------------ the actor's head, one thread per (row, agent)
struct SccActor {
  const float* q;                        // [T + 1, S, A] time-major, the eval agent
  const int32_t* actions;                // [B, T, n]
  const float *credits, *mask;           // [R, n], [R]
  const double* alivesum;
  int B, T, n, A;
  float* dq;                             // [T + 1, S, A]
  double* rowloss;                       // [R n]
};

__global__ __launch_bounds__(256) void scc_actor_head_kernel(const SccActor a) {
  const int it = blockIdx.x * 256 + threadIdx.x;
  if (it >= a.B * a.T * a.n) return;
  const int r = it / a.n, i = it % a.n, b = r / a.T, t = r % a.T, S = a.B * a.n;
  const int act = a.actions[it];
  const float* q = a.q + ((long long)t * S + b * a.n + i) * a.A;
  const float chosen = act >= 0 && act < a.A ? q[act] : 0.f;      // (tf.one_hot: an index outside the depth makes a zero row)
  const float alive = a.mask[r];
  const float d = chosen * alive - a.credits[it] * alive;         // alive is applied to both sides, as the reference does
  a.rowloss[it] = (double)d * (double)d;
  const float g = (float)(2.0 * (double)(d * alive) / a.alivesum[0]);
  float* dq = a.dq + ((long long)t * S + b * a.n + i) * a.A;
  for (int c = 0; c < a.A; ++c) {
    dq[c] = c == act ? g : 0.f;
    if (t == a.T - 1) dq[(long long)S * a.A + c] = 0.f;           // the last step's rows: no chosen action reads them
  }
}

// ------------------------------------------------------------------ the optimisers; blockIdx.y = tensor of the chunk
// TF1's ApplyAdam: alpha = lr sqrt(1 - b2^t) / (1 - b1^t); m += (g - m)(1 - b1); v += (g g - v)(1 - b2); p -= m alpha / (sqrt(v) + eps)
__global__ __launch_bounds__(256) void scc_adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                       float* __restrict__ v, const QmSegs s, const double* __restrict__ norm2, float lr,
                                                       float b1, float b2, float eps, float clip, const float* __restrict__ state,
                                                       float* __restrict__ norms) {
  const int seg = blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;
  const float norm = (float)sqrt(norm2[seg]);
  if (i == 0) norms[seg] = norm;
  if (i >= s.cnt[seg]) return;
  const double t = (double)state[0] + 1.0;
  const float alpha = (float)((double)lr * sqrt(1.0 - pow((double)b2, t)) / (1.0 - pow((double)b1, t)));
  const long long o = (long long)s.off[seg] + i;
  const float gc = clip > 0.f ? (g[o] * clip) / fmaxf(norm, clip) : g[o];
  const float m1 = m[o] + (gc - m[o]) * (1.f - b1);
  const float v1 = v[o] + (gc * gc - v[o]) * (1.f - b2);
  m[o] = m1;
  v[o] = v1;
  p[o] = p[o] - (m1 * alpha) / (sqrtf(v1) + eps);
}

// TF1's ApplyRMSProp, momentum 0: ms += (g g - ms)(1 - rho); p -= g lr / sqrt(ms + eps)
__global__ __launch_bounds__(256) void scc_rmsprop_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ ms,
                                                          const QmSegs s, const double* __restrict__ norm2, float lr, float decay, float eps,
                                                          float clip, float* __restrict__ norms) {
  const int seg = blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;
  const float norm = (float)sqrt(norm2[seg]);
  if (i == 0) norms[seg] = norm;
  if (i >= s.cnt[seg]) return;
  const long long o = (long long)s.off[seg] + i;
  const float gc = clip > 0.f ? (g[o] * clip) / fmaxf(norm, clip) : g[o];
  const float ms1 = ms[o] + (gc * gc - ms[o]) * (1.f - decay);
  ms[o] = ms1;
  p[o] = p[o] - (gc * lr) / sqrtf(ms1 + eps);
}

__global__ void scc_count_kernel(float* state) { state[0] = state[0] + 1.f; }

}  // namespace xt

// ------------------------------------------------------------------ the handle
struct xt_scc {
  xt_scc_desc d;
  int max_batch, o, nt;                  // o = obs_dim - n_actions - n_agents; nt tensors
  int64_t off[XT_SCC_MAX_TENSORS + 1];
  int cnt[XT_SCC_MAX_TENSORS];
  int gstart[XT_SCC_MAX_GROUPS + 1];     // first agent of every group
  xt::SccNet net;
  float *pe, *pt, *grads, *s1, *s2, *state, *ws;
  int64_t ws_floats;
  int64_t o_x1, o_xg, o_out, o_q, o_saved, o_dq, o_dout, o_dg3, o_dx1;
  int64_t o_sc, o_h1, o_h2, o_dh1, o_dh2, o_credits, o_dv, o_slabs, o_rowloss, o_scalars;
};

namespace xt {

static int scc_check_desc(const xt_scc_desc& d, const char* who) {
  XT_REQUIRE(d.multi_channel != 0, "%s: enable_critic_multi_channel = False (the plain critic is not additive over the agents; the "
             "credits kernel rests on that)", who);
  XT_REQUIRE(d.merge == XT_SCC_MERGE_CONCAT || d.merge == XT_SCC_MERGE_ADD, "%s: channel_merge = %d is neither concat nor add", who, d.merge);
  XT_REQUIRE(d.units == 32 || d.units == 64 || d.units == 128, "%s: dense_unit_number = %d (the critic kernels take 32, 64 or 128)", who,
             d.units);
  XT_REQUIRE(d.hidden == 32 || d.hidden == 64, "%s: rnn_hidden_dim = %d (the recurrent kernels take 32 or 64)", who, d.hidden);
  XT_REQUIRE(d.n_agents >= 1 && d.n_agents <= 32 && d.n_actions >= 1 && d.n_actions <= 64,
             "%s: n_agents = %d, n_actions = %d beyond the kernels' limits (32, 64)", who, d.n_agents, d.n_actions);
  const int o = d.obs_dim - d.n_actions - d.n_agents;
  XT_REQUIRE(o >= 1 && d.obs_dim <= 65536, "%s: obs_shape = %d leaves a raw observation of %d columns", who, d.obs_dim, o);
  XT_REQUIRE(o + d.n_actions <= 1024, "%s: o + n_actions = %d above 1024", who, o + d.n_actions);
  XT_REQUIRE(d.seq_len >= 1 && d.seq_len <= 65536, "%s: seq_len = %d out of range", who, d.seq_len);
  XT_REQUIRE(d.n_groups >= 1 && d.n_groups <= XT_SCC_MAX_GROUPS, "%s: %d agent groups", who, d.n_groups);
  int sum = 0;
  for (int g = 0; g < d.n_groups; ++g) {
    XT_REQUIRE(d.groups[g] >= 1, "%s: agent group %d has %d agents", who, g, d.groups[g]);
    sum += d.groups[g];
  }
  XT_REQUIRE(sum == d.n_agents, "%s: agent_group sums to %d, n_agents = %d", who, sum, d.n_agents);
  return 0;
}

static int scc_layout(const xt_scc_desc& d, int64_t* off, int* cnt) {
  const int D = d.obs_dim, H = d.hidden, A = d.n_actions, U = d.units, KA = D - d.n_agents;
  int c[XT_SCC_MAX_TENSORS] = {D * H, H, 4 * H * H, 2 * H, 2 * H * H, H, H * A, A};
  int nt = kSccAgentTensors;
  for (int g = 0; g < d.n_groups; ++g) { c[nt++] = KA * U; c[nt++] = U; c[nt++] = U * U; c[nt++] = U; }
  c[nt++] = d.merge == XT_SCC_MERGE_ADD ? U : d.n_agents * U;
  c[nt++] = 1;
  int64_t o = 0;
  for (int i = 0; i < nt; ++i) {
    off[i] = o;
    if (cnt) cnt[i] = c[i];
    o += al4(c[i]);
  }
  off[nt] = o;
  return nt;
}

static void scc_plan(xt_scc* z) {
  const xt_scc_desc& d = z->d;
  const int64_t B = z->max_batch, T = d.seq_len, T1 = T + 1, n = d.n_agents, S = B * n, M = T1 * S, R = B * T, NR = n * R;
  const int64_t H = d.hidden, A = d.n_actions, U = d.units, D = d.obs_dim, KA = D - n;
  int64_t off = 0;
  auto take = [&](int64_t k) { const int64_t o = off; off += al4(k); return o; };
  z->o_x1 = take(M * H); z->o_xg = take(M * 3 * H); z->o_out = take(M * H); z->o_q = take(M * A); z->o_saved = take(M * 4 * H);
  z->o_dq = take(M * A); z->o_dout = take(M * H); z->o_dg3 = take(M * 3 * H); z->o_dx1 = take(M * H);
  z->o_sc = take(3 * NR); z->o_h1 = take(NR * U); z->o_h2 = take(NR * U); z->o_dh1 = take(NR * U); z->o_dh2 = take(NR * U);
  z->o_credits = take(NR); z->o_dv = take(R);
  const int64_t km = (D > H ? D : H) + 1, nm = 2 * H > A ? 2 * H : A;
  int64_t sl = qm_nslab(M) * km * nm;
  const int64_t sc1 = qm_nslab(NR) * ((KA > U ? KA : U) + 1) * U, sc2 = qm_nslab(NR) * (n * U + 1);
  sl = sl > sc1 ? sl : sc1;
  z->o_slabs = take(sl > sc2 ? sl : sc2);
  z->o_rowloss = take(2 * (R + NR) + 4);          // doubles: the critic's rows, then the actor's
  z->o_scalars = take(2 * (4 + z->nt));           // doubles: [0] sum(mask), [1] n sum(mask), [4 ..] the tensors' squared norms
  z->ws_floats = off;
}

// the agent's view of the handle: its tensors and its part of the workspace (one parameter set per forward)
static RnnAgent scc_agent(const xt_scc* z) {
  RnnAgent g{};
  g.obs_dim = z->d.obs_dim; g.H = z->d.hidden; g.A = z->d.n_actions; g.n = z->d.n_agents;
  for (int i = 0; i < kSccAgentTensors; ++i) g.off[i] = z->off[i];
  float* ws = z->ws;
  g.x1[0] = ws + z->o_x1; g.xg[0] = ws + z->o_xg; g.out[0] = ws + z->o_out; g.q[0] = ws + z->o_q;
  g.saved = ws + z->o_saved; g.dq = ws + z->o_dq; g.dout = ws + z->o_dout; g.dg3 = ws + z->o_dg3; g.dx1 = ws + z->o_dx1;
  g.slabs = ws + z->o_slabs;
  return g;
}

static SccSrc scc_src(const xt_scc* z, const float* x, const int32_t* actions, int B, bool raw) {
  SccSrc s{};
  s.x = x; s.actions = raw ? nullptr : actions; s.A = z->d.n_actions; s.B = B; s.T = z->d.seq_len;
  s.K = raw ? z->o + z->d.n_actions : z->o; s.ldx = s.K; s.Tsrc = raw ? s.T : s.T + 1; s.shift = raw ? 0 : 1;
  return s;
}

// the critic pass: the three scalars per item (the target's only with p_tgt), h1 / h2 of the eval set when `save`
static int scc_critic_fwd(const xt_scc* z, const float* p_eval, const float* p_tgt, const SccSrc& src, bool save, hipStream_t st) {
  SccCriticFwd f{};
  f.p[0] = p_eval; f.p[1] = p_tgt; f.net = z->net; f.src = src; f.alt_zero = z->d.n_agents <= 2; f.sc = z->ws + z->o_sc;
  f.h1 = save ? z->ws + z->o_h1 : nullptr; f.h2 = save ? z->ws + z->o_h2 : nullptr;
  return launch_scc_fwd(f, z->d.units, p_tgt ? 2 : 1, st);
}

// all critic gradients of dv [R] into `grads` (a flat set), from the h1 / h2 the forward saved
static int scc_critic_bwd(const xt_scc* z, const float* p_eval, const SccSrc& src, const float* dv, float* grads, hipStream_t st) {
  const xt_scc_desc& d = z->d;
  const int U = d.units, n = d.n_agents, R = src.B * src.T;
  float* ws = z->ws;
  float* slabs = ws + z->o_slabs;
  SccCriticBwd b{};
  b.p = p_eval; b.net = z->net; b.dv = dv; b.h1 = ws + z->o_h1; b.h2 = ws + z->o_h2; b.dh1 = ws + z->o_dh1; b.dh2 = ws + z->o_dh2; b.R = R;
  if (int rc = launch_scc_bwd(b, U, st)) return rc;
  for (int g = 0; g < d.n_groups; ++g) {
    const int i0 = z->gstart[g], M = d.groups[g] * R, t0 = kSccAgentTensors + 4 * g;
    const long long row0 = (long long)i0 * R * U;
    DenseWgrad w2{};
    w2.x = ws + z->o_h1 + row0; w2.ldx = U; w2.dy = ws + z->o_dh2 + row0; w2.ldy = U; w2.M = M; w2.K = U; w2.N = U;
    if (int rc = launch_dense_wgrad(w2, grads + z->off[t0 + 2], grads + z->off[t0 + 3], slabs, kQmWgradRows, false, st)) return rc;
    SccWgrad1 w1{};
    w1.src = src; w1.dy = ws + z->o_dh1 + row0; w1.U = U; w1.n = n; w1.i0 = i0; w1.M = M; w1.nslab = qm_nslab(M); w1.out = slabs;
    const long long count = (long long)(src.K + src.A + 1) * U, nw = (long long)(src.K + src.A) * U;
    hipLaunchKernelGGL(scc_wgrad1_kernel, dim3((unsigned)((count * w1.nslab + 255) / 256)), dim3(256), 0, st, w1);
    XT_LAUNCH_CHECK();
    if (int rc = launch_slab_sum(slabs, count, nw, w1.nslab, grads + z->off[t0], grads + z->off[t0 + 1], st)) return rc;
  }
  SccVgrad v{};
  v.h2 = ws + z->o_h2; v.dv = dv; v.U = U; v.R = R; v.n = n; v.per_agent = d.merge == XT_SCC_MERGE_CONCAT;
  v.nslab = qm_nslab(v.per_agent ? R : (long long)n * R); v.out = slabs;
  const long long nW = v.per_agent ? n * U : U;
  hipLaunchKernelGGL(scc_vgrad_kernel, dim3((unsigned)(((nW + 1) * v.nslab + 255) / 256)), dim3(256), 0, st, v);
  XT_LAUNCH_CHECK();
  const int tv = kSccAgentTensors + 4 * d.n_groups;
  return launch_slab_sum(slabs, nW + 1, nW, v.nslab, grads + z->off[tv], grads + z->off[tv + 1], st);
}

}  // namespace xt

extern "C" {

int xt_scc_layout(const xt_scc_desc* desc, int64_t* offsets, int32_t* n_tensors) {
  using namespace xt;
  XT_REQUIRE(desc && offsets, "xt_scc_layout: null argument");
  if (int rc = scc_check_desc(*desc, "xt_scc_layout")) return rc;
  const int nt = scc_layout(*desc, offsets, nullptr);
  if (n_tensors) *n_tensors = nt;
  return 0;
}

int xt_scc_create(const xt_scc_desc* desc, int32_t max_batch, xt_scc** out) {
  using namespace xt;
  XT_REQUIRE(desc && out, "xt_scc_create: null argument");
  *out = nullptr;
  if (int rc = scc_check_desc(*desc, "xt_scc_create")) return rc;
  XT_REQUIRE(max_batch >= 1 && max_batch <= (1 << 20), "xt_scc_create: max_batch = %d outside [1, 2^20]", max_batch);
  const xt_scc_desc& d = *desc;
  const long long M = (long long)(d.seq_len + 1) * max_batch * d.n_agents;
  long long widest = 4ll * d.hidden > d.obs_dim ? 4ll * d.hidden : d.obs_dim;
  widest = widest > d.units ? widest : d.units;
  XT_REQUIRE(M * widest < (1ll << 31), "xt_scc_create: (seq_len + 1) * max_batch * n_agents * %lld elements exceed 2^31", widest);
  xt_scc* z = new (std::nothrow) xt_scc();
  XT_REQUIRE(z, "xt_scc_create: out of memory");
  z->d = d;
  z->max_batch = max_batch;
  z->o = d.obs_dim - d.n_actions - d.n_agents;
  z->nt = scc_layout(d, z->off, z->cnt);
  z->net.KA = z->o + d.n_actions; z->net.n = d.n_agents; z->net.merge_add = d.merge == XT_SCC_MERGE_ADD;
  z->net.wv = (int)z->off[kSccAgentTensors + 4 * d.n_groups];
  int i = 0;
  for (int g = 0; g < d.n_groups; ++g) {
    z->gstart[g] = i;
    for (int k = 0; k < d.groups[g]; ++k) z->net.l1[i++] = (int)z->off[kSccAgentTensors + 4 * g];
  }
  z->gstart[d.n_groups] = i;
  scc_plan(z);
  *out = z;
  return 0;
}

void xt_scc_destroy(xt_scc* h) { delete h; }

int64_t xt_scc_workspace_bytes(const xt_scc* h) { return h ? h->ws_floats * 4 : 0; }

int xt_scc_bind(xt_scc* h, float* params_eval, float* params_target, float* grads, float* slot1, float* slot2, float* state,
                void* workspace, int64_t workspace_bytes) {
  XT_REQUIRE(h && params_eval && params_target && grads && slot1 && slot2 && state && workspace, "xt_scc_bind: null argument");
  XT_REQUIRE(workspace_bytes >= h->ws_floats * 4, "xt_scc_bind: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
             (long long)h->ws_floats * 4);
  XT_REQUIRE((((uintptr_t)params_eval | (uintptr_t)params_target | (uintptr_t)grads | (uintptr_t)slot1 | (uintptr_t)slot2 |
               (uintptr_t)workspace) & 15) == 0, "xt_scc_bind: buffers must be 16-byte aligned");
  h->pe = params_eval; h->pt = params_target; h->grads = grads; h->s1 = slot1; h->s2 = slot2; h->state = state;
  h->ws = static_cast<float*>(workspace);
  return 0;
}

int xt_scc_step(xt_scc* h, const float* agent_obs, const float* obs, const int32_t* lens, const int32_t* actions, const float* rewards,
                const float* terminated, const float* mask, int32_t B, const xt_scc_cfg* cfg, double* loss_out, void* stream) {
  using namespace xt;
  if (int rc = check_bound(h, &xt_scc::pe, B, "xt_scc_step")) return rc;
  XT_REQUIRE(agent_obs && obs && actions && rewards && terminated && mask && cfg && loss_out, "xt_scc_step: null argument");
  const xt_scc* z = h;
  const xt_scc_desc& d = z->d;
  const hipStream_t st = as_stream(stream);
  const int n = d.n_agents, T = d.seq_len, R = B * T, NR = n * R, tv = kSccAgentTensors + 4 * d.n_groups;
  float* ws = z->ws;
  double* scal = reinterpret_cast<double*>(ws + z->o_scalars);
  double* rowloss = reinterpret_cast<double*>(ws + z->o_rowloss);

  // ---- the critic: one pass, the TD error, the credits (from the eval critic before its update), the backward
  const SccSrc src = scc_src(z, obs, actions, B, false);
  if (int rc = scc_critic_fwd(z, z->pe, z->pt, src, true, st)) return rc;
  if (int rc = launch_dense_sum(mask, (long long)R, nullptr, scal, st)) return rc;
  SccTd td{};
  td.sc = ws + z->o_sc; td.bv_e = z->pe + z->off[tv + 1]; td.bv_t = z->pt + z->off[tv + 1]; td.rewards = rewards; td.terminated = terminated;
  td.mask = mask; td.masksum = scal; td.gamma = cfg->gamma; td.R = R; td.n = n; td.credits = ws + z->o_credits; td.dv = ws + z->o_dv;
  td.rowloss = rowloss; td.alivesum = scal + 1;
  hipLaunchKernelGGL(scc_td_kernel, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, st, td);
  XT_LAUNCH_CHECK();
  if (int rc = launch_dense_sum((const double*)rowloss, (long long)R, scal, loss_out + 1, st)) return rc;
  if (int rc = scc_critic_bwd(z, z->pe, src, ws + z->o_dv, z->grads, st)) return rc;

  // ---- the actor: the agent's forward, the head against the credits, the agent's backward
  const RnnAgent ag = scc_agent(z);
  if (int rc = agent_fwd(ag, &z->pe, 1, agent_obs, B, T + 1, nullptr, lens, true, nullptr, nullptr, st)) return rc;
  SccActor ac{};
  ac.q = ws + z->o_q; ac.actions = actions; ac.credits = ws + z->o_credits; ac.mask = mask; ac.alivesum = scal + 1; ac.B = B; ac.T = T;
  ac.n = n; ac.A = d.n_actions; ac.dq = ws + z->o_dq; ac.rowloss = rowloss + R;
  hipLaunchKernelGGL(scc_actor_head_kernel, dim3((unsigned)((NR + 255) / 256)), dim3(256), 0, st, ac);
  XT_LAUNCH_CHECK();
  if (int rc = launch_dense_sum((const double*)(rowloss + R), (long long)NR, scal + 1, loss_out, st)) return rc;
  return agent_bwd(ag, z->pe, z->grads, agent_obs, lens, B, T + 1, st);
}

int xt_scc_apply(xt_scc* h, const xt_scc_cfg* cfg, void* stream) {
  using namespace xt;
  XT_REQUIRE(h && h->pe && h->ws && cfg, "xt_scc_apply: the handle is not bound");
  const hipStream_t st = as_stream(stream);
  double* norm2 = reinterpret_cast<double*>(h->ws + h->o_scalars) + 4;
  // (the reference gates both clips on actor_grad_norm_clip > 0)
  const bool clip = cfg->actor_clip > 0.f;
  for (int t0 = 0; t0 < h->nt;) {        // chunks of one optimiser, at most a QmSegs each: the agent's 8 tensors, then the critic's
    const bool agent = t0 < kSccAgentTensors;
    const int end = agent ? kSccAgentTensors : h->nt;
    QmSegs s{};
    int widest = 0;
    for (; t0 < end && s.n < kQmTensors; ++t0, ++s.n) {
      s.off[s.n] = (int)h->off[t0]; s.cnt[s.n] = h->cnt[t0];
      widest = h->cnt[t0] > widest ? h->cnt[t0] : widest;
    }
    const int first = t0 - s.n;
    hipLaunchKernelGGL(qmix_norm_kernel, dim3(s.n), dim3(256), 0, st, h->grads, s, norm2 + first);
    XT_LAUNCH_CHECK();
    const dim3 grid((unsigned)((widest + 255) / 256), s.n);
    if (agent)
      hipLaunchKernelGGL(scc_rmsprop_kernel, grid, dim3(256), 0, st, h->pe, h->grads, h->s2, s, norm2 + first, cfg->a_lr, cfg->rms_decay,
                         cfg->rms_eps, clip ? cfg->actor_clip : 0.f, h->state + 8 + first);
    else
      hipLaunchKernelGGL(scc_adam_kernel, grid, dim3(256), 0, st, h->pe, h->grads, h->s1, h->s2, s, norm2 + first, cfg->c_lr, cfg->beta1,
                         cfg->beta2, cfg->adam_eps, clip ? cfg->mixer_clip : 0.f, h->state, h->state + 8 + first);
    XT_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(scc_count_kernel, dim3(1), dim3(1), 0, st, h->state);      // behind the Adam launches, which read the count
  XT_LAUNCH_CHECK();
  return 0;
}

int xt_scc_sync_target(xt_scc* h, void* stream) {
  XT_REQUIRE(h && h->pe && h->pt, "xt_scc_sync_target: the handle is not bound");
  const int64_t c0 = h->off[xt::kSccAgentTensors];
  XT_CHECK_HIP(hipMemcpyAsync(h->pt + c0, h->pe + c0, (size_t)(h->off[h->nt] - c0) * 4, hipMemcpyDeviceToDevice, xt::as_stream(stream)));
  return 0;
}

int xt_scc_agent_forward(xt_scc* h, const float* agent_params, const float* obs, int32_t B, int32_t T, const float* hidden_in,
                         const int32_t* lens, float* q, float* hidden_out, void* stream) {
  using namespace xt;
  if (int rc = check_bound(h, &xt_scc::pe, B, "xt_scc_agent_forward")) return rc;
  XT_REQUIRE(agent_params && obs && q, "xt_scc_agent_forward: null argument");
  XT_REQUIRE(T >= 1 && T <= h->d.seq_len + 1, "xt_scc_agent_forward: T = %d outside [1, %d]", T, h->d.seq_len + 1);
  return agent_fwd(scc_agent(h), &agent_params, 1, obs, B, T, hidden_in, lens, false, q, hidden_out, as_stream(stream));
}

int xt_scc_critic(xt_scc* h, const float* params_eval, const float* params_target, const float* obs, const int32_t* actions, int32_t B,
                  int32_t raw, float* scalars, float* credits, float* v, const float* dv, float* grads, void* stream) {
  using namespace xt;
  if (int rc = check_bound(h, &xt_scc::pe, B, "xt_scc_critic")) return rc;
  XT_REQUIRE(params_eval && obs && (raw || actions), "xt_scc_critic: null argument");
  XT_REQUIRE(!dv == !grads && !(raw && dv), "xt_scc_critic: gradients take dv and grads, and the placeholder layout of obs");
  XT_REQUIRE(!(raw && (scalars || credits)), "xt_scc_critic: a raw critic state has no actions to zero: it yields v alone");
  const xt_scc* z = h;
  const hipStream_t st = as_stream(stream);
  const int n = z->d.n_agents, R = B * z->d.seq_len, tv = kSccAgentTensors + 4 * z->d.n_groups;
  const SccSrc src = scc_src(z, obs, actions, B, raw != 0);
  if (int rc = scc_critic_fwd(z, params_eval, params_target, src, dv != nullptr, st)) return rc;
  if (scalars)
    XT_CHECK_HIP(hipMemcpyAsync(scalars, z->ws + z->o_sc, (size_t)(params_target ? 3 : 2) * n * R * 4, hipMemcpyDeviceToDevice, st));
  SccTd td{};
  td.sc = z->ws + z->o_sc; td.bv_e = params_eval + z->off[tv + 1]; td.bv_t = params_target ? params_target + z->off[tv + 1] : nullptr;
  td.R = R; td.n = n; td.credits = credits ? credits : z->ws + z->o_credits; td.v = v;
  hipLaunchKernelGGL(scc_td_kernel, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, st, td);
  XT_LAUNCH_CHECK();
  if (dv) return scc_critic_bwd(z, params_eval, src, dv, grads, st);
  return 0;
}

}  // extern "C"
