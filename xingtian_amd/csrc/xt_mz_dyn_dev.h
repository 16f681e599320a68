// MuZero: the dynamics unroll in two persistent kernels on fp32 matrix cores (included by xt_muzero.hip only).
//
// The dynamics chain is the one sequential part of xt_mz_step, and row b of step i + 1 depends on row b of step i alone.
// So one workgroup OWNS a tile of R = 16 RT batch rows for the whole unroll and walks the steps itself:
//   forward   i = 0 .. U-1:  t_0 = relu(h_i W0[:H] + W0[H + a_i] + b0), t_l = relu(t_{l-1} W_l + b_l), h_{i+1} = relu(t_last Wh + bh)
//   backward  i = U-1 .. 0:  dt_last = relu'(t_last) (tr + dpre(h_{i+1}) Wh^T), dt_{l-1} = relu'(t_{l-1}) (dt_l W_l^T),
//                            dpre(h_i) = relu'(h_i) (g_pred(h_i) + c dt_0 W0[:H]^T),  c = 0.5 (i >= 1) or 1 (i = 0)
// Both are the same walk over a table of layers (MzDynChain): the backward reads the transposed kernels that
// mz_transpose_all forms once per step, so its product is the forward's, y[R, N] = x[R, K] . w[K, N] with w row-major.
//
// Work split: kMzDynWaves wavefronts; wavefront v owns the 16-column output tiles v, v + kMzDynWaves, ... of every layer and,
// per tile, one accumulator for each of the RT 16-row sub-tiles -- a weight fragment is loaded once and used RT times.
// v_mfma_f32_16x16x4_f32 (the lane layout at the top of xt_qmix_dev.h): lane l = 16 g + j holds A[row j][k], B[k][column j] for
// ONE k of the instruction's four, and D[row 4 g + v][column j].  Which four k one instruction sums is free as long as A and
// B agree; here instruction kk of the 16-wide chunk c takes k = 16 c + 4 g + kk, so a lane's four A values of a chunk are one
// 16-byte LDS read.
// Data movement: the tile's current activation lives in LDS, two ping-pong buffers [R][ld], ld = widest layer + 4 floats (rows
// stay 16-byte aligned; ld = 4 mod 32 spreads the 16 rows of a b128 read over the banks).  A layer reads one buffer as the A
// operand and its epilogue writes the other, and the same value to the global buffer the rest of the step reads; one barrier
// per layer.  h_{i+1} / dpre(h_{i+1}) is simply the buffer the last layer of a step wrote: it never comes back from global
// memory.  The B fragments stream from global / L2 through a register ring kMzDynRing chunks deep: the slot an instruction
// group has just consumed is refilled with the chunk kMzDynRing ahead before the group's MFMAs issue.
// LDS per workgroup: 2 R ld floats.  The cap on every width is kMzDynMaxWidth = 256: ld = 260, 33,280 bytes at R = 16 and
// 66,560 bytes at R = 32, so two workgroups of either form still fit one CU's 160 KiB.
// Rows at and past B of the last tile are zero in LDS and touch no global address.  No atomics: a row's sums have a fixed
// order, two runs give the same bits (not the bits of dense_gemm_kernel: the matrix core sums four k at a time).
#pragma once
#include "xt_common.h"

namespace xt {
namespace {

typedef float mz_f4 __attribute__((ext_vector_type(4)));
constexpr int kMzDynWaves = 8;
constexpr int kMzDynRing = 4;            // chunks of 16 k in flight per lane (16 VGPRs)
constexpr int kMzDynMaxWidth = 256;
constexpr int kMzDynMaxLayers = XT_MZ_MAX_CHAIN;
constexpr int kMzDynRowsDefault = 16;    // batch rows per workgroup of xt_mz_set_dyn_fused(on = 1): profiles/muzero_step.md

// Layer p of a step, p = 0 .. nl - 1, in the order the walk takes them.  Every global tensor of layer p is [., N[p]] with the
// rows of step i at [i B, (i + 1) B).
struct MzDynChain {
  int nl, U, B, H, A, ld, a_stride;
  const float* w[kMzDynMaxLayers];       // [K, N] row-major (forward p == 0: H + A rows, the last A the conditioning rows)
  int K[kMzDynMaxLayers], N[kMzDynMaxLayers];
  const float* bias[kMzDynMaxLayers];    // forward
  const float* add[kMzDynMaxLayers];     // backward: null, or the term joined before the mask
  const float* mask[kMzDynMaxLayers];    // backward: the forward activation whose relu is undone
  float* out[kMzDynMaxLayers];
  const int32_t* actions;                // forward: row b of step i took actions[b * a_stride + i]
  const float* x0;                       // forward: h_0 [B, H]; backward: h_U (the mask of the first tile)
  const float* g0;                       // backward: g_pred(h_U) [B, H]
  float* d0;                             // backward: dpre(h_U) [B, H]
};

// out[row][col] = epi(row, col, sum_k in[row][k] w[k][col]) for the R rows of the tile and this wavefront's column tiles
template <int RT, typename Epi>
__device__ __forceinline__ void mz_dyn_layer(const float* __restrict__ in, float* __restrict__ out, int ld, const float* __restrict__ w,
                                             int K, int N, Epi epi) {
  const int wave = threadIdx.x >> 6, l = threadIdx.x & 63, j = l & 15, g = l >> 4;
  const int nchunk = K >> 4;
  for (int tile = wave; tile < (N >> 4); tile += kMzDynWaves) {
    const int col = 16 * tile + j;
    const float* __restrict__ wp = w + (long long)(4 * g) * N + col;       // chunk c, instruction kk: row 16 c + 4 g + kk
    float ring[kMzDynRing][4];
#pragma unroll
    for (int p = 0; p < kMzDynRing; ++p)
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) ring[p][kk] = p < nchunk ? wp[(long long)(16 * p + kk) * N] : 0.f;
    mz_f4 acc[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) acc[rt] = mz_f4{0.f, 0.f, 0.f, 0.f};
    for (int c0 = 0; c0 < nchunk; c0 += kMzDynRing) {
#pragma unroll
      for (int p = 0; p < kMzDynRing; ++p) {
        const int c = c0 + p;
        if (c < nchunk) {                  // (uniform over the workgroup)
          float b[4];
#pragma unroll
          for (int kk = 0; kk < 4; ++kk) b[kk] = ring[p][kk];
          if (c + kMzDynRing < nchunk) {
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) ring[p][kk] = wp[(long long)(16 * (c + kMzDynRing) + kk) * N];
          }
#pragma unroll
          for (int rt = 0; rt < RT; ++rt) {
            const mz_f4 av = *reinterpret_cast<const mz_f4*>(in + (16 * rt + j) * ld + 16 * c + 4 * g);
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) acc[rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[kk], b[kk], acc[rt], 0, 0, 0);
          }
        }
      }
    }
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int row = 16 * rt + 4 * g + v;
        out[row * ld + col] = epi(row, col, acc[rt][v]);
      }
  }
}

// the tile's rows of a [B, H] tensor into LDS through f(global element index); rows at and past B become zero
template <int RT, typename F>
__device__ __forceinline__ void mz_dyn_stage(float* __restrict__ buf, int ld, int H, int B, int r0, F f) {
  for (int e = threadIdx.x; e < 16 * RT * H; e += kMzDynWaves * 64) {
    const int row = e / H, k = e - row * H, m = r0 + row;
    buf[row * ld + k] = m < B ? f((long long)m * H + k) : 0.f;
  }
}

template <int RT>
__global__ __launch_bounds__(kMzDynWaves * 64) void mz_dyn_unroll_fwd_kernel(const MzDynChain a) {
  extern __shared__ __attribute__((aligned(16))) float mz_lds[];
  constexpr int R = 16 * RT;
  const int r0 = blockIdx.x * R, ld = a.ld, B = a.B;
  mz_dyn_stage<RT>(mz_lds, ld, a.H, B, r0, [&](long long e) { return a.x0[e]; });
  __syncthreads();
  int cur = 0;
  for (int i = 0; i < a.U; ++i) {
    for (int p = 0; p < a.nl; ++p) {
      const float* __restrict__ w = a.w[p];
      const float* __restrict__ bias = a.bias[p];
      float* __restrict__ y = a.out[p] + (long long)i * B * a.N[p];
      const int N = a.N[p];
      const bool cond = p == 0;
      mz_dyn_layer<RT>(mz_lds + cur * R * ld, mz_lds + (cur ^ 1) * R * ld, ld, w, a.K[p], N, [&](int row, int col, float v) {
        const int m = r0 + row;
        if (m >= B) return 0.f;
        if (cond) {                        // the conditioning row, gathered: [h | onehot] is never formed
          const int act = a.actions[(long long)m * a.a_stride + i];
          if (act >= 0 && act < a.A) v = v + w[(long long)(a.H + act) * N + col];
        }
        v = v + bias[col];
        v = v > 0.f ? v : 0.f;
        y[(long long)m * N + col] = v;
        return v;
      });
      __syncthreads();
      cur ^= 1;
    }
  }
}

template <int RT>
__global__ __launch_bounds__(kMzDynWaves * 64) void mz_dyn_unroll_bwd_kernel(const MzDynChain a) {
  extern __shared__ __attribute__((aligned(16))) float mz_lds[];
  constexpr int R = 16 * RT;
  const int r0 = blockIdx.x * R, ld = a.ld, B = a.B;
  // step U has no consumer but the prediction net: dpre(h_U) = relu'(h_U) * g_pred(h_U)
  mz_dyn_stage<RT>(mz_lds, ld, a.H, B, r0, [&](long long e) {
    const float v = a.x0[e] > 0.f ? a.g0[e] : 0.f;
    a.d0[e] = v;
    return v;
  });
  __syncthreads();
  int cur = 0;
  for (int i = a.U - 1; i >= 0; --i) {
    for (int p = 0; p < a.nl; ++p) {
      const int N = a.N[p];
      const long long base = (long long)i * B * N;
      const float* __restrict__ add = a.add[p] ? a.add[p] + base : nullptr;
      const float* __restrict__ mask = a.mask[p] + base;
      float* __restrict__ y = a.out[p] + base;
      const float c = p == a.nl - 1 && i >= 1 ? 0.5f : 1.f;      // the hidden-state join behind scale_gradient
      mz_dyn_layer<RT>(mz_lds + cur * R * ld, mz_lds + (cur ^ 1) * R * ld, ld, a.w[p], a.K[p], N, [&](int row, int col, float v) {
        const int m = r0 + row;
        if (m >= B) return 0.f;
        const long long e = (long long)m * N + col;
        v = c * v;                         // scale, add, mask: the order dense_gemm_kernel<., true> documents
        if (add) v = add[e] + v;
        if (!(mask[e] > 0.f)) v = 0.f;
        y[e] = v;
        return v;
      });
      __syncthreads();
      cur ^= 1;
    }
  }
}

template <int RT, bool BWD>
static int launch_mz_dyn_rt(const MzDynChain& a, hipStream_t st) {
  const int lds = 2 * 16 * RT * a.ld * (int)sizeof(float);
  auto kernel = BWD ? mz_dyn_unroll_bwd_kernel<RT> : mz_dyn_unroll_fwd_kernel<RT>;
  static PerDeviceOnce attr_once;
  attr_once.run([kernel] {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                              2 * 16 * RT * (kMzDynMaxWidth + 4) * (int)sizeof(float));
    (void)hipGetLastError();
  });
  hipLaunchKernelGGL(kernel, dim3((unsigned)((a.B + 16 * RT - 1) / (16 * RT))), dim3(kMzDynWaves * 64), lds, st, a);
  XT_LAUNCH_CHECK();
  return 0;
}

// rows = 16 or 32 batch rows per workgroup
template <bool BWD>
static int launch_mz_dyn(MzDynChain a, int rows, hipStream_t st) {
  XT_REQUIRE(a.nl >= 2 && a.nl <= kMzDynMaxLayers && a.U >= 1 && a.B >= 1 && (rows == 16 || rows == 32), "mz dyn unroll: bad arguments");
  int widest = a.H;
  for (int p = 0; p < a.nl; ++p) {
    XT_REQUIRE(a.w[p] && a.out[p] && a.K[p] >= 16 && a.K[p] % 16 == 0 && a.N[p] >= 16 && a.N[p] % 16 == 0 &&
               a.K[p] <= kMzDynMaxWidth && a.N[p] <= kMzDynMaxWidth && (BWD ? a.mask[p] != nullptr : a.bias[p] != nullptr),
               "mz dyn unroll: layer %d is %d -> %d (multiples of 16 up to %d)", p, a.K[p], a.N[p], kMzDynMaxWidth);
    XT_REQUIRE(a.K[p] == (p == 0 ? a.H : a.N[p - 1]), "mz dyn unroll: layer %d reads %d columns, its producer writes %d", p, a.K[p],
               p == 0 ? a.H : a.N[p - 1]);
    if (a.N[p] > widest) widest = a.N[p];
  }
  XT_REQUIRE(a.N[a.nl - 1] == a.H && a.x0 && (BWD ? (a.g0 && a.d0) : (a.actions && a.a_stride >= a.U)), "mz dyn unroll: bad arguments");
  a.ld = widest + 4;
  return rows == 16 ? launch_mz_dyn_rt<1, BWD>(a, st) : launch_mz_dyn_rt<2, BWD>(a, st);
}

}  // namespace
}  // namespace xt
