// Noisy layers (NoisyNet, Fortunato et al. 2018, factorised Gaussian) beside the net: include/xt_mi355x.h, "noisy layers".
// A noisy Dense layer is an ordinary Dense layer on W_eff = mu + sigma * (f_in f_out^T), so the layer kernels stay as
// they are: one pass writes the effective parameters of the whole net in front of the step (noisy_compose_kernel), one
// forms the sigma gradients behind it (noisy_grads_kernel).  Both are elementwise over 16-byte vectors and memory-bound.
#include "xt_common.h"

namespace xt {

constexpr int kNoisyTile = 1024;          // floats of [0, n_net) a workgroup handles at a time: one 16-byte vector per thread

struct NoisyTable {
  int n;
  xt_noisy_layer l[XT_NOISY_MAX_LAYERS];
};
struct NoisyKey { uint32_t k0, k1, call, stream_id; };

static inline int64_t noisy_len(const xt_noisy_layer& L) { return ((int64_t)L.K + 1) * L.N; }
__host__ __device__ static inline int noisy_out_off(int K) { return (K + 3) & ~3; }

// Element i of vector `side` (0: f_in, 1: f_out) of a layer: out of line so that every caller runs the one body -- the
// values a workgroup recomputes are bit for bit the values another stored in `noise`.
__device__ __noinline__ static float noisy_f(const NoisyKey key, int index, int side, int i) {
  const Philox4 r = philox4x32_10((uint32_t)i >> 1, (uint32_t)(2 * index + side), key.call, key.stream_id, key.k0, key.k1);
  const float u1 = philox_uniform((i & 1) ? r.z : r.x), u2 = philox_uniform((i & 1) ? r.w : r.y);
  const float x = sqrtf(-2.f * logf(u1)) * cosf(6.283185307179586f * u2);
  return copysignf(sqrtf(fabsf(x)), x);
}

// Tiles of kNoisyTile floats, grid-strided.  A thread owns one float4 of the tile: it is store's, except where it lies in a
// layer's mean block.  For every layer the tile meets, the workgroup first forms the f_in of the rows and the f_out of the
// columns the tile covers in LDS -- at most kNoisyTile + 1 rows (N = 1) and kNoisyTile columns (all N of them when the
// tile spans a whole row, else the span's own, indexed by position) -- then every thread patches its elements.  The bias
// is row K with f_in = 1 (1 * f_out is exact).  The tile that holds the first element of row k stores f_in[k], the tile
// that holds bias element n stores f_out[n]: every vector element is stored exactly once per launch.
__global__ __launch_bounds__(256) void noisy_compose_kernel(const NoisyTable t, const float* __restrict__ store,
                                                            float* __restrict__ eff, const long long n_net,
                                                            float* __restrict__ noise, const float* __restrict__ noise_in,
                                                            const NoisyKey key, const int mean_only) {
  __shared__ float s_in[kNoisyTile + 4];
  __shared__ float s_out[kNoisyTile];
  const long long n_tiles = (n_net + kNoisyTile - 1) / kNoisyTile;
  for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const long long t0 = tile * kNoisyTile, t1 = t0 + kNoisyTile < n_net ? t0 + kNoisyTile : n_net;
    const long long e0 = t0 + 4 * (long long)threadIdx.x;
    const bool live = e0 < n_net;                       // (n_net is a multiple of 4: a vector is inside or outside)
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (live) v = *reinterpret_cast<const float4*>(store + e0);
    for (int l = 0; l < (mean_only ? 0 : t.n); ++l) {
      const xt_noisy_layer L = t.l[l];
      const long long len = ((long long)L.K + 1) * L.N;
      const long long lo = t0 > L.w_off ? t0 : L.w_off, hi = t1 < L.w_off + len ? t1 : L.w_off + len;
      if (lo >= hi) continue;                           // (the same in every thread of the workgroup)
      const int N = L.N, r0 = (int)(lo - L.w_off), r1 = (int)(hi - L.w_off), span = r1 - r0;
      const bool by_n = N <= span;
      const int krow0 = r0 / N, krows = (r1 - 1) / N - krow0 + 1;
      __syncthreads();                                  // the previous layer's (tile's) readers are done with the LDS
      for (int j = threadIdx.x; j < krows; j += 256) {
        const int k = krow0 + j;
        float f = 1.f;
        if (k < L.K) {
          f = noise_in ? noise_in[L.noise_off + k] : noisy_f(key, L.index, 0, k);
          if ((long long)k * N >= r0) noise[L.noise_off + k] = f;
        }
        s_in[j] = f;
      }
      for (int j = threadIdx.x; j < (by_n ? N : span); j += 256) {
        const int n = by_n ? j : (r0 + j) % N;
        const float f = noise_in ? noise_in[L.noise_off + noisy_out_off(L.K) + n] : noisy_f(key, L.index, 1, n);
        const long long brel = (long long)L.K * N + n;
        if (brel >= r0 && brel < r1) noise[L.noise_off + noisy_out_off(L.K) + n] = f;
        s_out[j] = f;
      }
      __syncthreads();
      const long long rel0 = e0 - L.w_off;              // a multiple of 4: the vector starts inside the block or not at all
      if (live && rel0 >= 0 && rel0 < len) {
        const float* sg = store + L.sigma_off + rel0;
        float s[4], m[4] = {v.x, v.y, v.z, v.w};
        const int left = len - rel0 < 4 ? (int)(len - rel0) : 4;
        if (left == 4) {
          const float4 q = *reinterpret_cast<const float4*>(sg);
          s[0] = q.x; s[1] = q.y; s[2] = q.z; s[3] = q.w;
        } else {
          for (int c = 0; c < 4; ++c) s[c] = c < left ? sg[c] : 0.f;
        }
        int k = (int)rel0 / N, n = (int)rel0 - k * N;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          if (c < left) {
            const float e = s_in[k - krow0] * s_out[by_n ? n : (int)rel0 + c - r0];
            const float p = s[c] * e;
            m[c] = m[c] + p;
          }
          if (++n == N) { n = 0; ++k; }
        }
        v = make_float4(m[0], m[1], m[2], m[3]);
      }
    }
    if (live) *reinterpret_cast<float4*>(eff + e0) = v;
  }
}

// grads[sigma block] = grads[mean block] * e, one float4 per thread, the layers one after the other
__global__ __launch_bounds__(256) void noisy_grads_kernel(const NoisyTable t, const float* __restrict__ noise, float* grads) {
  for (int l = 0; l < t.n; ++l) {
    const xt_noisy_layer L = t.l[l];
    const long long len = ((long long)L.K + 1) * L.N;
    const float* f_in = noise + L.noise_off;
    const float* f_out = f_in + noisy_out_off(L.K);
    const int N = L.N;
    for (long long rel0 = 4 * ((long long)blockIdx.x * 256 + threadIdx.x); rel0 < len; rel0 += 4ll * 256 * gridDim.x) {
      const float* g = grads + L.w_off + rel0;
      float* gs = grads + L.sigma_off + rel0;
      const int left = len - rel0 < 4 ? (int)(len - rel0) : 4;
      float d[4];
      if (left == 4) {
        const float4 q = *reinterpret_cast<const float4*>(g);
        d[0] = q.x; d[1] = q.y; d[2] = q.z; d[3] = q.w;
      } else {
        for (int c = 0; c < 4; ++c) d[c] = c < left ? g[c] : 0.f;
      }
      int k = (int)(rel0 / N), n = (int)(rel0 - (long long)k * N);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        if (c < left) {
          const float e = (k < L.K ? f_in[k] : 1.f) * f_out[n];
          d[c] = d[c] * e;
        }
        if (++n == N) { n = 0; ++k; }
      }
      if (left == 4) {
        *reinterpret_cast<float4*>(gs) = make_float4(d[0], d[1], d[2], d[3]);
      } else {
        for (int c = 0; c < left; ++c) gs[c] = d[c];
      }
    }
  }
}

static inline bool ranges_overlap(int64_t a0, int64_t a1, int64_t b0, int64_t b1) { return a0 < b1 && b0 < a1; }

// what both entries refuse of a table; -> 0 or XT_REQUIRE's code
static int noisy_check_table(const char* who, const xt_noisy_layer* layers, int32_t n_layers) {
  XT_REQUIRE(layers, "%s: null layer table", who);
  XT_REQUIRE(n_layers >= 1 && n_layers <= XT_NOISY_MAX_LAYERS, "%s: n_layers = %d outside [1, %d]", who, n_layers,
             XT_NOISY_MAX_LAYERS);
  for (int i = 0; i < n_layers; ++i) {
    const xt_noisy_layer& L = layers[i];
    XT_REQUIRE(L.K >= 1 && L.N >= 1 && noisy_len(L) < (1ll << 31), "%s: layer %d: K = %d, N = %d (each must be at least 1 "
               "and (K + 1) * N below 2^31)", who, i, L.K, L.N);
    XT_REQUIRE(L.w_off >= 0 && L.sigma_off >= 0 && L.noise_off >= 0 && ((L.w_off | L.sigma_off | L.noise_off) & 3) == 0,
               "%s: layer %d: offsets w_off = %lld, sigma_off = %lld, noise_off = %lld must be non-negative multiples of 4",
               who, i, (long long)L.w_off, (long long)L.sigma_off, (long long)L.noise_off);
    XT_REQUIRE(L.index >= 0 && L.index < (1 << 30), "%s: layer %d: index = %d is negative", who, i, L.index);
    const int64_t nz = noisy_out_off(L.K) + L.N;
    for (int j = 0; j < i; ++j) {
      const xt_noisy_layer& M = layers[j];
      XT_REQUIRE(!ranges_overlap(L.w_off, L.w_off + noisy_len(L), M.w_off, M.w_off + noisy_len(M)),
                 "%s: the mean blocks of layers %d and %d overlap ([%lld, %lld) and [%lld, %lld))", who, j, i,
                 (long long)M.w_off, (long long)(M.w_off + noisy_len(M)), (long long)L.w_off,
                 (long long)(L.w_off + noisy_len(L)));
      XT_REQUIRE(!ranges_overlap(L.sigma_off, L.sigma_off + noisy_len(L), M.sigma_off, M.sigma_off + noisy_len(M)),
                 "%s: the sigma blocks of layers %d and %d overlap ([%lld, %lld) and [%lld, %lld))", who, j, i,
                 (long long)M.sigma_off, (long long)(M.sigma_off + noisy_len(M)), (long long)L.sigma_off,
                 (long long)(L.sigma_off + noisy_len(L)));
      XT_REQUIRE(!ranges_overlap(L.noise_off, L.noise_off + nz, M.noise_off, M.noise_off + noisy_out_off(M.K) + M.N),
                 "%s: the noise vectors of layers %d and %d overlap (noise_off %lld and %lld)", who, j, i,
                 (long long)M.noise_off, (long long)L.noise_off);
    }
  }
  return 0;
}

static NoisyTable noisy_table(const xt_noisy_layer* layers, int32_t n_layers) {
  NoisyTable t;
  t.n = n_layers;
  for (int i = 0; i < XT_NOISY_MAX_LAYERS; ++i) t.l[i] = layers[i < n_layers ? i : 0];
  return t;
}

}  // namespace xt

extern "C" {

int xt_noisy_compose(const xt_noisy_layer* layers, int32_t n_layers, const float* store, float* params_eff, int64_t n_net,
                     float* noise, const float* noise_in, uint64_t seed, uint64_t call, int32_t stream_id,
                     int32_t mean_only, void* stream) {
  XT_REQUIRE(store && params_eff && (noise || mean_only), "xt_noisy_compose: null buffer");
  XT_REQUIRE(store != params_eff && (((uintptr_t)store | (uintptr_t)params_eff) & 15) == 0,
             "xt_noisy_compose: store and params_eff must be two 16-byte aligned buffers");
  XT_REQUIRE(n_net > 0 && n_net % 4 == 0, "xt_noisy_compose: n_net = %lld is not a positive multiple of 4", (long long)n_net);
  XT_REQUIRE(stream_id >= 0, "xt_noisy_compose: stream_id = %d is negative", stream_id);
  if (int rc = xt::noisy_check_table("xt_noisy_compose", layers, n_layers)) return rc;
  for (int i = 0; i < n_layers; ++i) {
    const xt_noisy_layer& L = layers[i];
    XT_REQUIRE(L.w_off + xt::noisy_len(L) <= n_net, "xt_noisy_compose: layer %d: the mean block [%lld, %lld) leaves [0, %lld)",
               i, (long long)L.w_off, (long long)(L.w_off + xt::noisy_len(L)), (long long)n_net);
    XT_REQUIRE(L.sigma_off >= n_net, "xt_noisy_compose: layer %d: the sigma block at %lld lies in front of n_net = %lld", i,
               (long long)L.sigma_off, (long long)n_net);
  }
  const long long n_tiles = (n_net + xt::kNoisyTile - 1) / xt::kNoisyTile;
  const xt::NoisyKey key = {(uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)call, (uint32_t)stream_id};
  hipLaunchKernelGGL(xt::noisy_compose_kernel, dim3((unsigned)(n_tiles < 1024 ? n_tiles : 1024)), dim3(256), 0,
                     xt::as_stream(stream), xt::noisy_table(layers, n_layers), store, params_eff, (long long)n_net, noise,
                     noise_in, key, mean_only ? 1 : 0);
  XT_LAUNCH_CHECK();
  return 0;
}

int xt_noisy_grads(const xt_noisy_layer* layers, int32_t n_layers, const float* noise, float* grads, void* stream) {
  XT_REQUIRE(noise && grads && ((uintptr_t)grads & 15) == 0, "xt_noisy_grads: null buffer, or grads not 16-byte aligned");
  if (int rc = xt::noisy_check_table("xt_noisy_grads", layers, n_layers)) return rc;
  int64_t mean_end = 0, longest = 0;
  for (int i = 0; i < n_layers; ++i) {
    const int64_t end = layers[i].w_off + xt::noisy_len(layers[i]);
    mean_end = end > mean_end ? end : mean_end;
    longest = xt::noisy_len(layers[i]) > longest ? xt::noisy_len(layers[i]) : longest;
  }
  for (int i = 0; i < n_layers; ++i)
    XT_REQUIRE(layers[i].sigma_off >= mean_end, "xt_noisy_grads: layer %d: the sigma block at %lld lies in front of the end "
               "of the mean blocks (%lld)", i, (long long)layers[i].sigma_off, (long long)mean_end);
  const long long blocks = (longest + 1023) / 1024;
  hipLaunchKernelGGL(xt::noisy_grads_kernel, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(256), 0,
                     xt::as_stream(stream), xt::noisy_table(layers, n_layers), noise, grads);
  XT_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
