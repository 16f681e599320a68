// Prioritised replay on the device (xt/algorithm/prioritized_replay_buffer_muzero.py::PrioritizedReplayBuffer on
// xt/algorithm/segment_tree.py): a sum tree and a min tree of 2 * cap2 float64 nodes each in HBM, node i = op(node 2i,
// node 2i + 1), leaf cap2 + slot = ring slot `slot`.  Every kernel here is ONE workgroup walking the levels with a
// barrier between them: the whole read-modify-write stays inside one CU, stream order does the rest.  They are latency
// chains of <= 31 dependent levels; bandwidth is irrelevant.  A node is a pure function of the final leaves, so the
// trees are bit for bit what the reference's sequential __setitem__ calls leave, whatever order the threads run in.
#include "xt_common.h"

namespace xt {

// (cap2 is a power of two: its level count)
__device__ __forceinline__ int per_levels(long long cap2) { return 63 - __clzll(cap2); }

__device__ __forceinline__ void per_node(double* sum, double* mn, long long i) {
  sum[i] = sum[2 * i] + sum[2 * i + 1];
  const double l = mn[2 * i], r = mn[2 * i + 1];
  mn[i] = r < l ? r : l;                               // Python's min(l, r): r only if r < l
}

// leaves [first, first + count) <- max_prio ** alpha, then their ancestors level by level (256 threads stride over each
// level's node range)
__global__ __launch_bounds__(256) void per_add_kernel(double* sum, double* mn, long long cap2,
                                                      const double* __restrict__ max_prio, long long first,
                                                      long long count, double alpha) {
  const double leaf = pow(*max_prio, alpha);
  for (long long i = threadIdx.x; i < count; i += 256) {
    sum[cap2 + first + i] = leaf;
    mn[cap2 + first + i] = leaf;
  }
  long long lo = cap2 + first, hi = cap2 + first + count - 1;
  while (lo > 1) {
    __syncthreads();
    lo >>= 1; hi >>= 1;
    for (long long i = lo + threadIdx.x; i <= hi; i += 256) per_node(sum, mn, i);
  }
}

// One thread per sample.  Every thread forms p_total itself (the same <= 31 loads in every lane).
__global__ __launch_bounds__(1024) void per_sample_kernel(const double* __restrict__ sum, const double* __restrict__ mn,
                                                          long long cap2, long long size, const double* __restrict__ u,
                                                          int B, double beta, int32_t* __restrict__ slots_out,
                                                          double* __restrict__ weights_out) {
  const int b = threadIdx.x;
  if (b >= B) return;
  // p_total = reduce over leaves [0, size - 2]: v[L1] + (v[L2] + (... + v[Lk])) over the maximal left subtrees on the
  // way down to leaf size - 2, folded from the innermost term outwards
  long long node = cap2 + size - 2;
  while ((node & 1) && node > 1) node >>= 1;           // the highest node whose range ends at that leaf
  double p_total = sum[node];
  for (; node > 1; node >>= 1)
    if (node & 1) p_total = sum[node - 1] + p_total;
  const double every = p_total / (double)B;
  double mass = u[b] * every + (double)b * every;      // (no contraction: the library is built with -ffp-contract=off)
  long long idx = 1;
  while (idx < cap2) {
    const double left = sum[2 * idx];
    if (left > mass) {
      idx = 2 * idx;
    } else {
      mass -= left;
      idx = 2 * idx + 1;
    }
  }
  idx -= cap2;
  if (idx > size - 1) idx = size - 1;                  // (the reference raises an IndexError there)
  const double total = sum[1], n = (double)size;
  double p_min = mn[1] / total;
  p_min = p_min > 1e-5 ? p_min : 1e-5;
  const double max_w = pow(p_min * n, -beta);
  slots_out[b] = (int32_t)idx;
  weights_out[b] = pow(sum[cap2 + idx] / total * n, -beta) / max_w;
}

// One thread per sample: priority_b = |delta_b| + eps, leaf = priority_b ** alpha (of equal slots the largest b wins),
// max_prio = max(max_prio, every priority_b), then the ancestors level by level.
__global__ __launch_bounds__(1024) void per_update_kernel(double* sum, double* mn, long long cap2,
                                                          double* __restrict__ max_prio,
                                                          const int32_t* __restrict__ slots,
                                                          const float* __restrict__ delta, long long delta_stride, int B,
                                                          double eps, double alpha) {
  __shared__ int32_t s_slot[1024];
  __shared__ double s_max[1024];
  const int b = threadIdx.x;
  int32_t slot = -1;
  double prio = 0.0;
  if (b < B) {
    slot = slots[b];
    if (slot < 0 || slot >= cap2) slot = -1;           // (never stored through)
    prio = (double)fabsf(delta[b * delta_stride]) + eps;
  }
  s_slot[b] = slot;
  s_max[b] = prio;
  __syncthreads();
  bool wins = slot >= 0;
  for (int j = b + 1; j < B && wins; ++j) wins = s_slot[j] != slot;
  for (int o = 512; o > 0; o >>= 1) {
    if (b < o && b + o < (int)blockDim.x) s_max[b] = s_max[b] > s_max[b + o] ? s_max[b] : s_max[b + o];
    __syncthreads();
  }
  if (b == 0) {
    const double m = *max_prio;
    *max_prio = m > s_max[0] ? m : s_max[0];
  }
  if (wins) {
    const double leaf = pow(prio, alpha);
    sum[cap2 + slot] = leaf;
    mn[cap2 + slot] = leaf;
  }
  long long node = slot >= 0 ? cap2 + slot : 0;
  for (int level = per_levels(cap2); level > 0; --level) {
    __syncthreads();
    node >>= 1;
    if (node >= 1) per_node(sum, mn, node);            // (threads that share an ancestor store the same value)
  }
}

static inline bool is_pow2(int64_t x) { return x > 0 && (x & (x - 1)) == 0; }

}  // namespace xt

extern "C" {

int xt_per_add(double* sum, double* min, int64_t cap2, const double* max_prio, int64_t first, int64_t count, double alpha,
               void* stream) {
  XT_REQUIRE(sum && min && max_prio, "xt_per_add: null argument");
  XT_REQUIRE(xt::is_pow2(cap2) && cap2 <= (1ll << 31), "xt_per_add: cap2 = %lld is not a power of two <= 2^31",
             (long long)cap2);
  XT_REQUIRE(first >= 0 && count > 0 && first <= cap2 - count, "xt_per_add: leaves [%lld, %lld + %lld) outside [0, %lld)",
             (long long)first, (long long)first, (long long)count, (long long)cap2);
  XT_REQUIRE(alpha >= 0.0, "xt_per_add: alpha = %g is negative", alpha);
  hipLaunchKernelGGL(xt::per_add_kernel, dim3(1), dim3(256), 0, xt::as_stream(stream), sum, min, (long long)cap2, max_prio,
                     (long long)first, (long long)count, alpha);
  XT_LAUNCH_CHECK();
  return 0;
}

int xt_per_sample(const double* sum, const double* min, int64_t cap2, int64_t size, const double* u, int32_t B, double beta,
                  int32_t* slots_out, double* weights_out, void* stream) {
  XT_REQUIRE(sum && min && u && slots_out && weights_out, "xt_per_sample: null argument");
  XT_REQUIRE(xt::is_pow2(cap2) && cap2 <= (1ll << 31), "xt_per_sample: cap2 = %lld is not a power of two <= 2^31",
             (long long)cap2);
  XT_REQUIRE(size >= 2 && size <= cap2,
             "xt_per_sample: size = %lld outside [2, %lld] (fewer than two stored transitions cannot be sampled)",
             (long long)size, (long long)cap2);
  XT_REQUIRE(B > 0 && B <= 1024, "xt_per_sample: B = %d outside (0, 1024] (one thread per sample, one workgroup)", B);
  XT_REQUIRE(beta > 0.0, "xt_per_sample: beta = %g is not positive", beta);
  hipLaunchKernelGGL(xt::per_sample_kernel, dim3(1), dim3((B + 63) / 64 * 64), 0, xt::as_stream(stream), sum, min,
                     (long long)cap2, (long long)size, u, B, beta, slots_out, weights_out);
  XT_LAUNCH_CHECK();
  return 0;
}

int xt_per_update(double* sum, double* min, int64_t cap2, double* max_prio, const int32_t* slots, const float* delta,
                  int64_t delta_stride, int32_t B, double eps, double alpha, void* stream) {
  XT_REQUIRE(sum && min && max_prio && slots && delta, "xt_per_update: null argument");
  XT_REQUIRE(xt::is_pow2(cap2) && cap2 <= (1ll << 31), "xt_per_update: cap2 = %lld is not a power of two <= 2^31",
             (long long)cap2);
  XT_REQUIRE(B > 0 && B <= 1024, "xt_per_update: B = %d outside (0, 1024] (one thread per sample, one workgroup)", B);
  XT_REQUIRE(delta_stride >= 1, "xt_per_update: delta_stride = %lld", (long long)delta_stride);
  XT_REQUIRE(eps > 0.0 && alpha >= 0.0, "xt_per_update: eps = %g must be positive, alpha = %g non-negative", eps, alpha);
  hipLaunchKernelGGL(xt::per_update_kernel, dim3(1), dim3((B + 63) / 64 * 64), 0, xt::as_stream(stream), sum, min,
                     (long long)cap2, max_prio, slots, delta, (long long)delta_stride, B, eps, alpha);
  XT_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
