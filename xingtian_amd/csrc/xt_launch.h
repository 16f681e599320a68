// Host launchers and planners that are called across translation units, declared once (with their default arguments).
// Included by the file that defines each of them and by the files that call it.
#pragma once
#include "xt_common.h"
#include "xt_igemm.h"
#include "xt_heads_dev.h"

namespace xt {

struct DDgradArgs;      // xt_direct_dev.h

// ------------------------------------------------------------------ xt_igemm.hip: trunk layers
// deferred_ksplit (may be null): the split-K partials are left for the caller to sum and *deferred_ksplit says how many
int launch_fwd(const xt_conv_geom* cg, const xt_input_xform* xf, int B, const void* in, const int32_t* idx,
               const float* w, const float* bias, float* y, float* partial, int ksplit, hipStream_t st,
               int* deferred_ksplit = nullptr, uint32_t* relu_mask = nullptr, int* mask_written = nullptr);
int launch_wgrad(const xt_conv_geom* cg, const xt_input_xform* xf, int B, const void* in, const int32_t* idx,
                 const float* dy, float* dwb, float* slabs, int msplit, hipStream_t st, int reduce_now = 1,
                 int* msplit_out = nullptr, int slab_cap = 0);
int launch_dgrad(const xt_conv_geom* cg, int B, const float* dy, const float* w, const float* x, int act_prev,
                 float* dx, hipStream_t st);

// The producer's weight gradient offered to a fused backward launch (tuning.bwd_fuse21): the producer is a uint8 first
// layer, which has no input gradient, so the launch's input-gradient blocks may keep dX and write the producer's
// weight-gradient slabs instead (xt_igemm.hip: Fuse21Args).  *fused_out tells whether the launch did.
struct Fuse21Call {
  const xt_conv_geom* g0 = nullptr;    // the producer (first layer)
  const xt_input_xform* xf = nullptr;
  const void* in = nullptr;            // its uint8 input
  const int32_t* idx = nullptr;        // minibatch row gather (may be null)
  float* dwb = nullptr;                // its weight + bias gradient, when a single slab is written
  float* slabs = nullptr;              // ... else `*nslab_out` slabs
  int slab_cap = 0;
  int* nslab_out = nullptr;
  int* fused_out = nullptr;
};

// One fused backward launch of a non-first layer: weight gradient + input gradient (+ the head weight gradients).
struct BwdLayerCall {
  const xt_conv_geom* g = nullptr;
  int B = 0;
  const float* x = nullptr;            // the layer's input = its producer's output [B,H,W,C]
  const float* x_grad = nullptr;       // what the input gradient's activation-derivative epilogue reads: the producer's
                                       // PRE-activation when its activation is not monotonic (act_needs_preact); null = x
  const float* dy = nullptr;           // d(pre-activation) of this layer
  const float* w = nullptr;
  int act_prev = 0;                    // the producer's activation
  const uint32_t* xmask = nullptr;     // the producer's relu sign mask (may be null)
  float* dx = nullptr;                 // d(pre-activation) of the producer
  float* dwb = nullptr;                // the weight + bias gradient, when it is written as a single slab
  float* slabs = nullptr;              // ... else `*nslab_out` slabs for the caller to sum (may be null: msplit 1)
  int slab_cap = 0;                    // slabs that `slabs` can hold
  int msplit = 1;                      // requested weight-gradient split (the launch may lower it)
  const HeadWgArgs* hw = nullptr;      // head weight-gradient blocks riding along (may be null)
  float* sq_partials = nullptr;        // with npre_out: where a single-slab weight gradient leaves squared-norm partials
  hipStream_t st = nullptr;
  int* nslab_out = nullptr;            // slabs written: 1 = the gradient is final in dwb
  int* npre_out = nullptr;             // squared-norm partials written (0: none)
  int* path_out = nullptr;             // the branch taken, as xt_layer_bwd reports it
  const Fuse21Call* f21 = nullptr;     // the producer's weight gradient may ride along (may be null)
};
int launch_bwd_layer(const BwdLayerCall& c);
// xt_bwd_dense_lean_set: 1 (default) = the Dense instance of that launch in its table-free form (same bits), 0 = as before
int bwd_dense_lean();

// ------------------------------------------------------------------ xt_direct.hip: register-direct family (< 0: not taken)
int launch_fwd_direct(const xt_conv_geom* cg, const xt_input_xform* xf, int B, const void* in, const int32_t* idx,
                      const float* w, const float* bias, float* y, float* partial, int ksplit_max, hipStream_t st,
                      int* ksplit_out);
int launch_dgrad_direct(const xt_conv_geom* cg, int B, const float* dy, const float* w, const float* x, int act_prev,
                        float* dx, hipStream_t st);
bool plan_dgrad_direct_fused(const xt_tuning& t, const Geom& g, DDgradArgs* a, int* nblocks);

// ------------------------------------------------------------------ xt_conv1.hip: uint8 first layers (< 0: not taken)
int launch_conv1_fwd_bf16x3(const xt_conv_geom* g, const xt_input_xform* xf, int B, const void* in, const int32_t* idx,
                            const float* w, const float* bias, float* y, hipStream_t st, uint32_t* relu_mask,
                            int* mask_written);
int launch_conv1_wgrad_bf16x3(const xt_conv_geom* g, const xt_input_xform* xf, int B, const void* in,
                              const int32_t* idx, const float* dy, float* dwb, float* slabs, int max_slabs,
                              int* msplit_out, hipStream_t st);
int launch_conv1_same_fwd(const xt_conv_geom* g, const xt_input_xform* xf, int B, const void* in, const int32_t* idx,
                          const float* w, const float* bias, float* y, hipStream_t st);
int launch_conv1_same_wgrad(const xt_conv_geom* g, const xt_input_xform* xf, int B, const void* in, const int32_t* idx,
                            const float* dy, float* dwb, float* slabs, int max_slabs, int* msplit_out, hipStream_t st);
int launch_conv12_same_fwd(const xt_conv_geom* g, const xt_input_xform* xf, const xt_conv_geom* g2, int B,
                           const void* in, const int32_t* idx, const float* w, const float* bias, float* y,
                           const float* w2, const float* b2, float* y2, hipStream_t st);
// PpoCnn's conv1 -> conv2 (8x8/4 -> 4x4/2, VALID) in one launch over row-aligned flat tiles, every output bit what the two
// launches write (conv12_u8_valid_fwd_flat_kernel).  rows_per_block: 0 = the automatic split (<= 12 rows each, one block
// per CU while that holds).
bool conv12_valid_envelope(const xt_conv_geom* g, const xt_input_xform* xf, const xt_conv_geom* g2, int B,
                           int rows_per_block);
int launch_conv12_valid_fwd(const xt_conv_geom* g, const xt_input_xform* xf, const xt_conv_geom* g2, int B,
                            const void* in, const int32_t* idx, const float* w, const float* bias, float* y,
                            uint32_t* relu_mask, const float* w2, const float* b2, float* y2, int rows_per_block,
                            hipStream_t st, int* mask_written);
// PpoCnn's conv1 -> conv2 -> conv3 (3x3/1 VALID 32 -> 64 behind the pair above) in one launch, blocks owning runs of whole
// conv3 rows (conv123_u8_valid_fwd_flat_kernel); every output bit what the conv12 launch followed by conv3's own writes.
// rows_per_block: 0 = the automatic split.  in_net: the envelope in which the network takes it (neither conv2's nor
// conv3's own forward split over K, one block per CU at the most).  plan (may be null): the split and its LDS layout.
struct C123Plan { int G, N, nblk, cap, maxpos, maxn2, nps, nps3, tab_off, lds; };
bool conv123_valid_envelope(const xt_conv_geom* g, const xt_input_xform* xf, const xt_conv_geom* g2, const xt_conv_geom* g3,
                            int B, int rows_per_block, bool in_net, C123Plan* plan);
int launch_conv123_valid_fwd(const xt_conv_geom* g, const xt_input_xform* xf, const xt_conv_geom* g2, const xt_conv_geom* g3,
                             int B, const void* in, const int32_t* idx, const float* w, const float* bias, float* y,
                             uint32_t* relu_mask, const float* w2, const float* b2, float* y2, const float* w3,
                             const float* b3, float* y3, int rows_per_block, bool in_net, hipStream_t st, int* mask_written);

// ------------------------------------------------------------------ xt_heads.hip: heads and losses
int launch_act_apply(const float* z, float* y, long long count, int act, hipStream_t st);
int launch_ppo_heads_fused(const PpoHeadArgs& a, hipStream_t st);
int launch_ppo_gauss_heads_fused(const PpoGaussHeadArgs& a, hipStream_t st);
int launch_impala_heads_fwd(const ImpalaHeadArgs& a, hipStream_t st);
int launch_impala_vtrace_bwd(const ImpalaLossArgs& a, int n_traj, hipStream_t st);
int launch_impala_loss_reduce(const float* traj_loss, int n, float* out, float* acc, hipStream_t st,
                              const float* traj_stats = nullptr, double* stats = nullptr);
// xt_impala_loss with the optional trajectory rows / running sums of xt_net_set_impala_stats (both null: its two launches)
int launch_impala_loss(const float* logits, const float* baseline, const float* bp_logits, const int32_t* action,
                       const uint8_t* done, const float* reward, int n_traj, int T, int A, float gamma, float* dlogits,
                       float* dbaseline, float* out, float* acc, float* vs, float* pg_adv, float* traj_stats, double* stats,
                       hipStream_t st);
int launch_ppo_loss_gauss(const float* mean, const float* log_std, const float* value, int B, int A, const int32_t* idx,
                          const float* action, const float* old_logp, const double* adv, const float* old_v,
                          const double* target_v, float clip_ratio, float ent_coef, float vf_clip, float critic_coef,
                          float inv_b, float* dmean, float* dvalue, float* dls_rows, int ldls, float* terms,
                          hipStream_t st, float* rows = nullptr);
// xt_ppo_loss with the optional diagnostic rows of xt_net_set_train_stats (LossArgs::rows; null: the kernel of xt_ppo_loss)
int launch_ppo_loss(const float* logits, const float* value, int B, int A, const int32_t* idx, const int32_t* action,
                    const float* old_logp, const double* adv, const float* old_v, const double* target_v,
                    float clip_ratio, float ent_coef, float vf_clip, float critic_coef, float inv_b, float* dlogits,
                    float* dvalue, float* terms, float* rows, hipStream_t st);
// The acting heads (act_heads_kernel): heads forward + sampled action + its log-probability, one launch behind the trunk.
struct ActHeadArgs {
  const float *f_pi = nullptr, *f_v = nullptr;
  int B = 0, F = 0, A = 0;
  const float *wpi = nullptr, *bpi = nullptr, *wv = nullptr, *bv = nullptr;
  const float* log_std = nullptr;      // pi_logstd [A]: DiagGaussian; null: Categorical
  const float* noise = nullptr;        // injected noise [B,A] (Gumbel / standard normal), null: drawn from the generator
  uint32_t seed_lo = 0, seed_hi = 0, call_lo = 0, call_hi = 0;   // Philox key / counter words 2, 3
  long long row0 = 0;                  // global row of sample 0 (counter word 0 = row0 + b)
  float *ws_logits = nullptr, *ws_value = nullptr;               // the workspace copies ([B,A], [B])
  void* action = nullptr;              // int32 [B] | float32 [B,A]
  float* logp = nullptr;               // [B]
  float *value = nullptr, *logits = nullptr, *noise_out = nullptr;   // [B], [B,A], [B,A]; each may be null
};
int launch_act_heads(const ActHeadArgs& a, hipStream_t st);
int launch_heads_dfeat(const float* f_pi, const float* f_v, int B, int F, int A, const float* wpi, const float* wv,
                       const float* dlogits, const float* dvalue, int act_prev, float* df_pi, float* df_v,
                       hipStream_t st);
int launch_heads_fwd_wide(const float* feat, int B, int F, int A, const float* wpi, const float* bpi, const float* wv,
                          const float* bv, float* logits, float* value, hipStream_t st);
int launch_heads_dfeat_dist(const float* f_pi, int B, int F, int A, int N, const float* wpi, const float* wv,
                            const float* dlogits, const float* dvalue, const int32_t* slots, const int32_t* action,
                            int act_prev, float* df_pi, hipStream_t st);
// (A: the folded row's width (actions + 1) * N)
int launch_heads_dfeat_duel(const float* f_pi, int B, int F, int A, int N, const float* wpi, const float* dlogits,
                            const int32_t* slots, const int32_t* action, int act_prev, float* df_pi, hipStream_t st);
int launch_heads_wgrad_partial(const float* f_pi, const float* f_v, int B, int F, int A, const float* dlogits,
                               const float* dvalue, float* slab_pi, long long stride_pi, float* slab_v,
                               long long stride_v, int* nchunk_out, hipStream_t st);

// ------------------------------------------------------------------ xt_optim.hip: gradient reduction, norm, optimisers
int launch_global_norm(const float* grad, long long count, float clip_norm, float grad_scale, float lr, float beta1,
                       float beta2, int advance, float* state, float* scratch, hipStream_t st,
                       const float* lr_dev = nullptr, int* nblocks_out = nullptr);
int launch_sqnorm_partial(const float* grad, long long count, float* scratch, int* nblocks_out, hipStream_t st);
int launch_norm_finalize(const float* partial, int nblocks, float clip_norm, float grad_scale, float lr, float beta1,
                         float beta2, int advance, float* state, const LossArgs* la, hipStream_t st,
                         const float* lr_dev = nullptr);
int launch_grads_finish(GradTable* tab, float* partial, int max_partials, int* nblocks_out, const FinalizeArgs* fin,
                        hipStream_t st, unsigned select = 0, unsigned early = 0, const DpFinish* dpf = nullptr);
// the host half of launch_grads_finish (no device call): the table the kernel gets, the partial slots, the grid
struct GradsFinishPlan {
  GradTable sub;
  int npartials, grid;
};
int plan_grads_finish(GradTable* tab, int max_partials, int enable, bool has_counter, bool scatter, unsigned select,
                      unsigned early, GradsFinishPlan* plan);
int grads_finish_resident_blocks(bool stats = false);
int grads_finish_fused_grid(const GradTable* tab);
int grads_finish_fused_form(const GradTable* tab, bool stats);
int launch_adam(float* param, const float* grad, float* m, float* v, long long count, float beta1, float beta2,
                float eps, const float* state, hipStream_t st);
int launch_adam_clip(float* param, const float* grad, float* m, float* v, long long count, float beta1, float beta2,
                     float eps, float* state, const float* partial, int nblocks, float clip_norm, float grad_scale,
                     hipStream_t st, const DpStep* dp = nullptr, int block_cap = 0, const IoFold* io = nullptr,
                     double* stats = nullptr);
// xt_net_set_train_stats: the row / loss shares of a gradient-only step into the running sums; the sums cleared
int launch_train_stats_reduce(const LossArgs* la, hipStream_t st);
int launch_train_stats_clear(double* stats, hipStream_t st);
int launch_rmsprop_clip(float* param, const float* grad, float* mg, float* ms, long long count, float lr, float decay,
                        float eps, float* state, const float* partial, int nblocks, float clip_norm, float grad_scale,
                        hipStream_t st, const float* lr_dev = nullptr, const DpStep* dp = nullptr, int block_cap = 0,
                        double* stats = nullptr);
int launch_dp_tail_write(float* tail, int rank, float rows, const float* loss, float* state, float lr,
                         const float* lr_dev, float beta1, float beta2, int advance, hipStream_t st);
int launch_dp_tail_consume(const DpStep* dp, hipStream_t st);
int launch_dp_reduce_wait(const DpStep* dp, hipStream_t st);

// ------------------------------------------------------------------ xt_xgmi.hip: the direct exchange fused into the step
int direct_fill_finish(xt_direct_comm* c, int64_t count, DpFinish* f);
int direct_launch_scatter(xt_direct_comm* c, const float* buf, int64_t count, hipStream_t st);
int direct_fill_step(xt_direct_comm* c, int64_t count, int64_t count_grad, DpStep* s, const float** result,
                     const float** partial, int* npartial, int* block_cap);

}  // namespace xt
