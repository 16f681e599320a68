/*
 * xt_mi355x.h -- C ABI of the MI355X-native XingTian learner-update path.
 *
 * The reference (huawei-noah/xingtian) is 100 % Python and ships no native
 * interface: the learner arithmetic is TensorFlow graph ops called from
 * xt/model/ppo/ppo.py, xt/model/impala/impala_cnn_opt.py, xt/model/impala/vtrace.py
 * and numpy in xt/agent/ppo/ppo.py.  Each entry point below therefore cites the
 * reference *call site* whose arithmetic it replaces.  A reference maintainer binds
 * this library with ctypes (cffi is not installed in the target image); the stub is
 * shown in INTEGRATION.md.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless named host_*; the caller (PyTorch-ROCm
 *     tensors in our host code) owns all memory, nothing is allocated or freed here
 *     except inside an xt_net handle's own small descriptor tables;
 *   - `stream` is a hipStream_t passed as void* (0 = the null stream);
 *   - every function returns 0 on success, non-zero on error; xt_last_error() then
 *     returns a thread-local, NUL-terminated description;
 *   - layouts are TensorFlow's: activations NHWC, conv kernels HWIO [kh,kw,cin,cout],
 *     dense kernels [in,out]; a layer's kernel and bias are contiguous
 *     ([K*N] floats then [N] floats) inside one flat fp32 parameter buffer.
 */
#ifndef XT_MI355X_H_
#define XT_MI355X_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define XT_ABI_VERSION 12

#define XT_ACT_NONE 0
#define XT_ACT_RELU 1
#define XT_ACT_TANH 2
/* ABI >= 8: the other entries of ACTIVATION_MAP (xt/model/model_utils.py:8-20) */
#define XT_ACT_SIGMOID 3
#define XT_ACT_SOFTSIGN 4
#define XT_ACT_SOFTPLUS 5
#define XT_ACT_LEAKY_RELU 6      /* tf.nn.leaky_relu, alpha = 0.2 */
#define XT_ACT_ELU 7
#define XT_ACT_SELU 8
/* not monotonic: a network layer with one of these also keeps its PRE-activation (xt_net does; the stand-alone layer
 * entry points then take the pre-activation as `x` of xt_layer_dgrad) */
#define XT_ACT_SWISH 9           /* tf.nn.swish: x * sigmoid(x)                                   */
#define XT_ACT_GELU 10           /* xt/model/tf_utils.py:157-166 (tanh form)                      */

/* ------------------------------------------------------------------ misc */
int xt_abi_version(void);
const char* xt_last_error(void);
/* name of the gfx target the device code was compiled for ("gfx950") */
const char* xt_build_arch(void);
/* sha256 (16 hex digits) over the kernel sources this binary was compiled from, embedded at build time (ABI >= 9;
 * csrc/Makefile, -DXT_SRC_SHA): profile artefacts are tagged with it, so counters measured on another build of the
 * kernels -- or a stale prebuilt library next to newer sources -- are recognised (bench.py, tools/pmc_summary.py). */
const char* xt_build_sources_sha(void);

/* --------------------------------------------------------------- tuning */
/* Process-wide kernel-selection knobs (ABI >= 6).  The defaults (xt_tuning_get on a fresh process) are the forms
 * that measured fastest on MI355X for the BASELINE.json shapes; the alternatives are kept
 * for A/B measurements (tools/) and as fallbacks.  Set them BEFORE creating networks: captured hipGraphs and the
 * split counts cached in a net are not revisited.  Every form computes the same arithmetic up to fp32 summation
 * order; `bf16x6 = 0` / `conv1_bf16x3 = 0` select plain fp32 MFMA. */
typedef struct xt_tuning {
  int32_t bf16x6;             /* 1: conv input gradients as six bf16 MFMAs per 16-deep chunk (exact split)      */
  int32_t dgrad_all_classes;  /* 1: stride-2 VALID conv: all four parity classes of a position tile per block   */
  int32_t dgrad_tile64;       /* 1: stride-1 register-direct input gradient with 64-row tiles                   */
  int32_t dgrad_halo;         /* 1: ... with the dY halo of the tile staged in LDS                              */
  int32_t bwd_own_instance;   /* 1: halo input gradient in its own kernel instance (3 workgroups per CU)        */
  int32_t bwd_fit_slots;      /* co-resident workgroup slots a fused backward launch is cut to (0 = off)        */
  int32_t conv1_bf16x3;       /* 1: uint8 first layer on the bf16 matrix cores (exact three-way split)          */
  int32_t conv1_flat;         /* 1: first layer over the flattened position range (512-position workgroups)     */
  int32_t conv1_waves;        /* 8 | 4 waves per first-layer workgroup                                          */
  int32_t fwd_two_groups;     /* 1: two wave groups per forward block when the launch cannot fill the chip      */
  int32_t direct;             /* 1: register-direct kernels (xt_direct.hip) where they measured faster          */
  int32_t direct_fwd;         /* 1: ... for forwards                                                            */
  int32_t direct_dgrad;       /* 1: ... for input gradients                                                     */
  int32_t direct_all;         /* 1: ... for every shape inside their envelope (experiments)                     */
  int32_t direct_waves;       /* resident-wave target of a register-direct launch                               */
  int32_t direct_max_waves;   /* waves per register-direct workgroup (<= 8)                                     */
  int32_t direct_tile64_tiles;/* tile count from which the register-direct input gradient uses 64-row tiles     */
  int32_t fwd_split_target;   /* split-K forward: target block count                                            */
  int32_t wgrad_split_target; /* split-M weight gradient: target block count                                    */
  int32_t reduce_z_lanes;     /* gradient reduction: slab lanes per block (power of two <= 32)                  */
  int32_t defer_splitk;       /* 1: the fused head kernel finishes the last trunk layer's split-K partials      */
  int32_t finalize_ticket;    /* 1: last-block finalize of the norm instead of the clip factor inside Adam      */
  int32_t fwd_tiled_valid;    /* 1: un-padded fp32 layers with N <= 32 run the LDS-tiled bf16x6 forward instead
                                 of the register-direct fp32 one (ABI >= 7; PpoCnn conv2: -2 us per step)       */
  int32_t wgrad_rows;         /* fused backward of a 4x4/2 32->32 VALID conv (PpoCnn conv2), ABI >= 8:
                                 4 (default): two workgroups per CU (250 VGPRs) -- input gradient with all four taps'
                                   operands in flight, LDS-tiled im2col weight gradient with four register stages,
                                   the launch cut to 512 co-resident workgroups (20.5 vs 22.4 us per launch);
                                 0: the round-2 form (three workgroups per CU, one / two stages in flight);
                                 1 / 2: weight gradient from input ROWS staged in LDS (no im2col gather) with / without
                                   the deep input-gradient prefetch (measured slower: 24 us; kept for A/B)        */
  int32_t fwd_prefetch_all;   /* 0 (default): two reduction steps in flight.  1: bf16x6 forwards with <= 8 steps
                                 per wave group issue all operand loads up front (ABI >= 8; measured +0.1 ms)     */
  int32_t bwd_deep_prefetch;  /* 1: fused backward of Dense (1x1, stride 1) layers as a two-workgroups-per-CU instance:
                                 all (<= 8) reduction steps of the input gradient in flight, four register stages in
                                 the weight gradient, split cut to 512 co-resident workgroups (ABI >= 8)           */
  int32_t fwd_four_groups;    /* 1: bf16x6 forwards with <= one block per CU and >= 4 steps per group run FOUR 4-wave groups
                                 (a quarter of the reduction range each, one LDS stage) instead of two (ABI >= 8)  */
  int32_t reduce_deep_lanes;  /* gradient reduction: entries with at least this many slabs get up to 32 slab lanes per block
                                 (0 = off; default 128: the first layer's one-slab-per-workgroup gradients)         */
  int32_t fwd_xcd_chunk;      /* 1: LDS-tiled forwards with several N tiles / k splits give every XCD a contiguous
                                 run of the (m tile, n tile, k slice) order: tiles that share operand slices share
                                 an L2 (ABI >= 8)                                                                  */
  int32_t tail_overlap;       /* single-GPU update tail as graph branches (one-trunk nets with >= 2 layers; bit mask, ABI >= 8):
                                 1: the slab reduction of the last trunk layer + heads (95 % of PpoCnn's gradient bytes) runs on a
                                    side stream right after the first backward launch, under the conv backward;
                                 2: Adam is split into [first layer] on the compute stream and [everything else] on the side
                                    stream, which the NEXT step's first-layer forward overlaps (joined before layer 2)       */
  int32_t tail_fused;         /* 1: slab reduction + global norm + clip + Adam in ONE launch: the thread that reduced a group of
                                 elements also updates it, only the squared-norm partials and the step size cross a grid
                                 barrier (all workgroups resident, checked; Adam only; ABI >= 8)                          */
  int32_t dense_wgrad_x6;     /* 1 (default): the weight gradient of Dense trunk layers and of the generic 64x64 fused-backward
                                 pair (ImpalaCnnOpt's 11x11 conv) on the bf16 matrix cores (bf16x6, both operands split when
                                 they are written to LDS) inside the fused backward launch; 0: fp32 MFMA (ABI >= 10; measured
                                 18.0 -> 16.9 us for PpoCnn's Dense backward, -1.1 % for pong_impala_speedup; the other conv
                                 layers lose);
                                 2 = experiment: additionally the halo-instance conv weight gradient (PpoCnn conv3) in a
                                 one-LDS-stage bf16x6 form -- measured +0.9 us per step, kept for A/Bs only               */
  int32_t fwd_fuse12;         /* (round 6) > 0: a network whose first two layers are ImpalaCnnOpt's 84x84 pair (uint8 8x8/4 SAME
                               * 4 -> 16, then 4x4/2 SAME 16 -> 32) runs them as ONE launch per frame stack (conv1's output stays
                               * in LDS for conv2, xt_conv1.hip: conv_u8c4_same_fwd2_kernel) when the batch has at most this many
                               * frames.  DEFAULT 0 (two launches): built, parity-green and MEASURED SLOWER -- 87.6 vs 83.7 us
                               * per 128-frame train, same box: 128 workgroups leave half the CUs idle and conv2 from LDS on fp32
                               * MFMA is 64 MFMAs x 64 cycles per wave, two waves per SIMD = 3.4 us */
  int32_t bwd_fuse21;         /* (appended under ABI 12) a one-trunk network whose first two layers are PpoCnn's pair (uint8 8x8 VALID
                               * 4 -> 32 relu, then 4x4/2 VALID 32 -> 32): the input-gradient blocks of conv2's fused backward launch
                               * keep their 512 pixels of d(act1) in registers -- accumulator x relu' from conv1's sign mask, split
                               * into bf16 planes -- and run conv1's weight-gradient loop on them (xt_igemm.hip: Fuse21Args).  d(act1)
                               * is never written and conv1's own weight-gradient launch disappears.
                               * 0: off (two launches); 1: where the flattened first-layer weight gradient would run (>= 200
                               * workgroups, i.e. B >= 255 at 84x84); 2: at every batch size (tests).  Other nets are unaffected.
                               * Measured FASTER than the two launches on one box, alternating: 6.65 vs 6.95 ms per 4096-sample update
                               * (-4.3 %, every run below every run of the other arm); 27.3 us in one launch instead of 19.1 + 13.8 us,
                               * 16 MB less written and 16 MB less read per step (profiles/bwd_fuse21_ab.md).
                               * DEFAULT 0 all the same: it changes conv1's gradient at fp32 summation-order level (2e-7 relative per
                               * step, every other gradient bitwise equal), and 52 sign-like Adam steps amplify that to 19 % of an
                               * update's parameter delta -- the default update would no longer be the one the full-update parity test
                               * and recorded benchmark outputs pin.  Opt in with bwd_fuse21 = 1 */
} xt_tuning;
int xt_tuning_get(xt_tuning* out);
int xt_tuning_set(const xt_tuning* in);

/* ------------------------------------------------------------- geometry */
/* One Conv2D / Dense layer as an implicit GEMM  Y[M,N] = act(im2col(X)[M,K] . W[K,N] + b).
 * Dense: H=W=KH=KW=S=1, C=in features.  pad_top/pad_left are TensorFlow's
 * (SAME puts the odd cell at bottom/right, so only top/left are needed).
 * Replaces keras Conv2D/Dense built in xt/model/model_utils.py:83-97 and
 * xt/model/impala/impala_cnn_opt.py:119-141. */
typedef struct xt_conv_geom {
  int32_t H, W, C;      /* input height, width, channels (NHWC)            */
  int32_t KH, KW, S;    /* kernel height/width, stride                      */
  int32_t PT, PL;       /* zero padding before the first row / column       */
  int32_t OH, OW, N;    /* output height, width, channels                   */
  int32_t act;          /* XT_ACT_* applied to the output                   */
} xt_conv_geom;

/* how a uint8 observation becomes fp32: (x - mean) / std ; mean==0 -> x / std
 * (layer_function xt/model/model_utils.py:187-189, state_transform :192-201) */
typedef struct xt_input_xform {
  int32_t is_u8;        /* 1: `in` is uint8, 0: `in` is float32 (no transform) */
  float mean, std;
} xt_input_xform;

/* --------------------------------------------------- returns (HBM-bound) */
/* GAE(gamma, lambda), float64, one GPU thread per trajectory, bit-exact with numpy.
 * Replaces PPO.data_proc, xt/agent/ppo/ppo.py:87-104.
 *   value   [n_traj, T+1] f32   reward [n_traj, T] f64   done [n_traj, T] u8 (0/1)
 *   adv, target_value [n_traj, T] f64     old_value [n_traj, T] f32 */
int xt_gae_f64(const float* value, const double* reward, const uint8_t* done,
               double* adv, double* target_value, float* old_value,
               int32_t n_traj, int32_t T, double gamma, double lam, void* stream);

/* The same GAE for a whole rollout of RAGGED trajectories laid out back to back as rows, the form the learner-side
 * ingest holds them in (ABI >= 9): trajectory i = rows [offsets[i], offsets[i+1]) of reward / done / adv /
 * target_value; value_rows[r] = V(s_r) (float32: the column the reference ships as `old_value`); boot[i] = V of the
 * state after trajectory i's last step (value[T], xt/agent/ppo/ppo.py:90).  One workgroup per trajectory, bit-exact
 * with the reference's numpy loop (xt/agent/ppo/ppo.py:87-104; CartPole twin cartpole_ppo.py:98-115).  offsets:
 * int32 [n_traj + 1] on the device. */
int xt_gae_f64_ragged(const float* value_rows, const float* boot, const double* reward, const uint8_t* done,
                      const int32_t* offsets, double* adv, double* target_value, int32_t n_traj, double gamma,
                      double lam, void* stream);

/* v-trace of the non-opt IMPALA from action probabilities (xt/algorithm/impala/impala.py:139-167; appended under
 * ABI 12), float64, one workgroup per fragment.  ROW layout: a fragment holds T + 1 observation rows and T
 * transitions; every array here is indexed by observation row r = f*(T+1) + t, slot t = T of each fragment carries no
 * transition (its inputs are not read), so that xt_keras_impala_loss gathers labels and observations through one idx.
 *   policy    [n_frag*(T+1), A] f32   policy_is_logits 1: the forward's logits (float64 softmax taken here, max
 *                                     subtracted); 0: probabilities, used as they are
 *   value     [n_frag*(T+1)]    f32   V(s) of every row (slot T bootstraps the fragment)
 *   onehot, behaviour [n_frag*(T+1), A] f32   taken action / behaviour policy's probabilities
 *   reward    [n_frag*(T+1)]    f64   done [n_frag*(T+1)] u8
 *     disc = done ? 0 : gamma;  rho = min(1, exp(log(pt + 1e-10) - log(pb + 1e-10))), pt/pb = sum_a p_a * onehot_a
 *     acc_t = rho_t ((r_t + disc_t V_{t+1}) - V_t);  acc_j += (acc_{j+1} disc_{j+1}) rho_{j+1};  target_t = V_t + acc_t
 *     pg_t = rho_t ((r_t + disc_t target_{t+1}) - V_t),  target_T := V_T
 *   pg_adv, target [n_frag*(T+1)] f32: the float64 results rounded once; slot T: pg_adv = 0, target = V_T
 *   debug (may be NULL) [3, n_frag*(T+1)] f64: rho, pg_adv, target before the rounding; slot T: 0, 0, V_T
 * Everything after rho is rounded step by step in numpy's association: bit-for-bit numpy on the same rho.
 * 1 <= T <= 1024, 1 <= A <= 64. */
int xt_vtrace_probs_f64(const float* policy, int32_t policy_is_logits, const float* value, const float* onehot,
                        const float* behaviour, const double* reward, const uint8_t* done, int32_t n_frag, int32_t T,
                        int32_t A, double gamma, float* pg_adv, float* target, double* debug, void* stream);

/* Zero-pad the innermost axis: src [rows, c_src] -> dst [rows, c_dst], elements of elem_bytes = 1 (uint8) or 4
 * (float32) bytes (ABI >= 9).  The reference's get_cnn_backbone (xt/model/model_utils.py:49-80) takes any channel
 * count (examples/ant_ppo.yaml:20: [84, 84, 3]); the layer kernels read 4-channel groups, so such observations enter
 * the first layer with a zero plane and its kernel carries a zero input-channel row that stays zero (zero operand ->
 * zero gradient -> zero Adam step): bit-for-bit the arithmetic of the unpadded layer.  fill_u8: the byte written into
 * the extra uint8 planes -- the value the input transform maps to 0 (state_mean; 0 for x / 255); float32 planes get 0. */
int xt_pad_channels(const void* src, void* dst, int64_t rows, int32_t c_src, int32_t c_dst, int32_t elem_bytes,
                    int32_t fill_u8, void* stream);

/* Advantage normalisation over the whole rollout, in place, float64 (ABI >= 8):
 *     adv <- (adv - mean(adv)) / (std(adv) + eps)        (numpy's population std)
 * the line the reference carries commented out, xt/algorithm/ppo/ppo.py:73 -- so it is an option of the plugin
 * (model_config ADV_NORM, default False), applied to the concatenated rollout before Model.train.  One workgroup,
 * wave-level (DPP shuffle) reductions in a fixed order.  stats (may be NULL): 2 doubles, mean and std. */
int xt_adv_normalize_f64(double* adv, int64_t n, double eps, double* stats, void* stream);

/* ------------------------------------------------ rollout staging (host) */
/* Copy `bytes` of an arriving rollout array from (pageable) host memory `src` into the page-locked staging buffer
 * `dst_pinned` with a pool of native worker threads (non-temporal stores), in work units of `chunk_bytes` (<= 0:
 * 256 KiB); if dev_dst != NULL, a hipMemcpyAsync to dev_dst + offset is enqueued on `stream` for every `ship_bytes`
 * (<= 0: 4 MiB) of contiguous staged data and for the remainder, so the H2D of one piece runs under the staging of
 * the next (and the H2D of one trajectory under the staging of the following one).  n_threads < 0: the tuned count
 * (xt_stage_tune); 0: the calling thread copies inline (still chunked and pipelined with the H2D).  Returns when everything is staged and enqueued; the caller releases the GIL (ctypes does).
 * Host pointers.  ABI >= 8.  Replaces the host half of the reference's rollout hand-over: np.concatenate of the
 * trajectories + the feed_dict upload of every minibatch (xt/algorithm/ppo/ppo.py:66-71, xt/model/ppo/ppo.py:123-129;
 * called from the learner thread's prepare_data loop, xt/framework/learner.py:306-313). */
int xt_stage_rows(void* dst_pinned, const void* src, int64_t bytes, void* dev_dst, int64_t chunk_bytes,
                  int64_t ship_bytes, int32_t n_threads, void* stream);
/* Measure the staging copy on this host inline and with 1/2/4/8 worker threads x {memcpy, non-temporal stores} on a
 * private sample of `sample_bytes` (staged in trajectory-sized pieces, as an ingest burst does) and keep the fastest
 * as the default of xt_stage_rows.  gbps10 (may be NULL): the ten measured rates in GB/s,
 * [memcpy: inline,1,2,4,8 threads | non-temporal: inline,1,2,4,8 threads]. */
int xt_stage_tune(int64_t sample_bytes, float* gbps10);
int xt_stage_get(int32_t* threads, int32_t* non_temporal);
int xt_stage_set(int32_t threads, int32_t non_temporal);

/* ----------------------------------------------- implicit-GEMM layer ops */
/* Forward of one layer.  in: [B,H,W,C] (u8 or f32); idx (may be NULL): [B] int32 row
 * gather -- sample b is read from in[idx[b]] (replaces the numpy fancy-index minibatch
 * gather state[0][mbinds], xt/model/ppo/ppo.py:123).  w,bias: [K,N],[N]; y: [B*OH*OW,N].
 * ksplit>1 computes partial sums into `partial` [ksplit, M, N] and finishes (bias+act)
 * with a second kernel.  Replaces the Conv2D/Dense forward inside sess.run,
 * xt/model/ppo/ppo.py:129, impala_cnn_opt.py:255. */
int xt_layer_fwd(const xt_conv_geom* g, const xt_input_xform* xf, int32_t B,
                 const void* in, const int32_t* idx, const float* w, const float* bias,
                 float* y, float* partial, int32_t ksplit, void* stream);

/* Weight+bias gradient of one layer: dW[K,N] = im2col(X)^T . dY, db[N] = sum_m dY.
 * dy is the gradient w.r.t. the PRE-activation output, [M,N].  dwb receives
 * [(K+1)*N] floats (kernel grad then bias grad).  msplit>1 reduces over M in `msplit`
 * slabs written to `slabs` [msplit,(K+1)*N] and summed by a second kernel
 * (deterministic; no atomics).  Replaces tf.gradients inside
 * AdamOptimizer.compute_gradients, xt/model/ppo/ppo.py:99. */
int xt_layer_wgrad(const xt_conv_geom* g, const xt_input_xform* xf, int32_t B,
                   const void* in, const int32_t* idx, const float* dy,
                   float* dwb, float* slabs, int32_t msplit, void* stream);

/* Input gradient of one layer, fused with the activation gradient of the producer:
 * dx[b,iy,ix,c] = act'(x)*sum dY.W^T, where x (fp32 [B,H,W,C]) is the producer's
 * post-activation output and act_prev its activation.  Strided convs are decomposed
 * into S*S parity classes so that no MAC is spent on structural zeros.
 * Limit: the gradient tensor dy (B*OH*OW*N floats) must be smaller than 2 GiB -- the kernels
 * address it with 32-bit byte offsets of buffer loads (error otherwise; the same holds for the
 * activation and gradient tensors of a layer inside xt_net_*). */
int xt_layer_dgrad(const xt_conv_geom* g, int32_t B, const float* dy, const float* w,
                   const float* x, int32_t act_prev, float* dx, void* stream);

/* The fused backward launch of one non-first trunk layer as the update runs it (weight + bias gradient and input
 * gradient in ONE launch), stand-alone for tests: no head weight-gradient blocks, no norm partials.
 *   x      [B,H,W,C] f32: the producer's output (the weight gradient's operand)
 *   x_pre  NULL, or the producer's pre-activation when act_prev needs it (swish, gelu: see XT_ACT_SWISH)
 *   relu_mask NULL, or the producer's relu sign mask (bit c of word p = x[p,c] > 0; read where C = 32)
 *   dx     [B,H,W,C] = act_prev'(.) * col2im(dY . W^T);  dwb [(K+1)*N] = [dW | db] (final, as xt_layer_wgrad)
 *   slabs  [slab_cap, (K+1)*N] (may be NULL with msplit <= 1 -- the per-sample forms then stay off)
 * *path_out (may be NULL) receives the branch taken: XT_BWD_PATH_* | dg mode << XT_BWD_DG_SHIFT | XT_ARITH_* <<
 * XT_BWD_ARITH_SHIFT, where the dg mode is the input gradient's form (0 LDS-tiled, 1 register-direct, 2 all
 * parity classes per block, 3 register-direct 64-row tiles, 4 ... with the dY halo in LDS, 5 sample per workgroup). */
#define XT_BWD_PATH_S2FUSED 1        /* 4x4/2 16->32, B >= 512: input + weight gradient per sample, one slab each   */
#define XT_BWD_PATH_S2C16 2          /* 4x4/2 16->32: sample-per-workgroup bf16x6 input gradient, tiled weight grad */
#define XT_BWD_PATH_HALO 3           /* stride-1 halo input gradient in its own instance (bf16x6 or fp32)           */
#define XT_BWD_PATH_CLASSES_PF4 4    /* all-classes stride-2 input gradient, four taps in flight, launch cut to 512 */
#define XT_BWD_PATH_CLASSES_WROWS 5  /* ... next to the staged-rows weight gradient (wgrad_rows 1 / 2)             */
#define XT_BWD_PATH_CLASSES 6        /* ... plain form                                                              */
#define XT_BWD_PATH_PF_GENERIC 7     /* Dense deep-prefetch instance (1x1, stride 1)                                */
#define XT_BWD_PATH_PAIR_SS 8        /* generic tile pair: 128x32 weight gradient, 128x32 input gradient            */
#define XT_BWD_PATH_PAIR_SL 9        /* ... 128x32 weight gradient, 64x64 input gradient                            */
#define XT_BWD_PATH_PAIR_LS 10       /* ... 64x64 weight gradient, 128x32 input gradient                            */
#define XT_BWD_PATH_PAIR_LL 11       /* ... 64x64 weight gradient, 64x64 input gradient                             */
#define XT_BWD_PATH_PAIR_LL_WX6 12   /* ... 64x64 pair with the bf16x6 weight gradient (dense_wgrad_x6)             */
#define XT_BWD_DG_SHIFT 8
#define XT_BWD_ARITH_SHIFT 12
int xt_layer_bwd(const xt_conv_geom* g, int32_t B, const float* x, const float* x_pre, const float* dy,
                 const float* w, int32_t act_prev, const uint32_t* relu_mask, float* dx, float* dwb, float* slabs,
                 int32_t slab_cap, int32_t msplit, void* stream, int32_t* path_out);

/* --------------------------------------------------------------- heads */
/* logits[B,A] = f_pi.Wpi + bpi ; value[B] = f_v.Wv + bv.   (pi_latent / output_value
 * Dense layers, xt/model/model_utils.py:64-65; 1x1 Conv2D policy + dense baseline,
 * impala_cnn_opt.py:138-152). */
int xt_heads_fwd(const float* f_pi, const float* f_v, int32_t B, int32_t F, int32_t A,
                 const float* wpi, const float* bpi, const float* wv, const float* bv,
                 float* logits, float* value, void* stream);

/* PPO clipped-surrogate + entropy + clipped-critic loss and its gradient w.r.t.
 * logits and value.  Replaces actor_loss_with_entropy / critic_loss
 * (xt/model/ppo/__init__.py:4-25), CategoricalDist (xt/model/tf_dist.py:103-113) and
 * their tf.gradients.  Labels are gathered through idx (may be NULL) like the
 * observations.  adv/target_v are float64 as the actor produces them and are rounded
 * to fp32 on load (the reference's float32 placeholders, xt/model/ppo/ppo.py:65-68).
 * inv_b = 1/(global minibatch size).  loss_terms [B,4]: surr, entropy, vf, 0. */
int xt_ppo_loss(const float* logits, const float* value, int32_t B, int32_t A,
                const int32_t* idx, const int32_t* action, const float* old_logp,
                const double* adv, const float* old_v, const double* target_v,
                float clip_ratio, float ent_coef, float vf_clip, float critic_coef,
                float inv_b, float* dlogits, float* dvalue, float* loss_terms,
                void* stream);

/* The same loss with the continuous-action distribution: DiagGaussianDist
 * (xt/model/tf_dist.py:47-87) over dist_param = concat([pi_latent, pi_latent*0 + pi_logstd])
 * (xt/model/ppo/ppo.py:75-79; examples/pendulum_ppo.yaml).  mean [B,A] is the pi_latent
 * output, log_std [A] the trainable state-independent variable, action float32 [N,A]
 * (gathered through idx).  dmean [B,A]; dlogstd_rows [B,A] holds every sample's
 * contribution to d loss / d pi_logstd (their fixed-order sum over B is the gradient). */
int xt_ppo_loss_gauss(const float* mean, const float* log_std, const float* value, int32_t B,
                      int32_t A, const int32_t* idx, const float* action, const float* old_logp,
                      const double* adv, const float* old_v, const double* target_v,
                      float clip_ratio, float ent_coef, float vf_clip, float critic_coef,
                      float inv_b, float* dmean, float* dvalue, float* dlogstd_rows,
                      float* loss_terms, void* stream);

/* loss scalar from the per-sample terms of xt_ppo_loss:
 * out[0]=loss, out[1]=actor_loss, out[2]=critic_loss, out[3]=mean entropy;
 * if acc != NULL, acc[0] += loss (running sum for the mean over minibatches,
 * xt/model/ppo/ppo.py:130-132). */
int xt_ppo_loss_reduce(const float* loss_terms, int32_t B, float ent_coef, float critic_coef,
                       float inv_b, float* out, float* acc, void* stream);

/* IMPALA: v-trace targets + loss gradient for one chunk of n_traj trajectories of T
 * steps (flat env-major index b*T+t).  Replaces split_batches / vtrace_loss
 * (impala_cnn_opt.py:171-196,299-351) and vtrace.from_logic_outputs (vtrace.py:39-115).
 * done: u8, reward: f32 (clipped to [-1,1] here).  out: >= 4+n_traj floats, out[0]=loss (sum form).
 * vs/pg_adv (optional, may be NULL): [n_traj,T-1] for parity tests. */
int xt_impala_loss(const float* logits, const float* baseline, const float* bp_logits,
                   const int32_t* action, const uint8_t* done, const float* reward,
                   int32_t n_traj, int32_t T, int32_t A, float gamma,
                   float* dlogits, float* dbaseline, float* out, float* acc,
                   float* vs, float* pg_adv, void* stream);

/* Loss of the non-opt IMPALA models (ABI >= 5): Keras `impala_loss` on the SOFTMAX output plus 0.5 * mse of
 * the value head (xt/model/impala/impala_cnn.py:94-108 + model.compile(loss_weights), impala_mlp.py:83-93):
 *     p = softmax(logits);  L_pi = mean_{b,a}( adv_b * (-y_ba * log(p_ba + 1e-10)) - ent * (-p_ba * log(p_ba + 1e-10)) )
 *     L = L_pi + 0.5 * mean_b (value_b - target_b)^2
 * idx (may be NULL) gathers the rows of adv [N], onehot [N,A], target_v [N] that belong to this minibatch (the
 * logits / value rows are already in minibatch order).  out: >= 4 + 2*B floats; out[0] = L, out[1] = L_pi,
 * out[2] = mse, the rest is scratch.  acc (may be NULL): acc[0] += L * B, acc[1] += B (Keras reports the
 * sample-weighted mean of an epoch).  A <= 64. */
int xt_keras_impala_loss(const float* logits, const float* value, int32_t B, int32_t A, const int32_t* idx,
                         const float* adv, const float* onehot, const float* target_v, float ent_coef,
                         float* dlogits, float* dvalue, float* out, float* acc, void* stream);

/* tf.keras.optimizers.Adam(lr, clipnorm, decay) on a flat parameter buffer made of n_seg tensors
 * [seg_off[i], seg_off[i] + seg_size[i]) (ABI >= 5; impala_cnn.py:60 `Adam(lr=LR, clipnorm=40., decay=...)`):
 * every gradient TENSOR is clipped to clipnorm by its own norm (clip_by_norm; clipnorm <= 0: no clipping), then
 *     m = b1 m + (1-b1) g;  v = b2 v + (1-b2) g^2;  theta -= lr_t * m / (sqrt(v) + eps)
 * with lr_t = lr / (1 + decay * iterations) * sqrt(1 - b2^t) / (1 - b1^t), t = iterations + 1, computed by the
 * caller (eps = 1e-7 in tf.keras).  scratch: >= 16 * n_seg floats.  n_seg <= 32. */
int xt_adam_keras(float* param, const float* grad, float* m, float* v, int32_t n_seg, const int64_t* seg_off,
                  const int64_t* seg_size, float clipnorm, float lr_t, float beta1, float beta2, float eps,
                  float* scratch, void* stream);

/* Backward through the two heads: head weight/bias gradients and the gradient w.r.t.
 * the trunk features (times the producer's activation gradient).  If f_v == f_pi the
 * trunk is shared and df_v must equal df_pi (contributions are summed). */
int xt_heads_bwd(const float* f_pi, const float* f_v, int32_t B, int32_t F, int32_t A,
                 const float* wpi, const float* wv, const float* dlogits, const float* dvalue,
                 int32_t act_prev, float* dwpi, float* dbpi, float* dwv, float* dbv,
                 float* df_pi, float* df_v, void* stream);

/* ----------------------------------------------------------- optimiser */
/* state[8] floats on the device: [0]=beta1^t [1]=beta2^t [2]=scale [3]=alpha
 * [4]=global_norm [5]=step(as float) [6]=device-side error word (0 = none; 1 = the grid barrier of the fused update tail,
 * xt_tuning.tail_fused, timed out: that update was SKIPPED, parameters untouched) [7] reserved.  Initialise with
 * xt_adam_state_init (beta powers = 1). */
int xt_adam_state_init(float* state, void* stream);

/* tf.clip_by_global_norm + tf.train.AdamOptimizer.apply_gradients
 * (xt/model/ppo/ppo.py:97-102, impala_cnn_opt.py:204-217) over one flat buffer:
 *   g  = grad * grad_scale                       (grad_scale = 1/world for a mean loss)
 *   g  = g * clip / max(||g||_2, clip)
 *   lr_t = lr*sqrt(1-b2^t)/(1-b1^t); m += (g-m)(1-b1); v += (g*g-v)(1-b2)
 *   p -= lr_t*m/(sqrt(v)+eps)
 * scratch: >= 1024 floats. */
int xt_adam_tf_clip(float* param, const float* grad, float* m, float* v, int64_t count,
                    float lr, float beta1, float beta2, float eps, float clip_norm,
                    float grad_scale, float* state, float* scratch, void* stream);

/* the two halves of the above, for data-parallel use (all-reduce in between is the
 * caller's): xt_grad_sqnorm fills state[2..4] from the (already reduced) gradient. */
int xt_grad_global_norm(const float* grad, int64_t count, float clip_norm, float grad_scale,
                        float* state, float* scratch, void* stream);

/* ------------------------------------------------------------- network */
/* A whole actor-critic network + update loop, so that one C call enqueues a complete
 * Model.train().  Buffers stay caller-owned. */
typedef struct xt_net xt_net;

#define XT_ACTION_CATEGORICAL 0    /* action: int32 [N]       (CategoricalDist, tf_dist.py:89)  */
#define XT_ACTION_DIAG_GAUSSIAN 1  /* action: float32 [N, A]  (DiagGaussianDist, tf_dist.py:47) */

typedef struct xt_layer_desc {
  xt_conv_geom g;
  int64_t param_off;    /* offset (floats) of this layer's [K*N]+[N] block in the flat buffer */
  int32_t trunk;        /* 0 = pi (or shared) trunk, 1 = v trunk                                */
} xt_layer_desc;

typedef struct xt_net_desc {
  int32_t n_layers;
  const xt_layer_desc* layers;  /* trunk 0 layers first (in order), then trunk 1 layers */
  int32_t n_trunks;             /* 1 shared, 2 separate pi/v trunks                      */
  int32_t feat;                 /* features entering the heads                            */
  int32_t action_dim;
  int64_t pi_off, v_off;        /* offsets of [F*A]+[A] and [F]+[1] head blocks           */
  int64_t n_params;
  xt_input_xform xf;
  int32_t in_h, in_w, in_c;     /* observation shape                                      */
  int32_t action_type;          /* XT_ACTION_CATEGORICAL | XT_ACTION_DIAG_GAUSSIAN (ABI >= 2) */
  int64_t logstd_off;           /* offset of pi_logstd [A] (DiagGaussian only; multiple of 4) */
} xt_net_desc;

int xt_net_create(const xt_net_desc* desc, int32_t max_batch, xt_net** out);
void xt_net_destroy(xt_net* net);
/* bytes of fp32 workspace xt_net needs for minibatches of up to max_batch rows */
int64_t xt_net_workspace_bytes(const xt_net* net);
int xt_net_bind(xt_net* net, float* params, float* grads, float* adam_m, float* adam_v,
                float* adam_state, void* workspace, int64_t workspace_bytes);

/* forward only (Model.predict, xt/model/ppo/ppo.py:104-109): logits [B,A], value [B] */
int xt_net_forward(xt_net* net, const void* obs, const int32_t* idx, int32_t B,
                   float* logits, float* value, void* stream);

typedef struct xt_ppo_cfg {
  float lr, beta1, beta2, eps;
  float clip_ratio, ent_coef, vf_clip, critic_coef, max_grad_norm;
  int32_t batch_size, num_sgd_iter;
  float grad_scale;             /* 1/world_size for data parallel, else 1             */
  int32_t global_batch;         /* rows of the GLOBAL minibatch (for the mean); 0 -> local */
  /* ABI >= 9, xt_net_ppo_train only: shard_world > 1 = STRICT data parallelism inside the call -- every rank passes
   * the same rollout and permutations, and takes rows [b0, b1) of every global minibatch (balanced contiguous shards,
   * rank r of shard_world); the means run over the global rows (global_batch is set per minibatch), grad_scale = 1.
   * Needs a gradient exchange (xt_net_set_rccl / xt_net_set_grad_exchange).  0 / 1 = off. */
  int32_t shard_rank, shard_world;
} xt_ppo_cfg;

/* one SGD step on rows idx[0..B) of the rollout: forward, loss, backward -> net grads.
 * `apply` is a boolean: != 0 also runs clip+Adam (single GPU).  loss_out: 4 floats (see
 * xt_ppo_loss_reduce); loss_acc optional running sum. */
int xt_net_ppo_step(xt_net* net, const xt_ppo_cfg* cfg, const void* obs, const int32_t* idx,
                    int32_t B, const void* action /* int32 [N] | float32 [N,A], see XT_ACTION_* */,
                    const float* old_logp, const double* adv,
                    const float* old_v, const double* target_v, int32_t apply,
                    float* loss_out, float* loss_acc, void* stream);

/* Model.train of xt/model/ppo/ppo.py:111-132 in one call: NUM_SGD_ITER epochs x
 * ceil(n/BATCH_SIZE) minibatches; perm [num_sgd_iter, n] int32 holds the epoch
 * permutations (the reference's np.random.shuffle, injected).  loss_acc (4 floats): [0] receives the
 * SUM of minibatch losses, [1] the number of minibatches, [2] data-parallel error bits (0 = none; ABI >= 11).  use_graph != 0
 * captures the whole call into a hipGraph on first use and replays it afterwards
 * (pointers and sizes must then stay the same between calls).  The graph is looked up under a key that holds every
 * argument, every cfg field (floats by their exact bits) and the net-level switches that change the enqueued work
 * (training statistics, xt_net_set_gauss_fused, the data-parallel settings): a call that differs in any of them captures
 * its own graph, up to 8 per net (xt_net_graph_cache_info).  NOT part of the key: the process-wide xt_tuning knobs --
 * they stay "set before creating networks"; a graph captured under other knobs is replayed as it was captured. */
int xt_net_ppo_train(xt_net* net, const xt_ppo_cfg* cfg, const void* obs, int32_t n,
                     const int32_t* perm, const void* action, const float* old_logp,
                     const double* adv, const float* old_v, const double* target_v,
                     float* loss_acc, int32_t use_graph, void* stream);

/* Per-update PPO training diagnostics, accumulated on the device inside the step's own launches (appended under ABI 12;
 * opt-in).  `stats`: XT_TRAIN_STATS_DOUBLES doubles, `rows`: [max_batch, 4] floats of scratch (16-byte aligned), both
 * device memory owned by the caller like every other buffer of the net; xt_net_workspace_bytes does not change.  NULL,
 * NULL switches the diagnostics off (the default): every launch is then the one of a net that never had them.  Refused
 * while the net has a data-parallel tail or a gradient exchange hook (the row statistics would be rank-local).
 *
 * With the buffers set, the head launch of every PPO step also stores one float4 per sample,
 *     rows[b] = {old_logp - logp, (!in_rng) + 2 * (!in_v), tv, tv - v}
 * (its own clip predicates; tv = the float32-rounded target it uses), the loss reduction of the step -- the extra block of
 * the gradient-reduction launch in the default tail form, off the critical path; on it in the ticket form and behind a
 * gradient-only step -- reduces the four columns (tv and tv - v also squared, products in double) with the fixed-order
 * double tree of the loss terms, and the thread that writes the pre-clip global norm into adam_state[4] adds it.  Every
 * slot of `stats` is a sum over the SGD steps since the block was cleared, except XT_TRAIN_STATS_GNORM_MAX (a maximum);
 * the sums are taken in one fixed order, so a replayed hipGraph and the eager call give the same bits.  xt_net_ppo_train
 * clears the block at its start; xt_net_ppo_step only accumulates (its caller clears), and with apply == 0 it leaves the
 * three gradient-norm slots alone (no norm is formed).  The pointers are part of xt_net_ppo_train's hipGraph key. */
#define XT_TRAIN_STATS_DOUBLES 16
#define XT_TRAIN_STATS_STEPS 0          /* SGD steps                                                        */
#define XT_TRAIN_STATS_ROWS 1           /* rows visited (sum of the minibatch sizes)                        */
#define XT_TRAIN_STATS_SURR 2           /* sum of the steps' mean clipped surrogate (float, as the loss)    */
#define XT_TRAIN_STATS_ENT 3            /* ... mean entropy                                                 */
#define XT_TRAIN_STATS_VF 4             /* ... critic loss                                                  */
#define XT_TRAIN_STATS_KL 5             /* sum over rows of old_logp - logp                                 */
#define XT_TRAIN_STATS_CLIPPED 6        /* rows with the ratio outside [1 - clip, 1 + clip]                 */
#define XT_TRAIN_STATS_VF_CLIPPED 7     /* rows with |v - old_v| > vf_clip                                  */
#define XT_TRAIN_STATS_TV 8             /* sum over rows of tv                                              */
#define XT_TRAIN_STATS_TV_SQ 9          /* ... tv^2                                                         */
#define XT_TRAIN_STATS_ERR 10           /* ... tv - v                                                       */
#define XT_TRAIN_STATS_ERR_SQ 11        /* ... (tv - v)^2                                                   */
#define XT_TRAIN_STATS_GNORM_SUM 12     /* sum over steps of the pre-clip global gradient norm              */
#define XT_TRAIN_STATS_GNORM_MAX 13     /* its maximum                                                      */
#define XT_TRAIN_STATS_GNORM_CLIPPED 14 /* steps with the norm above max_grad_norm                          */
#define XT_TRAIN_STATS_RESERVED 15      /* 0                                                                */
int xt_net_set_train_stats(xt_net* net, double* stats, float* rows);
/* Which head / loss kernel the most recent PPO step of this net launched (diagnostic): the XT_HEAD_PATH_PPO_FUSED word
 * of xt_ppo_heads_fused_ex for the fused kernel (the XT_HEAD_PATH_PPO_GAUSS_FUSED word of xt_ppo_gauss_heads_fused_ex for
 * the fused DiagGaussian one, see xt_net_set_gauss_fused), else one of the two codes below; 0 before the first step. */
#define XT_NET_HEAD_PLAIN 0x10000       /* heads forward + ppo_loss_kernel + heads d(features)              */
#define XT_NET_HEAD_GAUSS 0x20000       /* heads forward + ppo_loss_gauss_kernel + heads d(features)        */
int32_t xt_net_last_head_path(const xt_net* net);
/* The fused head launch for a DiagGaussian policy (appended under ABI 12; opt-in, per net).  on == 0 (the default): every
 * launch is the one of a net that never had the switch (heads forward + ppo_loss_gauss_kernel + heads d(features);
 * xt_net_last_head_path == XT_NET_HEAD_GAUSS).  on != 0: a PPO step whose head is inside the fused kernel's envelope
 * (A <= 8, features <= 512, no layer that keeps its pre-activation) runs ppo_gauss_heads_fused_kernel instead, the last
 * trunk layer's split-K finish deferred into it as for a categorical policy; xt_net_last_head_path then returns
 * XT_HEAD_PATH_PPO_GAUSS_FUSED | nq | part | shared (see xt_ppo_gauss_heads_fused_ex).  Outside the envelope the step
 * silently keeps the three launches.  The fused kernel takes the sums over the action dimensions as wave sums, so its
 * float32 results differ from the default's in the last bits.  Refused on a categorical net.  The flag is part of
 * xt_net_ppo_train's hipGraph key. */
int xt_net_set_gauss_fused(xt_net* net, int32_t on);
/* PpoCnn's first two layers in one forward launch (appended under ABI 12; per net, default ON).  on != 0: a trunk whose
 * first layer is the uint8 8x8/4 VALID 4 -> 32 layer of the flat bf16x3 form, followed by a 4x4/2 VALID 32 -> 32 layer,
 * neither keeping its pre-activation, runs conv12_u8_valid_fwd_flat_kernel for both when the batch is inside the
 * kernel's envelope (the second layer's own forward would neither be split over K nor leave its four-wave-group form:
 * 201 <= B <= 404 for 84x84 frames); every other forward keeps the two launches.  Both activations, the
 * sign mask and everything downstream are bit for bit what the two launches give.  on == 0: always two launches.  The
 * flag is part of the key of every cached hipGraph of the net. */
int xt_net_set_fwd_fuse12_flat(xt_net* net, int32_t on);
/* PpoCnn's first THREE layers in one forward launch (appended under ABI 12; per net, default ON).  on != 0: a trunk that
 * would take the launch above and whose third layer is the 3x3/1 VALID 32 -> 64 one, with a further layer behind it, runs
 * conv123_u8_valid_fwd_flat_kernel for all three when neither the second nor the third layer's own forward would be split
 * over K and the automatic split needs at most one workgroup per CU (201 <= B <= 320 for 84x84 frames); every other
 * forward is the one of a net that never had the switch.  The three activations, the sign mask and everything downstream
 * are bit for bit what the separate launches give.  Needs xt_net_set_fwd_fuse12_flat on (its default).  The tail word
 * XT_STEP_TAIL_FWD_FUSE123 of xt_net_last_step_report is 1 after a forward that took it.  The flag is part of the key
 * of every cached hipGraph of the net. */
int xt_net_set_fwd_fuse123_flat(xt_net* net, int32_t on);

/* Gradient exchange hook of xt_net_ppo_train (ABI >= 4): the reference's learner is single-process
 * (its grad_communicate host averaging, xt/framework/trainer.py:89-92, is dead code); data parallelism is this
 * library's own extension.  When a hook is set, every SGD step of xt_net_ppo_train runs as
 *     gradient-only step -> fn(net.grads, n_params, user, stream) -> global norm of the EXCHANGED gradient,
 *     clip, Adam
 * on the same stream, so that with use_graph != 0 the exchange is captured into the hipGraph of the update
 * together with the kernels (fn is then called at capture time only).  fn must enqueue an in-place SUM
 * all-reduce of `count` floats at `grads` on `stream` and return 0 -- e.g. a wrapper around
 * ncclAllReduce(grads, grads, count, ncclFloat, ncclSum, comm, stream) of the RCCL instance the process already
 * uses (xingtian_amd/parallel.py::RcclComm).  cfg.grad_scale / cfg.global_batch carry the 1/world scaling as in
 * the step-wise path.  fn == NULL removes the hook. */
typedef int (*xt_grad_exchange_fn)(float* grads, int64_t count, void* user, void* stream);
int xt_net_set_grad_exchange(xt_net* net, xt_grad_exchange_fn fn, void* user);
/* The same with flags (ABI >= 8).  XT_XCHG_OVERLAP (shared-trunk networks): every SGD step of xt_net_ppo_train
 * exchanges the gradient in TWO buckets -- [offset of the last trunk layer, n_params) = that layer + the heads (the
 * first gradients the backward pass produces; 95 % of PpoCnn's parameters), reduced and handed to fn on a side stream
 * of the library right after the first backward launch, so that its all-reduce runs under the conv backward; then
 * [0, that offset) on the compute stream, which finally waits for the side stream before the norm + clip + Adam.
 * fn is called twice per step, each time with its own sub-range and stream; the calls are issued in the same order on
 * every rank (RCCL's ordering requirement for one communicator). */
#define XT_XCHG_OVERLAP 1
int xt_net_set_grad_exchange_ex(xt_net* net, xt_grad_exchange_fn fn, void* user, int32_t flags);

/* The exchange served by the library itself (ABI >= 9): every hook call becomes
 *     allreduce(grads, grads, count, ncclFloat32 (7), ncclSum (0), comm, stream)
 * through the ncclAllReduce entry point the caller resolved from the RCCL instance its process already uses (dlsym /
 * ctypes on torch's librccl.so) -- no host-language trampoline on the enqueue path.  comm == NULL removes it.
 * xt_net_rccl_status: number of calls made and the last non-zero ncclResult (0 = none). */
typedef int (*xt_nccl_allreduce_fn)(const void* sendbuff, void* recvbuff, size_t count, int datatype, int op,
                                    void* comm, void* stream);
int xt_net_set_rccl(xt_net* net, void* comm, xt_nccl_allreduce_fn allreduce, int32_t flags);
int xt_net_rccl_status(const xt_net* net, int32_t* calls, int32_t* last_error);

/* ---- Direct 2-phase all-reduce over peer-mapped device memory (ABI >= 10; SURVEY.md 8(b) `xt_allreduce_direct`).
 * Replaces: the reference's only gradient exchange, the host-side float64 sum of the whole flat gradient list through a
 * shared RawArray (xt/framework/trainer.py:86-92, message shape :139-144; dead code there) -- here between the GPUs of one
 * node, one process per GPU, without a host hop and without RCCL's ring (xGMI is a point-to-point mesh: both phases talk
 * to all N-1 peers at once).
 *
 *   xt_direct_create   allocates this rank's exchange block (flags + one inbox slot per rank + a result buffer, sized for
 *                      max_count floats) and writes its 64-byte hipIpcMemHandle_t to handle_out (may be NULL for in-process
 *                      groups).  rank in [0, world), world <= 16.  The block is UNCACHED device memory (published with
 *                      s_waitcnt + a system-scope flag store, nothing to invalidate on the consumer side); cached kinds
 *                      measured stale flag polls (plain) / wrong sums (fine-grained) across the XCDs' L2s and are not offered.
 *   xt_direct_connect  handles = world x XT_DIRECT_HANDLE_BYTES bytes, rank order (as gathered over any side channel,
 *                      e.g. torch.distributed all_gather); maps every peer's block (hipIpcOpenMemHandle).
 *   xt_direct_connect_local  the same for N logical ranks inside ONE process (ranks[q] = the comm object of rank q).
 *   xt_allreduce_direct  in-place SUM of buf[0..count) over the ranks, enqueued on `stream` as three kernels (push scatter ->
 *                      fixed-rank-order reduce + push gather -> copy back); capturable into a hipGraph (the sequence number
 *                      lives in device memory).  Every element is summed by exactly one rank in rank order 0..N-1, so all
 *                      replicas receive BIT-IDENTICAL results.  count <= max_count, buf 16-byte aligned.  All ranks must
 *                      call it the same number of times with the same count.  Waits are bounded (default 2 s): a missing
 *                      peer sets an error bit (xt_direct_status: 1 = scatter data never arrived, 2 = reduced slices never
 *                      arrived) instead of hanging the device; the bit is sticky and later waits of the comm return at once.
 *   xt_direct_exchange_hook  xt_grad_exchange_fn adapter: xt_net_set_grad_exchange_ex(net, xt_direct_exchange_hook, comm, 0)
 *                      makes xt_net_ppo_train / xt_net_impala_train exchange through this comm (one bucket per step).
 */
#define XT_DIRECT_HANDLE_BYTES 64
typedef struct xt_direct_comm xt_direct_comm;
int xt_direct_create(int32_t rank, int32_t world, int64_t max_count, void* handle_out, xt_direct_comm** out);
int xt_direct_connect(xt_direct_comm* comm, const void* handles);
int xt_direct_connect_local(xt_direct_comm* comm, xt_direct_comm* const* ranks);
int xt_allreduce_direct(xt_direct_comm* comm, float* buf, int64_t count, void* stream);
/* the all-reduce of an in-process group (xt_direct_connect_local) driven by one host thread: launches issued phase by
 * phase over the n ranks, each on its own stream */
int xt_allreduce_direct_group(int32_t n, xt_direct_comm* const* comms, float* const* bufs, int64_t count,
                              void* const* streams);
int xt_direct_exchange_hook(float* grads, int64_t count, void* user, void* stream);
int xt_direct_set_timeout_ms(xt_direct_comm* comm, int32_t ms);
/* xt_allreduce_direct as ONE launch (default, fused = 1: every block runs scatter -> reduce -> gather and only ever waits for
 * other RANKS' flags) or as the three launches described above (fused = 0; what the in-process group call always uses). */
int xt_direct_set_fused(xt_direct_comm* comm, int32_t fused);
int xt_direct_status(xt_direct_comm* comm, int32_t* calls, int32_t* seq, int32_t* error_bits);
int xt_direct_destroy(xt_direct_comm* comm);
/* ABI >= 11.  xt_direct_info: how many ranks of the group live on THIS rank's device (read from the device identity every
 * rank leaves in its exchange block; 1 on a real multi-GPU node, N when N test processes share one GPU) and the workgroup
 * cap the spinning kernels of this comm are launched with: (resident workgroups of the device) / (ranks on the device) --
 * a kernel whose blocks wait for other ranks' flags must leave room for those ranks' kernels.
 * xt_direct_read_result: the reduced buffer of the most recent exchange (tests; synchronises the device).
 * xt_direct_reset: clears the sticky error word, the tickets, the sequence number and this rank's flag words.  COLLECTIVE:
 * every rank calls it between two host barriers, with no exchange in flight (xingtian_amd/parallel.py::DirectComm.reset). */
int xt_direct_info(xt_direct_comm* comm, int32_t* ranks_on_device, int32_t* block_cap);
int xt_direct_read_result(xt_direct_comm* comm, float* host_out, int64_t count);
int xt_direct_reset(xt_direct_comm* comm);

/* ---- The data-parallel SGD step without host collectives and without gradient copies (ABI >= 11).
 * Replaces the two host-synchronous collectives per Model.train of ABI 10's learner (row-count check, global loss) and the
 * scatter / gather copies of the direct exchange; the reference's analogue of the message is xt/framework/trainer.py:139-144.
 *
 * xt_net_set_dp(net, rank, world, loss_scale): from now on the gradient buffer bound with xt_net_bind holds
 * align4(n_params) + XT_DP_TAIL_FLOATS floats and every exchange of xt_net_ppo_train / xt_net_impala_train covers the TAIL
 * too: slot [r] = rows rank r was handed for this update, slot [16 + r] = rank r's share of the step's loss, all other slots
 * zero -- after the SUM every rank holds every rank's values exactly and the optimiser kernel adds
 * loss_scale * (sum in rank order) to loss_acc[0] (PPO strict / IMPALA: 1, the shares of one sum; PPO weak: 1 / world, the
 * mean of the ranks' means) and raises loss_acc[2] (error bits, 4 = the ranks hold different numbers of rows) -- so one
 * train() is one C call and one read-back of loss_acc, as on one GPU.  world <= 0 switches it off; world == 1 is a
 * one-rank group (the whole chain runs against the rank's own buffers: how bench.py times the data-parallel form of the
 * step on one GPU).  The overlapped
 * two-bucket mode (XT_XCHG_OVERLAP) carries the tail in its first bucket.
 *
 * xt_net_set_direct(net, comm): the direct exchange FUSED into the step (needs xt_net_set_dp; comm sized for
 * align4(n_params) + XT_DP_TAIL_FLOATS floats): the gradient-reduction kernel writes every reduced float4 straight into the
 * owning peer's inbox and raises the ready flags; ONE small launch reduces this rank's slice in rank order, pushes it to every
 * peer's result buffer and leaves the squared-norm partials of the slice with it; the optimiser kernel waits for the done
 * flags, derives the clip factor from all ranks' partials (fixed order: bitwise the same factor everywhere) and reads the
 * gradient out of the result buffer.  Three launches per step tail instead of five, no scatter / gather copy, no separate
 * norm launch.  A wait that runs out (or a row mismatch) sets the sticky error word: the optimiser then SKIPS the update
 * (parameters and slots stay those of the last good step) and loss_acc[2] carries the bits to the host with the loss.
 * comm == NULL detaches. */
#define XT_DP_TAIL_FLOATS 32
int xt_net_set_dp(xt_net* net, int32_t rank, int32_t world, float loss_scale);
int xt_net_set_direct(xt_net* net, xt_direct_comm* comm);

/* One minibatch of Keras `model.fit` for the non-opt IMPALA models (ABI >= 5): forward, xt_keras_impala_loss,
 * backward; the flat gradient is left in the net's gradient buffer for xt_adam_keras.  obs rows are gathered with
 * idx like the label rows (idx may be NULL: rows 0..B-1). */
int xt_net_keras_impala_step(xt_net* net, const void* obs, const int32_t* idx, int32_t B, const float* adv,
                             const float* onehot, const float* target_v, float ent_coef, float* loss_out,
                             float* loss_acc, void* stream);

/* One whole `IMPALA.train` of the non-opt algorithm in ONE call that never synchronises (appended under ABI 12):
 *   1. forward over all n_frag*(T+1) resident observation rows (obs_row_bytes each) in chunks of at most the net's
 *      max batch, logits / value into the caller's buffers;
 *   2. xt_vtrace_probs_f64 (logits mode) -> pg_adv / target, row layout as documented there;
 *   3. for every entry e of the HOST table, in order: xt_net_keras_impala_step on idx[e.off .. e.off + e.rows) with the
 *      labels pg_adv / onehot / target, its loss accumulated into acc[2*e.chunk .. +2), then xt_adam_keras with e.lr_t.
 * acc [2*n_chunks] f32 is zeroed first; the epoch loss of algorithm chunk c (one `model.fit`) is acc[2c] / acc[2c+1].
 * idx holds observation ROWS (f*(T+1) + t, never a slot t = T).  seg_off / seg_size / table are host arrays.
 * Categorical heads only; refused while a gradient exchange or the data-parallel tail is installed. */
typedef struct xt_keras_fit_entry {
  int32_t off, rows;            /* minibatch = idx[off .. off + rows), 1 <= rows <= 128                     */
  int32_t chunk;                /* BATCH_SIZE chunk of the algorithm this minibatch belongs to               */
  float lr_t;                   /* step size of xt_adam_keras for this update                               */
} xt_keras_fit_entry;
typedef struct xt_keras_train_cfg {
  float ent_coef, clipnorm, beta1, beta2, eps;
  double gamma;
  int32_t n_seg;                /* tensors of the flat parameter buffer, as for xt_adam_keras               */
  const int64_t* seg_off;
  const int64_t* seg_size;
  float* adam_scratch;          /* >= 16 * n_seg floats on the device                                       */
} xt_keras_train_cfg;
int xt_net_keras_impala_train(xt_net* net, const xt_keras_train_cfg* cfg, const void* obs, int64_t obs_row_bytes,
                              int32_t n_frag, int32_t T, const float* onehot, const float* behaviour,
                              const double* reward, const uint8_t* done, float* logits, float* value, float* pg_adv,
                              float* target, const int32_t* idx, int32_t n_idx, const xt_keras_fit_entry* table,
                              int32_t n_entries, int32_t n_chunks, float* acc, void* stream);

typedef struct xt_impala_cfg {
  float lr, beta1, beta2, eps;
  float grad_norm_clip, gamma;
  int32_t sample_batch_step;    /* T */
  float grad_scale;
  int32_t opt_type;             /* XT_OPT_ADAM | XT_OPT_RMSPROP_CENTERED (ABI >= 3)                          */
  float rms_decay, rms_eps;     /* tf.train.RMSPropOptimizer(LR, decay=0.99, epsilon=0.1, centered=True),    */
                                /* impala_cnn_opt.py:205-206: uses adam_m as the mean gradient `mg` and       */
                                /* adam_v as the mean square `ms` (the caller initialises ms to ONES as TF)   */
  /* strict data parallelism inside xt_net_impala_train (ABI >= 10): shard_world > 1 -> every rank is handed the SAME   */
  /* rollout and takes whole-trajectory shard shard_rank (balanced, contiguous) of every BATCH_SIZE chunk; the sum-form */
  /* loss makes the SUM of the shard gradients the chunk's gradient (grad_scale 1).  A rank whose shard of a chunk is   */
  /* empty (fewer trajectories than ranks) contributes a zero gradient.  Needs a gradient exchange.                     */
  int32_t shard_rank, shard_world;
} xt_impala_cfg;

#define XT_OPT_ADAM 0
#define XT_OPT_RMSPROP_CENTERED 1

/* ImpalaCnnOpt.train (impala_cnn_opt.py:251-265) on one chunk of n = n_traj*T frames */
int xt_net_impala_step(xt_net* net, const xt_impala_cfg* cfg, const void* obs, int32_t n,
                       const float* bp_logits, const int32_t* action, const uint8_t* done,
                       const float* reward, int32_t apply, float* loss_out, float* loss_acc,
                       void* stream);

/* IMPALAOpt.train of xt/algorithm/impala/impala_opt.py:73-106 in one call (ABI >= 6): the n frames of the
 * concatenated rollout messages are consumed in sequential chunks of batch_size frames (no shuffling; n and
 * batch_size must be multiples of sample_batch_step because split_batches, impala_cnn_opt.py:171-186, reshapes every
 * chunk to [B, T]), one ImpalaCnnOpt.train (forward, v-trace, sum-form loss, backward, clip, optimiser) per chunk.
 * lr_steps (device, may be NULL): step size of every chunk ([ceil(n/batch_size)] floats; the caller evaluates
 * lr_schedule / linear_cosine_decay, impala_cnn_opt.py:234-249, per global_step) -- read on the device so that a
 * replayed hipGraph sees new values; NULL -> cfg->lr.  loss_acc[0] receives the SUM of the chunk losses, loss_acc[1]
 * the number of chunks (the algorithm returns their mean, impala_opt.py:106).  use_graph != 0 captures the call into
 * a hipGraph on first use and replays it while pointers and sizes repeat (a small cache of graphs is kept, so that
 * alternating ingest buffer sets do not re-capture).  A gradient-exchange hook (xt_net_set_grad_exchange) makes every
 * chunk data parallel: local gradient -> exchange (SUM; the loss is a sum, grad_scale = 1) -> norm of the exchanged
 * gradient -> clip + the configured optimiser (Adam or centred RMSProp, lr_steps honoured; ABI >= 9).  The graph key
 * holds every argument, every cfg field (floats by their exact bits) and the v-trace statistics switch; as for
 * xt_net_ppo_train the process-wide xt_tuning knobs are NOT part of it and stay "set before creating networks". */
int xt_net_impala_train(xt_net* net, const xt_impala_cfg* cfg, const void* obs, int32_t n, int32_t batch_size,
                        const float* bp_logits, const int32_t* action, const uint8_t* done, const float* reward,
                        const float* lr_steps, float* loss_acc, int32_t use_graph, void* stream);

/* xt_net_impala_train plus the runtime calls a learner loop issues around it, in ONE call (ABI >= 11): the per-train host path
 * of IMPALAOpt.train (xt/algorithm/impala/impala_opt.py:73-106 inside xt/framework/learner.py:298-380) was ~10 separate
 * Python-level runtime calls (wait for the rollout's copies, launch, mark the buffer set consumed, snapshot the weights, read
 * the loss back, wait) around an 85 us train.  Every member of `io` is optional (NULL / 0 = skip):
 *   wait_event      the stream waits for this event before the first kernel (the rollout's H2D copies)
 *   consumed_event  recorded right behind the train (the rollout's buffer set may be overwritten once it has fired)
 *   loss_host       page-locked host block of 4 floats: loss_acc is copied there; loss_event is recorded behind the copy;
 *                   wait_loss != 0: the call returns when that copy has landed (hipEventSynchronize; the caller's language
 *                   runtime lock is released for the whole call by ctypes)
 *   publish_dst     page-locked HOST block of n_params floats (a transport.WeightsRing slot): the new parameters are copied
 *                   there in stream order BEHIND the loss copy (the next update cannot tear them, the caller's loss wait does
 *                   not include them); publish_event is recorded behind the copy (the ring's committer thread waits for it).
 *                   (Measured alternatives, round 6: a device-side snapshot + the D2H on a side stream under the next train is
 *                   SLOWER -- the D2H into registered host memory is a blit KERNEL that competes with the train's kernels:
 *                   0.29 vs 0.27 ms per 128-frame train --, and the same D2H enqueued later by a helper thread serialises with
 *                   the learner thread's next launch.)
 *   tail_in_graph   (ABI >= 12; honoured with wait_loss != 0 and loss_host set; wait_loss == 2: do not wait, see xt_net_io_wait)
 *                   1: the loss read-back and the parameter copy become the last two KERNELS OF THE TRAIN ITSELF -- inside the
 *                   replayed hipGraph, whose kernel arguments are fixed: the learner thread writes {destination, sequence
 *                   number} into a 64-byte page-locked mailbox the library owns; the first tail kernel reads the mailbox
 *                   over the bus, writes the loss sums + the sequence number back into it (and the sums to loss_acc) and hands
 *                   the destination to the copy kernel through device memory (so the host may rewrite the mailbox as soon as
 *                   it has seen the loss).  The chunks of such a train accumulate into 4 floats of the workspace that the loss
 *                   kernel re-arms: the graph holds no memset node.  The call returns when the sequence number has landed (a
 *                   bounded poll of the page-locked word, stream health checked every ~0.3 ms) and has copied the 4 floats to
 *                   loss_host.  consumed_event / publish_event are optional (an event record behind a replayed graph costs the
 *                   next graph ~10 us: the train's inputs are consumed once its loss has been seen, and the copy kernel reports
 *                   its own completion, xt_net_io_publish_wait); loss_event is not used.
 *                   2: the parameter copy leaves the GPU's critical path: the train's last kernel is a device-side SNAPSHOT
 *                   (params -> one of two buffers of the library, ~5 us, reported through the mailbox), and the 80 us bus-bound
 *                   copy snapshot -> publish_dst runs on the SDMA ENGINE under the next train, issued through the HSA runtime
 *                   by whoever calls xt_net_io_publish_wait for that train (a weights ring's committer thread; the learner
 *                   thread itself when it needs the buffer back, two publishes later).  publish_event must be NULL.  Why not a
 *                   copy kernel or hipMemcpyAsync on a side stream: csrc/xt_sdma.hip (both measured, round 6).  With plain Adam
 *                   and no gradient exchange both tail kernels are FOLDED into the Adam kernel of the train's last chunk (its
 *                   block 0 reports the loss before the update, every block writes the snapshot too, the last block reports it).
 *                   What 1 / 2 remove (rocprofv3 traces of the 128-frame loop): the 19-27 us between a replayed graph and the
 *                   next launch on the stream (twice), the wake-up of hipEventSynchronize, the host's share of the next
 *                   train's launch, and (2) the 74 us copy from between two trains: 210-235 -> ~194 (1) -> ~130 us of GPU time
 *                   per train + publish.
 * Events are hipEvent_t handles (e.g. torch.cuda.Event.cuda_event). */
typedef struct xt_train_io {
  void* wait_event;
  void* consumed_event;
  float* loss_host;
  void* loss_event;
  float* publish_dst;
  void* publish_event;
  int32_t wait_loss;
  int32_t tail_in_graph;
  uint64_t wait_dma_ticket;   /* != 0: the call waits (host side, before the launch) for xt_dma_wait_upto(ticket) */
} xt_train_io;
int xt_net_impala_train_io(xt_net* net, const xt_impala_cfg* cfg, const void* obs, int32_t n, int32_t batch_size,
                           const float* bp_logits, const int32_t* action, const uint8_t* done, const float* reward,
                           const float* lr_steps, float* loss_acc, int32_t use_graph, const xt_train_io* io, void* stream);
/* Second half of a train enqueued with io->tail_in_graph and io->wait_loss == 2 (ABI >= 12): xt_net_impala_train_io returned
 * right behind the launch -- the caller does whatever of its own book-keeping does not depend on the loss while the device
 * trains -- and this call waits (bounded poll of the mailbox, as above) for the loss of the MOST RECENT such train and copies
 * loss_acc's 4 floats to loss_host4 (any host memory). */
int xt_net_io_wait(xt_net* net, float* loss_host4, void* stream);

/* The parameter copy of a tail_in_graph train reports its own completion (ABI >= 12): the copy kernel's last workgroup writes
 * the train's sequence number into the mailbox, so a caller that passes NO publish_event / consumed_event (event records behind
 * a replayed graph delay the next graph on the stream by ~20 us) still learns when the block at publish_dst is complete:
 * xt_net_io_seq = sequence number of the most recent tail_in_graph train of this net (read it right behind the launch);
 * xt_net_io_publish_wait returns 0 once the copy of train `seq` (or a later one) has landed, 1 when timeout_ms ran out
 * (0 = query, < 0 = no limit).  For a tail_in_graph = 2 train it waits for the snapshot's report and then MAKES the copy (SDMA
 * engine, synchronous for the caller; the first thread that comes for a publish makes it, others wait for it; the query form
 * never starts it).  The train's inputs are consumed once its loss has been seen (the loss kernel runs behind every
 * kernel that reads them). */
uint32_t xt_net_io_seq(const xt_net* net);
/* 1 once the loss of the most recent tail_in_graph train has landed in the mailbox (xt_net_io_wait would return at once), else 0:
 * a learner thread that stages the next rollout message ITSELF while the device trains polls this between two messages */
int32_t xt_net_io_loss_ready(const xt_net* net);
int xt_net_io_publish_wait(xt_net* net, uint32_t seq, int32_t timeout_ms);

/* One synchronous device -> page-locked-host copy on the SDMA engine through the HSA runtime of the process (ABI >= 12;
 * csrc/xt_sdma.hip says why not hipMemcpyAsync).  dst_host: hipHostMalloc'ed or hipHostRegister'ed memory; src_dev: a device
 * allocation; the caller has made sure the source is complete (no stream is involved).  Diagnostic / test entry: the library
 * uses the same copy for the parameter block of xt_net_impala_train_io (tail_in_graph = 2). */
int xt_sdma_copy_d2h(void* dst_host, const void* src_dev, int64_t bytes);

/* Asynchronous page-locked-host -> device copies on the SDMA engines through the HSA runtime, with TICKETS instead of streams and
 * events (ABI >= 12): the rollout ingest's per-message H2D (hipMemcpyAsync + the event records around it cost the staging thread
 * ~30 us per message; this ~5).  xt_dma_h2d_async starts one copy and returns its ticket (tickets count up from 1; at most 64 in
 * flight); xt_dma_wait_upto returns 0 once EVERY copy with a ticket <= `ticket` has landed, 1 when timeout_ms ran out (0 = query,
 * < 0 = no limit).  No ordering against any HIP stream: the caller knows that the destination is free (xt_train_io: a train's
 * inputs are consumed once its loss has been seen) and waits for the ticket before it launches what reads the data
 * (xt_train_io.wait_dma_ticket). */
int xt_dma_h2d_async(void* dst_dev, const void* src_host, int64_t bytes, uint64_t* ticket_out);
int xt_dma_wait_upto(uint64_t ticket, int32_t timeout_ms);

/* diagnostic (ABI >= 12): host time (us, accumulated over *calls_out calls with a non-NULL io) of xt_net_impala_train_io's
 * phases -- [0] before the launch (wait for the copies, mailbox), [1] the launch (hipGraphLaunch, or the eager enqueue), [2] the
 * runtime calls behind it (event records, the separate copies when tail_in_graph is off), [3] the wait for the loss.
 * reset != 0 clears the accumulators. */
int xt_net_io_times(xt_net* net, double* us_out4, int64_t* calls_out, int32_t reset);

/* clip + Adam on the net's flat gradient (second half of a data-parallel step) */
int xt_net_apply(xt_net* net, float lr, float beta1, float beta2, float eps, float clip_norm,
                 float grad_scale, void* stream);

/* introspection for tests/tools: float offsets inside the bound workspace of layer `layer`'s post-activation
 * output [B,OH,OW,N] (out4[0]), its d(pre-activation) buffer (out4[1]), its weight-gradient slabs (out4[2]) and
 * their capacity in slabs (out4[3]) */
int xt_net_layer_offsets(const xt_net* net, int32_t layer, int64_t* out4);

/* arithmetic of the most recent layer launch made through this library by the calling process (diagnostic, for
 * bench.py's roofline: which matrix-core peak a timed kernel is priced against).  ABI >= 7. */
#define XT_ARITH_FP32 0          /* v_mfma_f32_32x32x2_f32                                                     */
#define XT_ARITH_BF16X3 1        /* uint8 x fp32 as 3 x v_mfma_f32_32x32x16_bf16 (first-layer kernels)          */
#define XT_ARITH_BF16X6 2        /* fp32 x fp32 as 6 x v_mfma_f32_32x32x16_bf16                                 */
#define XT_ARITH_FP32_BF16X6 3   /* fused backward launch: weight gradient fp32 MFMA, input gradient bf16x6     */
int32_t xt_last_launch_arith(void);

/* kernel-time probe: average duration (ms) of `reps` back-to-back launches of ONE layer kernel of the bound
 * network on `stream`, measured with HIP events on that stream (bench.py's roofline, tools/layer_bench.py). */
int xt_net_time_layer(xt_net* net, int32_t layer, int32_t which /* 0 fwd, 1 wgrad, 2 dgrad, 3 fused dgrad+wgrad */,
                      const void* obs, const int32_t* idx, int32_t B, int32_t reps,
                      float* ms_out, void* stream);

/* kernel-time probe of the SGD step's TAIL (ABI >= 11): average duration (ms, HIP events on `stream`) of `reps` back-to-back
 * repetitions of what follows the backward pass -- gradient reduction, [data parallel: exchange], global-norm clip + Adam --
 * in the net's CURRENT mode (plain; exchange hook; xt_net_set_dp + xt_net_set_direct: the fused three-launch chain), on the
 * weight-gradient slabs the most recent gradient step left in the workspace (parameters and slots ARE updated).  N processes
 * running it at the same time on one device give the kernel-side cost of the exchange per rank (tools/direct_probe.py). */
int xt_net_time_tail(xt_net* net, float lr, float clip_norm, int32_t reps, float* ms_out, void* stream);

/* xt_layer_fwd that reports the branch its dispatcher took, stand-alone for tests (appended; the ABI version stays).
 *   relu_mask    NULL, or [B*OH*OW] words for the first layer's relu sign mask (bit n of word p = y[p,n] > 0); only the
 *                flattened first-layer forward writes it, and only when the activation is relu
 *   mask_written NULL, or receives 1 when the mask was written, else 0
 * *path_out (may be NULL) receives XT_FWD_PATH_* | tile << XT_FWD_TILE_SHIFT | nst << XT_FWD_NST_SHIFT |
 * xcd << XT_FWD_XCD_SHIFT | XT_ARITH_* << XT_FWD_ARITH_SHIFT | units << XT_FWD_UNITS_SHIFT | ksplit << XT_FWD_KSPLIT_SHIFT:
 *   tile    XT_FWD_TILE_* (0 for the first-layer kernels)
 *   nst     steps per wave group the all-loads-up-front instance holds in flight (4 / 5 / 8), else 0
 *   xcd     1 when the blocks run in the XCD-chunked order (LDS-tiled forms only)
 *   units   LDS-tiled: wave groups per block (1 / 2 / 4); first-layer per frame stack: waves per block (4 / 8);
 *           first-layer flattened and SAME: output positions per workgroup (256 / 512); register-direct: waves per block
 *   ksplit  the EFFECTIVE split-K count the launch ran with (1 = none; reported up to 127) */
#define XT_FWD_PATH_C1_FLAT 1        /* uint8 first layer, VALID 8-wide kernel, 32 filters: positions flattened over the batch */
#define XT_FWD_PATH_C1_STACK 2       /* ... one frame stack per workgroup                                            */
#define XT_FWD_PATH_C1_SAME 3        /* uint8 first layer, SAME 8x8/4 or 4x4/2, 16 filters                           */
#define XT_FWD_PATH_DIRECT 4         /* register-direct forward (no LDS operand tiles)                               */
#define XT_FWD_PATH_TILED_FP32 5     /* LDS-tiled, fp32 MFMA (also every uint8 layer the first-layer kernels refuse) */
#define XT_FWD_PATH_TILED_X6 6       /* LDS-tiled, bf16x6                                                            */
#define XT_FWD_PATH_TILED_X6_ALL 7   /* LDS-tiled, bf16x6, two wave groups with all loads up front (fwd_prefetch_all) */
#define XT_FWD_TILE_128X32 1
#define XT_FWD_TILE_64X64 2
#define XT_FWD_TILE_DIRECT_TJ1 3     /* register-direct, one 32-column tile per wave                                 */
#define XT_FWD_TILE_DIRECT_TJ2 4     /* ... two                                                                      */
#define XT_FWD_TILE_SHIFT 4          /* 3 bits  */
#define XT_FWD_NST_SHIFT 7           /* 4 bits  */
#define XT_FWD_XCD_SHIFT 11          /* 1 bit   */
#define XT_FWD_ARITH_SHIFT 12        /* 2 bits  */
#define XT_FWD_UNITS_SHIFT 14        /* 10 bits */
#define XT_FWD_KSPLIT_SHIFT 24       /* 7 bits  */
int xt_layer_fwd_ex(const xt_conv_geom* g, const xt_input_xform* xf, int32_t B, const void* in, const int32_t* idx,
                    const float* w, const float* bias, float* y, float* partial, int32_t ksplit, void* stream,
                    uint32_t* relu_mask, int32_t* mask_written, int32_t* path_out);
/* xt_layer_fwd of the uint8 first layer g0 and of the 4x4/2 VALID 32 -> 32 layer g1 behind it as ONE launch
 * (conv12_u8_valid_fwd_flat_kernel, see xt_net_set_fwd_fuse12_flat; appended, the ABI version stays): act1 / relu_mask
 * (may be null; written when g0's activation is relu) / act2 receive what the two xt_layer_fwd calls (ksplit 1) write,
 * bit for bit.  rows_per_block: rows of g1's output (over all samples) per workgroup, 1..12; 0 = as the network splits
 * them (evenly over 256 workgroups, more once that exceeds 12 rows each).  Refused when the layers, the batch or
 * rows_per_block are outside the kernel's envelope. */
int xt_conv12_valid_fwd(const xt_conv_geom* g0, const xt_input_xform* xf, const xt_conv_geom* g1, int32_t B,
                        const void* in, const int32_t* idx, const float* w0, const float* b0, float* act1,
                        uint32_t* relu_mask, const float* w1, const float* b1, float* act2, int32_t rows_per_block,
                        void* stream);
/* The same with the 3x3/1 VALID 32 -> 64 layer g2 behind g1, three layers in ONE launch
 * (conv123_u8_valid_fwd_flat_kernel, see xt_net_set_fwd_fuse123_flat; appended, the ABI version stays): act1 / relu_mask /
 * act2 receive what xt_conv12_valid_fwd writes and act3 what xt_layer_fwd (ksplit 1) of g2 writes from that act2, bit for
 * bit.  rows_per_block: rows of g2's output (over all samples) per workgroup; 0 = the automatic split (groups of whole
 * samples cut into equal runs, one workgroup per CU while the batch allows).  Refused when the layers, the batch or
 * rows_per_block are outside the kernel's envelope (a workgroup holds 64 positions of g2's output, 128 of g1's and 768 of
 * g0's, within 160 KB of LDS: at 84x84 frames runs of up to 8 rows, or 9 that touch two samples). */
int xt_conv123_valid_fwd(const xt_conv_geom* g0, const xt_input_xform* xf, const xt_conv_geom* g1, const xt_conv_geom* g2,
                         int32_t B, const void* in, const int32_t* idx, const float* w0, const float* b0, float* act1,
                         uint32_t* relu_mask, const float* w1, const float* b1, float* act2, const float* w2, const float* b2,
                         float* act3, int32_t rows_per_block, void* stream);
/* The envelope and the split of xt_conv123_valid_fwd as host words (no device call): out[0 .. XT_CONV123_PLAN_WORDS), then
 * XT_CONV123_BLOCK_WORDS per workgroup while `cap` words last.  INSIDE = 1 when xt_conv123_valid_fwd would launch (all
 * other words but LDS_LIMIT are 0 when not); IN_NET = 1 when a network with the switch on takes the launch at this batch;
 * BLOCKS; GROUP_ROWS / GROUP_BLOCKS = the rows of g2's output are cut into groups of GROUP_ROWS, each into GROUP_BLOCKS
 * equal runs; LDS_BYTES of the launch and the LDS_LIMIT it is held to; MAX_CONV1_POS / MAX_CONV2_POS = positions of g0's /
 * g1's output the largest workgroup computes.  Per workgroup: the rows [0], [1]) of g2's output it owns, the rows [2], [3])
 * of g1's output it computes (both over all samples), its first sample, the positions of g0's output it computes, then
 * for each of its three sample pieces {rows of g1's output, first row of g0's output (it computes 2 n + 2 from there), 1
 * when the piece ends its sample}. */
enum {
  XT_CONV123_PLAN_INSIDE = 0, XT_CONV123_PLAN_IN_NET = 1, XT_CONV123_PLAN_BLOCKS = 2, XT_CONV123_PLAN_GROUP_ROWS = 3,
  XT_CONV123_PLAN_GROUP_BLOCKS = 4, XT_CONV123_PLAN_LDS_BYTES = 5, XT_CONV123_PLAN_LDS_LIMIT = 6,
  XT_CONV123_PLAN_MAX_CONV1_POS = 7, XT_CONV123_PLAN_MAX_CONV2_POS = 8, XT_CONV123_PLAN_WORDS = 9,
  XT_CONV123_BLOCK_WORDS = 15
};
int xt_conv123_valid_plan(const xt_conv_geom* g0, const xt_input_xform* xf, const xt_conv_geom* g1, const xt_conv_geom* g2,
                          int32_t B, int32_t rows_per_block, int32_t* out, int32_t cap);

/* xt_layer_wgrad the way a network's update runs it (appended; the ABI version stays): the gradient is left in slabs
 * (no reduction inside the launcher) and the slab buffer has `slab_cap` slabs, which is what lets the uint8 first-layer
 * kernels in; more than one slab is then summed into dwb by the slab-reduction kernel, as xt_layer_bwd does.
 * msplit > slab_cap is refused.
 * *path_out (may be NULL) receives XT_WG1_PATH_* | XT_ARITH_* << XT_WG1_ARITH_SHIFT | units << XT_WG1_UNITS_SHIFT |
 * slabs << XT_WG1_SLABS_SHIFT: units = waves per block (per frame stack: 4 / 8) or positions per workgroup (flattened
 * and SAME: 256 / 512), 0 for the generic kernel; slabs = the number of slabs written (1: dwb was written directly) */
#define XT_WG1_PATH_C1_FLAT 1        /* uint8 first layer, VALID 8x8, 32 filters: 512 positions per workgroup        */
#define XT_WG1_PATH_C1_STACK 2       /* ... one frame stack per workgroup                                            */
#define XT_WG1_PATH_C1_SAME 3        /* uint8 first layer, SAME 8x8/4 or 4x4/2, 16 filters                           */
#define XT_WG1_PATH_GENERIC 4        /* LDS-tiled fp32 weight gradient                                               */
#define XT_WG1_ARITH_SHIFT 4         /* 2 bits  */
#define XT_WG1_UNITS_SHIFT 6         /* 10 bits */
#define XT_WG1_SLABS_SHIFT 16        /* 15 bits */
int xt_layer_wgrad_slabs(const xt_conv_geom* g, const xt_input_xform* xf, int32_t B, const void* in, const int32_t* idx,
                         const float* dy, float* dwb, float* slabs, int32_t slab_cap, int32_t msplit, void* stream,
                         int32_t* path_out);

/* Model.predict on the device (appended; the ABI version stays): the trunk, then ONE head launch that leaves logits and
 * value exactly as xt_net_forward does (bit for bit) and adds the sampled action and its log-probability.
 *   Categorical   action = first argmax_a (logits[a] + g[a]) in float32, g = injected noise or -log(-log(u));
 *                 logp = log_softmax(logits)[action] by the expressions and summation order of xt_ppo_loss
 *   DiagGaussian  action[a] = mean[a] + exp(pi_logstd[a]) * eps[a], eps = injected noise or Box-Muller;
 *                 logp = the log-density of the stored action by the expressions of xt_ppo_loss_gauss
 * so a loss kernel fed these outputs on unchanged weights computes ratio == 1 exactly.
 * Generator: Philox4x32-10, key = (seed low, seed high), counter = (row0 + b, j, call low, call high), word w ->
 * u = (float(w >> 9) + 0.5) * 2^-23 in [2^-24, 1 - 2^-24].  Categorical: action a draws word a & 3 of block j = a >> 2;
 * DiagGaussian: dimension a draws words 2(a & 1) and 2(a & 1) + 1 of block j = a >> 1 as u1, u2 and
 * eps = sqrt(-2 log u1) * cos(2 pi u2).  A row's draw depends on (seed, call, row0 + b, a) only.  action_dim <= 64. */
typedef struct xt_act_cfg {
  uint64_t seed, call;   /* the generator's key; the caller's running predict count                       */
  int64_t row0;          /* index of this call's first row in the whole predict batch (chunked callers)   */
  int32_t want_noise;    /* != 0: noise_out receives the noise each action was drawn with                 */
} xt_act_cfg;
int xt_net_act(xt_net* net, const xt_act_cfg* cfg, const void* obs, const int32_t* idx, int32_t B,
               const float* noise /* [B,A] or NULL */, void* action /* int32 [B] | float32 [B,A], see XT_ACTION_* */,
               float* logp /* [B] */, float* value /* [B] */, float* logits /* [B,A] */,
               float* noise_out /* [B,A]; NULL unless cfg->want_noise */, void* stream);
/* the head launch of xt_net_act alone, on given features and head weights like xt_heads_fwd (kernel tests);
 * log_std: pi_logstd [A] for DiagGaussian, NULL for Categorical */
int xt_act_heads(const float* f_pi, const float* f_v, int32_t B, int32_t F, int32_t A, const float* wpi,
                 const float* bpi, const float* wv, const float* bv, const float* log_std, const xt_act_cfg* cfg,
                 const float* noise, void* action, float* logp, float* value, float* logits, float* noise_out,
                 void* stream);

/* The fused head launches of xt_net_ppo_step / xt_net_impala_step stand-alone, on given buffers, for kernel tests
 * (appended; the ABI version stays).  Each entry fills the argument struct the step fills and calls the step's launcher.
 * *path_out (may be NULL) receives the kernel instance(s) taken: XT_HEAD_PATH_* | nq << XT_HEAD_NQ_SHIFT |
 * part << XT_HEAD_PART_SHIFT | shared << XT_HEAD_SHARED_SHIFT | am << XT_HEAD_AM_SHIFT, 0 when nothing was launched:
 *   nq      features per lane of the sample's wave: 1 / 2 / 4 / 8 for ceil(F / 64) <= 1 / 2 / 4 / 8
 *   part    1 when the kernel sums split-K partial slabs, adds the trunk bias and applies the feature activation
 *   shared  PPO: 1 for one trunk under both heads
 *   am      IMPALA: actions the v-trace kernel holds in registers, 8 (A <= 8) or 32 */
#define XT_HEAD_PATH_PPO_FUSED 1     /* ppo_heads_fused_kernel<nq, part, shared>                                      */
#define XT_HEAD_PATH_IMPALA 2        /* impala_heads_fwd_kernel<nq, part> (nq = 0: not run), impala_vtrace_bwd_kernel<am> */
#define XT_HEAD_NQ_SHIFT 4           /* 4 bits  */
#define XT_HEAD_PART_SHIFT 8         /* 1 bit   */
#define XT_HEAD_SHARED_SHIFT 9       /* 1 bit   */
#define XT_HEAD_AM_SHIFT 10          /* 6 bits  */
/* Heads forward + PPO loss + d(logits, value) + d(features), one launch.
 *   f_pi, f_v       features [B,F] (shared: f_v is not read); not read when part_pi is given
 *   part_pi, part_v NULL, or ksplit_pi / ksplit_v partial slabs [ksplit][part_stride floats] of the last trunk layer:
 *                   feature = act_feat(sum of the slabs + tbias), also written to feat_pi_w / feat_v_w [B,F]
 *                   (shared: part_v, tbias_v, feat_v_w and ksplit_v are not read)
 *   idx             NULL, or [B] rows of the label pools action / old_logp / adv / old_v / target_v
 *   cfg             clip_ratio, ent_coef, vf_clip and critic_coef are read
 *   terms [B,4]     per sample: min(surr1, surr2), entropy, max(vf1, vf2), 0
 *   df_pi, df_v     d(features) times the derivative of act_prev at the feature (shared: df_v is not written)
 * Refused (before any device call): A > 8, F > 512, more than 16 slabs. */
int xt_ppo_heads_fused_ex(const float* f_pi, const float* f_v, const float* part_pi, const float* part_v,
                          int32_t ksplit_pi, int32_t ksplit_v, int64_t part_stride, const float* tbias_pi,
                          const float* tbias_v, int32_t act_feat, int32_t B, int32_t F, int32_t A, int32_t shared,
                          const float* wpi, const float* bpi, const float* wv, const float* bv, const int32_t* idx,
                          const int32_t* action, const float* old_logp, const double* adv, const float* old_v,
                          const double* target_v, const xt_ppo_cfg* cfg, float inv_b, int32_t act_prev, float* logits,
                          float* value, float* dlogits, float* dvalue, float* terms, float* df_pi, float* df_v,
                          float* feat_pi_w, float* feat_v_w, void* stream, int32_t* path_out);
/* The same launch for a DiagGaussian policy (appended under ABI 12): ppo_gauss_heads_fused_kernel<nq, part, shared>, the
 * head launch of a net with xt_net_set_gauss_fused(net, 1).  As xt_ppo_heads_fused_ex, except
 *   log_std         pi_logstd [A]
 *   action          [pool, A] float32 rows, picked through idx like the other labels
 *   mean, dmean     [B,A] (the categorical entry's logits / dlogits)
 *   dls_rows        [B][ldls] (ldls >= A): every sample's share of d loss / d pi_logstd, columns < A written
 *   rows            NULL, or [B,4] floats (16-byte aligned): the diagnostic rows of xt_net_set_train_stats, written by the
 *                   STATS instances
 * *path_out = XT_HEAD_PATH_PPO_GAUSS_FUSED | nq | part | shared.  Refused (before any device call): A > 8, F > 512, more
 * than 16 slabs. */
#define XT_HEAD_PATH_PPO_GAUSS_FUSED (4) /* ppo_gauss_heads_fused_kernel<nq, part, shared>; its case table is
                                          * tests/test_gpu_gauss_heads.py (the plain-integer XT_HEAD_PATH_* macros above are
                                          * the families whose tables tests/test_gpu_heads_branch.py holds) */
int xt_ppo_gauss_heads_fused_ex(const float* f_pi, const float* f_v, const float* part_pi, const float* part_v,
                                int32_t ksplit_pi, int32_t ksplit_v, int64_t part_stride, const float* tbias_pi,
                                const float* tbias_v, int32_t act_feat, int32_t B, int32_t F, int32_t A, int32_t shared,
                                const float* wpi, const float* bpi, const float* wv, const float* bv,
                                const float* log_std, const int32_t* idx, const float* action, const float* old_logp,
                                const double* adv, const float* old_v, const double* target_v, const xt_ppo_cfg* cfg,
                                float inv_b, int32_t act_prev, float* mean, float* value, float* dmean, float* dvalue,
                                float* dls_rows, int32_t ldls, float* terms, float* df_pi, float* df_v,
                                float* feat_pi_w, float* feat_v_w, float* rows, void* stream, int32_t* path_out);
/* IMPALA (one trunk): heads forward, then v-trace + loss + d(logits, baseline) + d(features), then the loss sum.
 *   run_fwd         1: logits / baseline [n_traj*T (,A)] are computed from feat [n_traj*T,F], or from `ksplit` partial
 *                   slabs as above (the finished features go to feat_w, which the second launch reads);
 *                   0: logits / baseline are inputs and feat is given -- the forward kernel holds A <= 8, the v-trace
 *                   kernel A <= 32
 *   vs, pg_adv      [n_traj, T-1], each may be NULL;  traj_loss [n_traj];  loss_out [1] their sum
 * Refused (before any device call): T > 256, A > 32; with run_fwd also A > 8, F > 512, more than 16 slabs. */
int xt_impala_heads_ex(const float* feat, const float* part, int32_t ksplit, int64_t part_stride, const float* tbias,
                       int32_t act_feat, int32_t run_fwd, int32_t n_traj, int32_t T, int32_t F, int32_t A,
                       const float* wpi, const float* bpi, const float* wv, const float* bv, const float* bp_logits,
                       const int32_t* action, const uint8_t* done, const float* reward, float gamma, int32_t act_prev,
                       float* feat_w, float* logits, float* baseline, float* dlogits, float* dbaseline, float* vs,
                       float* pg_adv, float* dfeat, float* traj_loss, float* loss_out, void* stream, int32_t* path_out);
/* Head weight-gradient partial slabs as every step writes them: chunk c of 8 samples leaves its share of
 * [dWpi (F*A) | dbpi (A)] at slab_pi + c * stride_pi and of [dWv (F) | dbv (1)] at slab_v + c * stride_v (strides in
 * floats); *nchunk_out = ceil(B / 8) slabs are written, for the caller (the gradient-reduction launch) to sum. */
int xt_heads_wgrad_partial_ex(const float* f_pi, const float* f_v, int32_t B, int32_t F, int32_t A,
                              const float* dlogits, const float* dvalue, float* slab_pi, int64_t stride_pi,
                              float* slab_v, int64_t stride_v, int32_t* nchunk_out, void* stream);

/* Per-train IMPALA v-trace diagnostics (ImpalaCnnOpt's path: xt_net_impala_step / xt_net_impala_train / _train_io),
 * accumulated on the device inside the train's own launches (appended under ABI 12; opt-in).  `stats`:
 * XT_IMPALA_STATS_DOUBLES doubles (8-byte aligned), `traj_stats`: [max_traj, XT_IMPALA_TRAJ_STATS_FLOATS] floats of scratch
 * (16-byte aligned), both device memory owned by the caller; xt_net_workspace_bytes does not change.  NULL, NULL switches
 * the diagnostics off (the default): every launch is then the one of a net that never had them.  Refused on a net with a
 * data-parallel tail, a gradient exchange hook or a direct comm (the row statistics would be rank-local), and
 * xt_net_set_dp / xt_net_set_grad_exchange are refused while they are on.
 *
 * With the buffers set, the v-trace / loss kernel of every chunk is its STATS instance: the lead workgroup of a trajectory
 * also leaves one row of traj_stats -- per column a float sum over the transitions t < T - 1 (wave sums, then the waves in
 * wave order; never an atomic) of values the kernel holds anyway:
 *     column 0 ce * pg   1 entropy   2 (vs - v)^2   3 vs - v   4 vs   5 vs^2   6 blp - tlp (= -log rho)   7 rho
 *            8 [rho > 1] (the transitions the rho_bar = c_bar = 1 clip cuts)   9 max rho (a maximum)   10 T - 1   11 0
 * (tlp / blp: log-probability of the taken action under the target / behaviour logits).  Wherever the chunk's loss scalar
 * is formed -- the extra block of the gradient-reduction launch, or the loss-reduce launch of the unfused heads and of a
 * gradient-only step -- one thread per column adds the rows in trajectory order, in double, to the slots below, and the
 * thread that writes the pre-clip global norm into adam_state[4] (Adam, its folded-IO instance, centred RMSProp, the fused
 * and the ticket tail) adds the norm.  One fixed order everywhere: a replayed hipGraph and the eager call give the same
 * bits.  xt_net_impala_train(_io) clears the block at its start with a kernel inside the graph; xt_net_impala_step only
 * accumulates (its caller clears), and with apply == 0 it leaves the three gradient-norm slots alone.  The pointers are part
 * of the IMPALA trains' hipGraph key.  max_traj: rows of traj_stats; a chunk with more trajectories is refused. */
#define XT_IMPALA_STATS_DOUBLES 16
#define XT_IMPALA_TRAJ_STATS_FLOATS 12
#define XT_IMPALA_STATS_CHUNKS 0         /* chunks (optimiser steps)                                          */
#define XT_IMPALA_STATS_TRANSITIONS 1    /* transitions that carry loss: trajectories x (T - 1)               */
#define XT_IMPALA_STATS_PG 2             /* sum of ce * pg_advantage (the policy-gradient piece of the loss)  */
#define XT_IMPALA_STATS_ENT 3            /* ... entropy of the target policy                                  */
#define XT_IMPALA_STATS_VERR_SQ 4        /* ... (vs - v)^2                                                    */
#define XT_IMPALA_STATS_VERR 5           /* ... vs - v                                                        */
#define XT_IMPALA_STATS_VS 6             /* ... vs                                                            */
#define XT_IMPALA_STATS_VS_SQ 7          /* ... vs^2                                                          */
#define XT_IMPALA_STATS_NEG_LOG_RHO 8    /* ... blp - tlp: KL(behaviour || target) on behaviour samples       */
#define XT_IMPALA_STATS_RHO 9            /* ... rho = exp(tlp - blp)                                          */
#define XT_IMPALA_STATS_RHO_CLIPPED 10   /* transitions with rho > 1                                          */
#define XT_IMPALA_STATS_RHO_MAX 11       /* largest rho (a maximum)                                           */
#define XT_IMPALA_STATS_GNORM_SUM 12     /* sum over chunks of the pre-clip global gradient norm              */
#define XT_IMPALA_STATS_GNORM_MAX 13     /* its maximum                                                       */
#define XT_IMPALA_STATS_GNORM_CLIPPED 14 /* chunks with the norm above grad_norm_clip                         */
#define XT_IMPALA_STATS_RESERVED 15      /* 0                                                                 */
int xt_net_set_impala_stats(xt_net* net, double* stats, float* traj_stats, int32_t max_traj);
/* xt_impala_heads_ex / xt_impala_loss through the STATS instances, for kernel tests: the same arguments and launchers, plus
 * traj_stats [n_traj, XT_IMPALA_TRAJ_STATS_FLOATS] (16-byte aligned) and stats [XT_IMPALA_STATS_DOUBLES], which the loss-reduce
 * launch ADDS to (the caller clears; the gradient-norm slots are not touched).  The instance is recorded as the existing
 * entries record theirs: *path_out of xt_impala_heads_stats_ex carries XT_IMPALA_PATH_STATS_BIT on top of
 * xt_impala_heads_ex's word; xt_impala_loss_stats returns through *path_out (may be NULL)
 *     XT_IMPALA_PATH_LOSS | (MAXT / 64) << XT_HEAD_AM_SHIFT | XT_IMPALA_PATH_STATS_BIT
 * for impala_loss_kernel<MAXT, true>, MAXT = 64 / 128 / 256 / 1024 (the smallest that holds T).  xt_net_last_head_path
 * returns the same words (without the bit when the statistics are off) after an IMPALA step. */
#define XT_IMPALA_PATH_LOSS 3
#define XT_IMPALA_PATH_STATS_BIT 0x10000
int xt_impala_heads_stats_ex(const float* feat, const float* part, int32_t ksplit, int64_t part_stride, const float* tbias,
                             int32_t act_feat, int32_t run_fwd, int32_t n_traj, int32_t T, int32_t F, int32_t A,
                             const float* wpi, const float* bpi, const float* wv, const float* bv, const float* bp_logits,
                             const int32_t* action, const uint8_t* done, const float* reward, float gamma, int32_t act_prev,
                             float* feat_w, float* logits, float* baseline, float* dlogits, float* dbaseline, float* vs,
                             float* pg_adv, float* dfeat, float* traj_loss, float* loss_out, void* stream, int32_t* path_out,
                             float* traj_stats, double* stats);
int xt_impala_loss_stats(const float* logits, const float* baseline, const float* bp_logits,
                         const int32_t* action, const uint8_t* done, const float* reward,
                         int32_t n_traj, int32_t T, int32_t A, float gamma,
                         float* dlogits, float* dbaseline, float* out, float* acc,
                         float* vs, float* pg_adv, void* stream, float* traj_stats, double* stats, int32_t* path_out);

/* ------------------------------------------------------------------ DQN (appended under ABI 12)
 * The replay store lives in HBM as rings [capacity, row] (xt/algorithm/replay_buffer.py holds a host deque); a train
 * gathers its minibatch out of them on the device.
 *
 * xt_replay_gather: dst[b] = ring[slots[b]] for b < B; ring [capacity, row_bytes], dst [B, row_bytes], slots int32 [B] on
 * the device.  Rows are stored in the form the first layer reads (channel-padded images, feature-padded vectors), so
 * row_bytes is a multiple of 16: anything else is refused.  16-byte loads and stores; slot * row_bytes is 64-bit
 * arithmetic (the ring may be larger than 4 GB).  ring and dst 16-byte aligned.  A slot outside [0, capacity) is not
 * read: its row of dst is zero. */
int xt_replay_gather(const void* ring, int64_t row_bytes, int64_t capacity, const int32_t* slots, int32_t B, void* dst,
                     void* stream);

/* TD target and MSE head of DQN.train (xt/algorithm/dqn/dqn.py:61-103) + Keras `loss='mse'` on labels that equal the
 * prediction except in the taken column.  Q from the heads: Q = logits [B,A], or with `dueling`
 * Q_a = value + (logits_a - mean_a logits) (value: the 1-wide head [B]).
 *     a*   = argmax_a Q_target(next)  (o_logits == NULL)  |  argmax_a Q_online(next)  (double DQN), first maximal index
 *     maxq = Q_target(next)[a*]
 *     y    = done ? (float)r : (float)(r + gamma * (double)maxq)          (r float64, one rounding)
 *     L    = sum_b (Q_{b,a_b} - y_b)^2 / (B A);   g_b = 2 (Q_{b,a_b} - y_b) / (B A)
 *     dueling: dlogits_{b,j} = g_b (1[j = a_b] - 1/A), dvalue_b = g_b;   else dlogits_{b,j} = g_b 1[j = a_b], dvalue_b = 0
 * logits / value: online heads on the states; t_*: target-net heads on the next states; o_* (may be NULL): online heads
 * on the next states.  The value pointers are read only with `dueling`.  slots (may be NULL: rows 0..B-1) gathers
 * action int32 [N], reward float64 [N], done uint8 [N] (truthiness) from the label rings; an action outside [0, A) is
 * clamped into it.  out: >= 4 + 2*B floats, 8-byte aligned; out[0] = L, out[1] = mean_b |Q_{b,a_b} - y_b|,
 * out[2] = mean_b maxq_b, the rest is scratch (sums in double, fixed order).  y [B], astar [B], maxq [B] (each may be
 * NULL): the per-row target, bootstrap action and bootstrap value.  acc (may be NULL): acc[0] += L, acc[1] += 1.
 * One thread per sample plus a one-block reduction.  A <= 64. */
int xt_dqn_loss(const float* logits, const float* value, const float* t_logits, const float* t_value,
                const float* o_logits, const float* o_value, int32_t B, int32_t A, int32_t dueling, const int32_t* slots,
                const int32_t* action, const double* reward, const uint8_t* done, double gamma, float* dlogits,
                float* dvalue, float* out, float* y, int32_t* astar, float* maxq, float* acc, void* stream);

/* One DQN.train up to the gradient, in ONE call that never synchronises.  Enqueued in order: gather of the next-state
 * rows; target_net forward on them, its heads copied to q_scratch; double DQN only: net forward on them, copied too; gather
 * of the state rows; net training forward; xt_dqn_loss; backward through the heads and the trunk; gradient reduction.  The
 * flat gradient is left in net's gradient buffer for xt_adam_keras, as xt_net_keras_impala_step leaves it.
 * target_net: a second net of the same description bound to its own parameter buffer and workspace (forward only).
 * cur_ring / next_ring [capacity, row_bytes] with row_bytes = the first layer's input row; action / reward / done: the
 * label rings [capacity]; slots int32 [B] on the device.  loss_out (may be NULL): 3 floats, out[0..2] of xt_dqn_loss.
 * Categorical nets, A <= 64; refused while a gradient exchange or the data-parallel tail is installed. */
typedef struct xt_dqn_cfg {
  double gamma;
  int32_t dueling;              /* Q = value + (logits - mean logits)                                       */
  int32_t double_dqn;           /* the online net picks the bootstrap action                                */
  void* cur_rows;               /* scratch [B, row_bytes], 16-byte aligned: the gathered state rows         */
  void* next_rows;              /* scratch [B, row_bytes], 16-byte aligned: the gathered next-state rows    */
  float* q_scratch;             /* scratch >= 2 * B * (A + 1) floats: the copied heads of the next states   */
} xt_dqn_cfg;
int xt_net_dqn_step(xt_net* net, xt_net* target_net, const xt_dqn_cfg* cfg, const void* cur_ring, const void* next_ring,
                    int64_t row_bytes, int64_t capacity, const int32_t* slots, int32_t B, const int32_t* action,
                    const double* reward, const uint8_t* done, float* loss_out, float* loss_acc, void* stream);

/* ------------------------------------------------------------------ DQN: prioritised replay (appended under ABI 12)
 * xt/algorithm/prioritized_replay_buffer_muzero.py::PrioritizedReplayBuffer on xt/algorithm/segment_tree.py, kept on the
 * device: a sum tree (neutral element 0) and a min tree (neutral element +inf) of 2 * cap2 float64 nodes each, cap2 the
 * smallest power of two >= the ring's capacity; node i = op(node 2i, node 2i + 1), leaf cap2 + slot belongs to ring slot
 * `slot` (the reference's _next_idx is the ring's write position).  max_prio: one float64 on the device, 1.0 at the
 * start.  Every entry enqueues ONE workgroup on `stream` and never synchronises; the levels are walked with a barrier
 * between them, so a node is recomputed from final children and the trees are bit for bit what the reference's
 * sequential __setitem__ calls leave.
 *
 * xt_per_add: leaves [first, first + count) <- pow(*max_prio, alpha) in both trees (*max_prio read on the device), then
 * their ancestors.  A message that wraps the ring is two calls.  256 threads stride over each level's node range. */
int xt_per_add(double* sum, double* min, int64_t cap2, const double* max_prio, int64_t first, int64_t count, double alpha,
               void* stream);

/* PrioritizedReplayBuffer.sample(B, beta) on `size` stored transitions, one thread per sample (B <= 1024):
 *     p_total = v[L1] + (v[L2] + (... + v[Lk]))   over the maximal left subtrees on the way down to leaf size - 2 (the
 *               reference's sum(0, size - 1) leaves the LAST stored slot outside the mass range: kept)
 *     every   = p_total / B;   mass_b = u_b * every + b * every          (two roundings per product and sum, no fma)
 *     idx_b   = find_prefixsum_idx(mass_b): at each level left iff sum[2i] > mass, else mass -= sum[2i] and right
 *     p_min   = max(min[1] / sum[1], 1e-5);   max_w = (p_min * size) ** (-beta)
 *     w_b     = (leaf[idx_b] / sum[1] * size) ** (-beta) / max_w
 * u float64 [B] on the device (the caller's uniform draws in [0, 1)); slots_out int32 [B]; weights_out float64 [B].
 * A descent that ends at a leaf >= size is clamped to size - 1 (the reference raises an IndexError there).  size < 2 is
 * refused: the reference recurses without end. */
int xt_per_sample(const double* sum, const double* min, int64_t cap2, int64_t size, const double* u, int32_t B, double beta,
                  int32_t* slots_out, double* weights_out, void* stream);

/* PrioritizedReplayBuffer.update_priorities(slots, |delta| + eps), one thread per sample (B <= 1024):
 * priority_b = (double)|delta[b * delta_stride]| + eps; leaf slots[b] <- priority_b ** alpha in both trees -- of equal
 * slots the largest b wins, as the reference's batch order leaves it (resolved in LDS before the leaf stores) --
 * *max_prio = max(*max_prio, every priority_b), then the ancestors.  delta float32 with a stride in elements (2 reads
 * terms[b].x of xt_dqn_loss in place); a slot outside [0, cap2) is not stored through.  eps > 0. */
int xt_per_update(double* sum, double* min, int64_t cap2, double* max_prio, const int32_t* slots, const float* delta,
                  int64_t delta_stride, int32_t B, double eps, double alpha, void* stream);

/* xt_dqn_loss with importance weights (Keras train_on_batch(..., sample_weight=w) with 'mse'): weights float64 [B] on the
 * device, each rounded once to float32;  L = sum_b w_b delta_b^2 / (B A),  g_b = 2 w_b delta_b / (B A);  out[1], out[2],
 * y, astar, maxq and the scratch terms (delta_b, maxq_b) at out + 4 are unweighted.  weights == NULL is xt_dqn_loss bit
 * for bit (xt_dqn_loss calls this entry with NULL). */
int xt_dqn_loss_w(const float* logits, const float* value, const float* t_logits, const float* t_value,
                  const float* o_logits, const float* o_value, int32_t B, int32_t A, int32_t dueling, const int32_t* slots,
                  const int32_t* action, const double* reward, const uint8_t* done, double gamma, float* dlogits,
                  float* dvalue, float* out, float* y, int32_t* astar, float* maxq, float* acc, const double* weights,
                  void* stream);

/* One prioritised DQN.train up to the gradient, in ONE call that never synchronises.  After the refusals of
 * xt_net_dqn_step (the same ones, data parallelism included) it enqueues, in order: xt_per_sample on `size` stored
 * transitions into cfg->slots / cfg->weights; the chain of xt_net_dqn_step on those slots with the weighted head
 * (xt_dqn_loss_w); xt_per_update on the TD errors the head left.  size <= capacity <= cap2. */
typedef struct xt_per_cfg {
  double* sum;                  /* sum tree [2 * cap2]                                                      */
  double* min;                  /* min tree [2 * cap2]                                                      */
  int64_t cap2;
  double* max_prio;             /* the running maximum priority (one float64)                               */
  const double* u;              /* [B] uniform draws in [0, 1)                                              */
  int32_t* slots;               /* scratch [B]: the sampled ring slots                                      */
  double* weights;              /* scratch [B]: their importance weights                                    */
  float* terms_out;             /* may be NULL; [2 * B]: copy of (delta_b, maxq_b) the update read          */
  double alpha, beta, eps;
} xt_per_cfg;
int xt_net_dqn_step_per(xt_net* net, xt_net* target_net, const xt_dqn_cfg* cfg, const xt_per_cfg* per, const void* cur_ring,
                        const void* next_ring, int64_t row_bytes, int64_t capacity, int64_t size, int32_t B,
                        const int32_t* action, const double* reward, const uint8_t* done, float* loss_out, float* loss_acc,
                        void* stream);

/* ------------------------------------------------------------------ DQN: n-step returns (appended under ABI 12)
 * The learner holds every message's rows in time order in the rings, so the m-step target of a sampled row is formed on
 * the device inside the next-state gather.  follow int32 [capacity]: follow[s] = the number of rows that come after slot s
 * in the message that wrote it (a negative value counts as 0).  For a start slot s (all float64; the product is rounded,
 * then the sum: no fma):
 *     R = reward[s]; g = gamma; j = s; k = 0
 *     while k < n - 1 and k < follow[s] and not done[j]:  k += 1; j = (s + k) % capacity; R = R + g * reward[j]; g = g * gamma
 *     boot_slot = j; reward_n = R; disc_n = g; done_n = done[j]; action_n = action[s]
 *     y = done_n ? (float)R : (float)(R + disc_n * (double)maxq)                 (maxq from next_ring[boot_slot])
 * n = 1 is (s, reward[s], gamma, done[s]): the one-step target bit for bit.  A walk that reaches the end of its message
 * stops there (a shorter target); rows behind s in its message are newer than s, so a live row only walks live rows.
 *
 * xt_replay_gather_nstep: xt_replay_gather (same grid, same refusals) with the walk in front: dst[b] =
 * next_ring[boot_slot_b], and the five labels of sample b go to boot_slots / action_n / reward_n / disc_n / done_n [B].
 * 1 <= n <= 256; action / reward / done / follow: the label rings [capacity].  A start slot outside [0, capacity) reads
 * nothing: a zero row, boot_slot = slot, action_n = 0, reward_n = 0, disc_n = gamma, done_n = 1. */
int xt_replay_gather_nstep(const void* next_ring, int64_t row_bytes, int64_t capacity, const int32_t* slots, int32_t B,
                           const int32_t* action, const double* reward, const uint8_t* done, const int32_t* follow,
                           int32_t n, double gamma, void* dst, int32_t* boot_slots, int32_t* action_n, double* reward_n,
                           double* disc_n, uint8_t* done_n, void* stream);

/* xt_dqn_loss_w with a per-sample discount: disc float64 [B] on the device (indexed by the sample, never through slots)
 * takes gamma's place, y_b = done ? (float)r : (float)(r + disc[b] * (double)maxq).  disc == NULL is xt_dqn_loss_w bit
 * for bit (xt_dqn_loss_w calls this entry with NULL). */
int xt_dqn_loss_n(const float* logits, const float* value, const float* t_logits, const float* t_value,
                  const float* o_logits, const float* o_value, int32_t B, int32_t A, int32_t dueling, const int32_t* slots,
                  const int32_t* action, const double* reward, const uint8_t* done, double gamma, float* dlogits,
                  float* dvalue, float* out, float* y, int32_t* astar, float* maxq, float* acc, const double* weights,
                  const double* disc, void* stream);

/* One DQN.train with n-step targets up to the gradient, uniform (per == NULL: `slots` int32 [B] on the device) or
 * prioritised (per set: `slots` is ignored, `size` stored transitions are sampled), in ONE call that never synchronises.
 * The refusals of xt_net_dqn_step(_per) in their order, then 1 <= ns->n <= 256 and non-null pointers in ns; then the chain
 * of xt_net_dqn_step(_per) with two changes: the first gather is xt_replay_gather_nstep, so both next-state forwards run
 * on the boot rows, and the head (xt_dqn_loss_n) reads the dense labels the gather left with disc = ns->disc_n.  The state
 * rows are gathered by the start slots and xt_per_update writes the new priorities to the start slots.  The launches
 * are those of the one-step chain in number; ns->n == 1 gives its loss, gradient and trees bit for bit. */
typedef struct xt_nstep_cfg {
  int32_t n;                    /* steps of the return, 1 <= n <= 256                                       */
  const int32_t* follow;        /* ring [capacity]: rows behind each slot in its message                    */
  int32_t* boot_slots;          /* scratch [B]: the slot whose next state bootstraps sample b               */
  int32_t* action_n;            /* scratch [B]: action[start slot]                                          */
  double* reward_n;             /* scratch [B]: the discounted reward sum                                   */
  double* disc_n;               /* scratch [B]: gamma ** (rows walked + 1)                                  */
  uint8_t* done_n;              /* scratch [B]: done[boot slot]                                             */
} xt_nstep_cfg;
int xt_net_dqn_step_n(xt_net* net, xt_net* target_net, const xt_dqn_cfg* cfg, const xt_nstep_cfg* ns,
                      const xt_per_cfg* per, const void* cur_ring, const void* next_ring, int64_t row_bytes,
                      int64_t capacity, int64_t size, const int32_t* slots, int32_t B, const int32_t* action,
                      const double* reward, const uint8_t* done, float* loss_out, float* loss_acc, void* stream);

/* ------------------------------------------------------------------ distributional (C51) Q head (appended under ABI 12)
 * Bellemare et al. 2017: the Q head is A * N wide, column a * N + i is the logit of atom i of action a, and the TD target
 * is a distribution projected onto the fixed support.  Definitions (host twins dist_support / dist_q /
 * categorical_projection of xingtian_amd/algorithm/dqn/dqn.py):
 *     delta = (v_max - v_min) / (N - 1), z_i = v_min + i * delta in float64; (float)z_i where float32 is used
 *     dist_q(l) = (sum_i z_i e_i) / (sum_i e_i), e_i = expf(l_i - max l), float32
 *     a* = first maximal index over a of dist_q of the picking logits (t_logits, or o_logits when given: double DQN)
 *     p_j = softmax(t_logits[a*, :])_j in float32;  (R, g, dn) = (reward, disc ? disc[b] : gamma, done) of the sample
 *     Tz_j = clamp(dn ? R : R + g * z_j, v_min, v_max);  b_j = (Tz_j - v_min) / delta              (float64)
 *     m_i = (float) sum_{j ascending} (double)p_j * max(0, 1 - |b_j - i|)                 (float64, one rounding)
 *     logq_i = (l_i - mx) - logf(sum_k expf(l_k - mx)) on the online logits l of the taken action (clamped into [0, A))
 *     loss_b = -sum_i m_i logq_i;  L = sum_b w_b loss_b / B  (w_b = (float)weights[b], 1 without weights)
 *     dlogits[b, act * N + i] = w_b (expf(logq_i) M_b - m_i) / B with M_b = sum_i m_i; every other entry 0; dvalue[b] = 0
 * The projection is Algorithm 1 of the paper in gather form: equal to its l/u scatter whenever no b_j is an integer, and
 * it keeps the mass the published pseudo-code drops when l == u.  No atomics: the result does not depend on thread order.
 * logits / t_logits / o_logits [B, A * N]; labels through `slots` (int32 [B]) or dense (slots == NULL); out: 4 + 2 B floats,
 * 8-byte aligned: out[0] = L, out[1] = sum_b loss_b / B, out[2] = sum_b dist_q_target(a*_b) / B and from out + 4 the
 * terms (loss_b, dist_q_target(a*_b)), where xt_per_update reads its |x|.  astar / maxq [B] / m [B, N] / acc / weights /
 * disc may be NULL.  Two launches.  Refused: atoms outside [2, 256], A outside [1, 64], v_min >= v_max or not finite. */
int xt_dqn_loss_dist(const float* logits, const float* t_logits, const float* o_logits, int32_t B, int32_t A, int32_t atoms,
                     double v_min, double v_max, const int32_t* slots, const int32_t* action, const double* reward,
                     const uint8_t* done, double gamma, float* dlogits, float* dvalue, float* out, int32_t* astar,
                     float* maxq, float* m, float* acc, const double* weights, const double* disc, void* stream);
/* Marks a net (per net, opt-in) as carrying a distributional head of `atoms` atoms on [v_min, v_max]: its action_dim is
 * actions * atoms.  atoms == 1 clears the mark.  Refused: atoms outside [1, 256], bounds as above, a width that is no
 * multiple of atoms, a DiagGaussian net.  A marked net is refused by xt_net_dqn_step / _per / _n. */
int xt_net_set_dist(xt_net* net, int32_t atoms, double v_min, double v_max);
/* The two head kernels of a marked net (on by default, re-armed by every xt_net_set_dist): heads_fwd_wide_kernel (one
 * thread per output column instead of one wave reduction per output) for every forward of the net, and in
 * xt_net_dqn_step_dist d(features) summed over the taken action's atoms only (bit-identical to the full sum).  on == 0:
 * the kernels of an unmarked net, for same-run comparisons; on == 2: the wide forward with heads_dfeat_kernel behind it, so
 * that a run can time a mark's d(features) kernel against the generic one under the same forward.  Refused on an unmarked
 * net. */
int xt_net_set_dist_wide(xt_net* net, int32_t on);
/* xt_net_dqn_step_n's chain (ns == NULL: one-step targets; per == NULL: uniform, `slots`) with xt_dqn_loss_dist as the
 * head, same launches in number.  Both nets must carry equal marks; cfg->dueling must be 0; actions <= 64; cfg->q_scratch
 * holds 2 * B * (actions * atoms + 1) floats.  With per, the new priority of a start slot is loss_b + eps. */
int xt_net_dqn_step_dist(xt_net* net, xt_net* target_net, const xt_dqn_cfg* cfg, const xt_nstep_cfg* ns,
                         const xt_per_cfg* per, const void* cur_ring, const void* next_ring, int64_t row_bytes,
                         int64_t capacity, int64_t size, const int32_t* slots, int32_t B, const int32_t* action,
                         const double* reward, const uint8_t* done, float* loss_out, float* loss_acc, void* stream);

/* ------------------------------------------------------------------ quantile-regression (QR-DQN) Q head (appended under ABI 12)
 * Dabney et al. 2018: the Q head is A * N wide, column a * N + i is quantile theta_i of action a at the midpoint tau_i;
 * there is no support and there are no bounds.  Definitions (host twins quantile_midpoints / quant_q /
 * quantile_huber of xingtian_amd/algorithm/dqn/dqn.py):
 *     tau_i = (2 i + 1) / (2 N)                                                                    (float64)
 *     quant_q(theta) = (float)((sum_{i ascending} (double)theta_i) / N)                            (one rounding)
 *     a* = first maximal index over a of quant_q of the picking quantiles (t_logits, or o_logits when given: double DQN)
 *     (R, g, dn) = (reward, disc ? disc[b] : gamma, done) of the sample
 *     T_j = (float)(dn ? R : R + g * (double)theta'_j), theta' = t_logits[a*, :]       (float64, no fma, one rounding)
 *     u_ij = T_j - theta_i in float32, theta = the online quantiles of the taken action (clamped into [0, A))
 *     wt_ij = u_ij < 0 ? (float)(1 - tau_i) : (float)tau_i
 *     H(u) = |u| <= kappa ? 0.5f u u : kappa (|u| - 0.5f kappa)                                    (float32)
 *     r_i = (float)((sum_{j ascending} (double)(wt_ij * H(u_ij) / kappa)) / N)
 *     g_i = (float)(-(sum_{j ascending} (double)(wt_ij * clamp(u_ij, -kappa, kappa) / kappa)) / N)
 *     loss_b = sum_i r_i;  L = sum_b w_b loss_b / B  (w_b = (float)weights[b], 1 without weights)
 *     dlogits[b, act * N + i] = w_b g_i / B; every other entry 0; dvalue[b] = 0
 * kappa (used as a float32) must be finite and > 0: loss and gradient are then continuous in u, at 0 and at |u| = kappa;
 * the pure |u| loss (kappa = 0) is not provided.  No atomics: the result does not depend on thread order.
 * logits / t_logits / o_logits [B, A * N]; labels through `slots` (int32 [B]) or dense (slots == NULL); out: 4 + 2 B floats,
 * 8-byte aligned: out[0] = L, out[1] = sum_b loss_b / B, out[2] = sum_b quant_q(theta'(a*_b)) / B and from out + 4 the
 * terms (loss_b, quant_q(theta'(a*_b))), where xt_per_update reads its |x|.  astar / maxq [B] / acc / weights / disc may
 * be NULL.  Two launches.  Refused: quantiles outside [2, 256], A outside [1, 64], kappa not finite or <= 0, a null
 * required pointer, a misaligned out. */
int xt_dqn_loss_quant(const float* logits, const float* t_logits, const float* o_logits, int32_t B, int32_t A,
                      int32_t quantiles, double kappa, const int32_t* slots, const int32_t* action, const double* reward,
                      const uint8_t* done, double gamma, float* dlogits, float* dvalue, float* out, int32_t* astar, float* maxq,
                      float* acc, const double* weights, const double* disc, void* stream);
/* The head a net is marked with: a net carries at most one mark, and both marks fill the same columns-per-action count. */
#define XT_HEAD_SCALAR 0
#define XT_HEAD_C51 1     /* xt_net_set_dist  */
#define XT_HEAD_QUANT 2   /* xt_net_set_quant */
/* Marks a net (per net, opt-in) as carrying a quantile head of `quantiles` quantiles with Huber threshold kappa: its
 * action_dim is actions * quantiles.  quantiles == 1 clears the mark.  Refused: quantiles outside [1, 256], kappa as
 * above, a width that is no multiple of quantiles, a DiagGaussian net, a net marked by xt_net_set_dist (as xt_net_set_dist
 * refuses one marked here: clear the other mark first).  A quantile-marked net takes the two wide-head kernels of a
 * C51-marked one (xt_net_set_dist_wide works on it) and is refused by xt_net_dqn_step / _per / _n / _dist. */
int xt_net_set_quant(xt_net* net, int32_t quantiles, double kappa);
/* xt_net_dqn_step_dist's chain with xt_dqn_loss_quant as the head, same launches in number.  Both nets must carry equal
 * quantile marks; cfg->dueling must be 0; actions <= 64; cfg->q_scratch holds 2 * B * (actions * quantiles + 1) floats.  A
 * C51-marked net is refused (its step is xt_net_dqn_step_dist).  With per, the new priority of a start slot is
 * loss_b + eps. */
int xt_net_dqn_step_quant(xt_net* net, xt_net* target_net, const xt_dqn_cfg* cfg, const xt_nstep_cfg* ns,
                          const xt_per_cfg* per, const void* cur_ring, const void* next_ring, int64_t row_bytes,
                          int64_t capacity, int64_t size, const int32_t* slots, int32_t B, const int32_t* action,
                          const double* reward, const uint8_t* done, float* loss_out, float* loss_acc, void* stream);

/* ------------------------------------------------------------------ dueling distributional heads (added under ABI 12; beside
 * the two heads they extend: tests keep xt_net_graph_cache_info the last xt_net_ prototype of this header)
 * A dueling network with a C51 or a quantile head (the architecture of Rainbow).  The state-value stream is folded into
 * the Q head: rows are (A + 1) * N wide, column a * N + i (a < A) is the advantage of atom / quantile i of action a and
 * group A, columns A * N + i, the state-value stream.  Definitions (host twins dist_dueling_combine /
 * dist_dueling_combine_grad of xingtian_amd/model/dqn/dqn_cnn.py):
 *     adv[a, i] = col[a N + i] (a < A);  v[i] = col[A N + i]
 *     mean_i = (sum over ascending a of adv[a, i]) / (float)A                        float32, sequential
 *     l[a, i] = v[i] + (adv[a, i] - mean_i)                                           float32
 * Everything xt_dqn_loss_dist / xt_dqn_loss_quant read as logits[a, :] / quantiles[a, :] -- of the picking, the target and
 * the online rows -- is l[a, :]; the projection, the losses, the terms and out are theirs.  With d_i = what those entries
 * leave in dlogits[b, act * N + i] (w_b and / B included):
 *     dcol[b, a N + i] = d_i * (hot(a == act) - inv_A), inv_A = 1.f / (float)A  (every a < A);  dcol[b, A N + i] = d_i
 *     dvalue[b] = 0
 * The kernels write the whole (A + 1) * N row; no atomics, no dependence on thread order.  The argument lists are those of
 * the entries without _duel; A is the number of actions, logits / t_logits / o_logits / dlogits are [B, (A + 1) * N].
 * Refused: what those entries refuse, with A outside [1, 63]. */
int xt_dqn_loss_dist_duel(const float* logits, const float* t_logits, const float* o_logits, int32_t B, int32_t A,
                          int32_t atoms, double v_min, double v_max, const int32_t* slots, const int32_t* action,
                          const double* reward, const uint8_t* done, double gamma, float* dlogits, float* dvalue, float* out,
                          int32_t* astar, float* maxq, float* m, float* acc, const double* weights, const double* disc,
                          void* stream);
int xt_dqn_loss_quant_duel(const float* logits, const float* t_logits, const float* o_logits, int32_t B, int32_t A,
                           int32_t quantiles, double kappa, const int32_t* slots, const int32_t* action, const double* reward,
                           const uint8_t* done, double gamma, float* dlogits, float* dvalue, float* out, int32_t* astar,
                           float* maxq, float* acc, const double* weights, const double* disc, void* stream);
/* Marks a net that carries the mark of xt_net_set_dist / xt_net_set_quant as dueling: the last of its width / N groups is
 * the state-value stream.  xt_net_dqn_step_dist / _quant then run the _duel head on width / N - 1 actions and take
 * d(features) from heads_dfeat_duel_kernel (with xt_net_set_dist_wide(net, 0): the generic forward and heads_dfeat_kernel,
 * for same-run comparisons); the launches are those of the step without the mark in number.  Both nets of a step must
 * carry the same mark; the dueling flag of xt_dqn_cfg stays refused on a marked net.  Clearing the distributional or
 * quantile mark clears this one.  Refused: a net without such a mark, fewer than 2 groups, more than 63 actions. */
int xt_net_set_duel(xt_net* net, int32_t on);
/* heads_dfeat_duel_kernel stand-alone, for kernel tests and same-run timing: dfeat[b, f] = act'(feat[b, f]) * sum_i d_i *
 * (wq[f, act N + i] + wq[f, A N + i] - inv_A * sum_a wq[f, a N + i]) with d_i = dlogits[b, A N + i], i.e. the product of a
 * row the _duel heads left with the folded head's kernel wq [F, (A + 1) * N].  feat / dfeat [B, F]; the taken action is
 * read through `slots` (may be NULL) and clamped into [0, A).  Refused: a null pointer, A outside [1, 63], N outside
 * [1, 256]. */
int xt_heads_dfeat_duel(const float* feat, int32_t B, int32_t F, int32_t A, int32_t N, const float* wq, const float* dlogits,
                        const int32_t* slots, const int32_t* action, int32_t act_prev, float* dfeat, void* stream);

/* ------------------------------------------------------------------ the step tail stand-alone (appended under ABI 12)
 * The gradient-reduction launch and the optimiser launches every xt_net_*_step ends in, on given buffers, for kernel
 * tests (tests/test_gpu_optim_branch.py).  Each entry fills the argument structs the step fills and calls the step's own
 * launcher; the data-parallel arguments and the folded-IO form are passed as zero.
 *
 * xt_grad_entry: one parameter block.  dst[0..count) = sum of the `nslab` slabs src + z * stride (lane z0 of the entry's
 * zl lanes adds slabs z0, z0 + zl, ... in order, then the lanes are added in order); nslab == 1 with src == dst writes
 * nothing.  pre > 0: the producer has left dst final and `pre` squared-norm partials in the entry's slots already.
 * src, dst 16-byte aligned, stride a multiple of 4.  zl / nblk / pblk0 are outputs: z lanes per block, blocks, first
 * squared-norm partial slot (block j of the entry owns slot pblk0 + j; the entries named by `early` own the first slots). */
typedef struct xt_grad_entry {
  const float* src;
  float* dst;
  int32_t count, nslab;
  int64_t stride;
  int32_t pre;
  int32_t zl, nblk, pblk0;      /* out */
} xt_grad_entry;
/* form: 0 = squared-norm partials only; 1 = the last block to arrive also finalises (norm, clip factor, step size, loss;
 * `counter`); 2 = an extra block does the norm-independent scalars (loss, beta powers, step size), the optimiser derives
 * the clip factor itself (xt_optim_clip_ex); 3 = fused tail: as 2, and the launch applies Adam behind a grid barrier
 * (`counter`, params / m / v; entry dst - grads_base = offset into them).
 * state: the 8 floats of xt_adam_state_init.  counter: 32 * 66 zeroed uint32 words, re-armed by every launch.
 * partial: max_partials floats.  lr_dev (may be NULL): the step size in device memory instead of lr.
 * Loss block (all NULL: none): PPO -- terms [B,4], ent_coef, critic_coef, inv_b, out [4], acc [2] (+=), and with stats
 * (XT_TRAIN_STATS_DOUBLES doubles) the STATS instance, which also reduces rows [B,4]; or IMPALA -- traj_loss [n_traj],
 * out [1], acc [2] (acc_set != 0: = instead of +=), and with stats (XT_IMPALA_STATS_DOUBLES) traj_stats
 * [n_traj, XT_IMPALA_TRAJ_STATS_FLOATS]. */
typedef struct xt_finish_args {
  int32_t form;
  float clip_norm, grad_scale, lr, beta1, beta2, eps;
  const float* lr_dev;
  float* state;
  float* partial;
  int32_t max_partials;
  uint32_t* counter;
  float *params, *m, *v;
  const float* grads_base;
  const float* terms;
  int32_t B;
  float ent_coef, critic_coef, inv_b;
  float* out;
  float* acc;
  const float* rows;
  double* stats;
  const float* traj_loss;
  int32_t n_traj, acc_set;
  const float* traj_stats;
} xt_finish_args;
/* The host half of the gradient-reduction launch, no device call: zl / nblk / pblk0 of every entry, *npartials_out = slots
 * of the whole table, *grid_out = blocks of the launch of `form` over the entries `select` names (bit i = entry i; 0 = all).
 * Refused: a misaligned entry, a stride that is no multiple of 4, more slots than max_partials, form 1 with `select` or a
 * pre-reduced entry, form 3 with `select`. */
int xt_grads_finish_plan_ex(xt_grad_entry* entries, int32_t n, uint32_t select, uint32_t early, int32_t form,
                            int32_t max_partials, int32_t* npartials_out, int32_t* grid_out);
/* The launch (the plan above, unchanged).  *form_out = the form that ran: a request for 3 runs as 2 when the device cannot
 * hold the fused grid resident at once (the step's own rule); form 3 without a counter is refused, as is everything the
 * plan refuses -- before any device call. */
int xt_grads_finish_ex(xt_grad_entry* entries, int32_t n, uint32_t select, uint32_t early, const xt_finish_args* a,
                       void* stream, int32_t* form_out, int32_t* npartials_out);
/* The optimiser launch behind forms 0 / 2: every block derives the clip factor from partial[0..nblocks) itself and block 0
 * leaves it and the norm in state[2] / state[4].  opt_type XT_OPT_ADAM: the step size is state[3] (lr / lr_dev are not
 * read); XT_OPT_RMSPROP_CENTERED: m = mg, v = ms, beta1 = decay, the step size is lr_dev[0] or lr.  stats (may be NULL): the
 * three gradient-norm slots of the running sums are added to. */
int xt_optim_clip_ex(int32_t opt_type, float* param, const float* grad, float* m, float* v, int64_t count, float lr,
                     const float* lr_dev, float beta1, float beta2, float eps, float* state, const float* partial,
                     int32_t nblocks, float clip_norm, float grad_scale, double* stats, void* stream);
/* The one-block finalize launch on given partials (norm, clip factor, beta powers, step size, loss block); `a` as above,
 * form / partial / counter / params are not read and the statistics are not kept. */
int xt_norm_finalize_ex(const float* partial, int32_t nblocks, const xt_finish_args* a, void* stream);

/* ------------------------------------------------------------------ what the last step did (appended under ABI 12)
 * The shape-dependent decisions of the most recent xt_net_*_step / xt_net_forward on `net`, as the host recorded them
 * while enqueueing: for tests (tests/test_gpu_net_zoo.py).  Host words only: no launch, no device memory is touched.
 * out[0 .. XT_STEP_REPORT_NET_WORDS): the net's words, then XT_STEP_REPORT_LAYER_WORDS per layer, trunk 0 first; `cap`
 * = words offered (refused when too few).
 * Net: WORDS = words written; LAYERS; TRUNKS; FWD_FUSE12 / BWD_FUSE21 = 1 when the one-launch conv1 + conv2 forward /
 * the first layer's weight gradient inside the second layer's backward launch was taken; HEAD_PATH =
 * xt_net_last_head_path; TAIL_OVERLAP = the xt_tuning.tail_overlap bits the step honoured (0: refused or off);
 * FINISH_FORM = form of the gradient-reduction launch (xt_finish_args.form; -1: none ran yet), FINISH_BLOCKS = its
 * squared-norm partial slots; PARTIAL_FLOATS = capacity of a split-K partial region; MAX_NORM_PARTIALS = capacity of
 * the squared-norm scratch; HEAD_CHUNKS = slabs of the head weight gradients.
 * Layer: KSPLIT = split-K partial slabs the last forward LEFT in the layer's own region (1: none -- a layer that was not
 * offered the deferral finishes its split itself and reports 1), DEFERRED = 1 when they were left for the fused head; MSPLIT = weight-gradient slabs of the last backward, SLAB_CAP = slabs the region holds;
 * MASK_VALID = 1 when the last forward wrote the relu sign mask; PREACT = 1 when the layer keeps its pre-activation
 * (swish / gelu); NPRE = squared-norm partials the last backward launch pre-reduced; TRUNK.
 * Tail (appended): XT_STEP_TAIL_WORDS words behind the out[WORDS] words above, written when `cap` has room for them
 * and not counted in WORDS: XT_STEP_TAIL_FWD_FUSE123 = 1 when the last forward ran the one-launch conv1 + conv2 + conv3 forward
 * (xt_net_set_fwd_fuse123_flat). */
enum {
  XT_STEP_REPORT_WORDS = 0, XT_STEP_REPORT_LAYERS = 1, XT_STEP_REPORT_TRUNKS = 2, XT_STEP_REPORT_FWD_FUSE12 = 3,
  XT_STEP_REPORT_BWD_FUSE21 = 4, XT_STEP_REPORT_HEAD_PATH = 5, XT_STEP_REPORT_TAIL_OVERLAP = 6,
  XT_STEP_REPORT_FINISH_FORM = 7, XT_STEP_REPORT_FINISH_BLOCKS = 8, XT_STEP_REPORT_PARTIAL_FLOATS = 9,
  XT_STEP_REPORT_MAX_NORM_PARTIALS = 10, XT_STEP_REPORT_HEAD_CHUNKS = 11, XT_STEP_REPORT_NET_WORDS = 12
};
enum {
  XT_STEP_REPORT_L_KSPLIT = 0, XT_STEP_REPORT_L_DEFERRED = 1, XT_STEP_REPORT_L_MSPLIT = 2, XT_STEP_REPORT_L_SLAB_CAP = 3,
  XT_STEP_REPORT_L_MASK_VALID = 4, XT_STEP_REPORT_L_PREACT = 5, XT_STEP_REPORT_L_NPRE = 6, XT_STEP_REPORT_L_TRUNK = 7,
  XT_STEP_REPORT_LAYER_WORDS = 8
};
enum { XT_STEP_TAIL_FWD_FUSE123 = 0, XT_STEP_TAIL_WORDS = 1 };
int xt_net_last_step_report(const xt_net* net, int32_t* out, int32_t cap);

/* What the hipGraph cache of xt_net_ppo_train / xt_net_impala_train(_io) has done on this net so far (appended under ABI
 * 12; diagnostic, for tests/test_gpu_train_entry.py).  Host words only: no launch, no device memory is touched.  `cap` =
 * words offered (refused below XT_GRAPH_CACHE_WORDS).  CAPTURES = calls that captured and instantiated a graph (a call
 * whose enqueue refused inside the capture is not one), LAUNCHES = graph launches (every use_graph call that succeeded),
 * EVICTIONS = graphs given up for a new key while all slots were taken (the least recently used one goes); these three
 * count over the net's lifetime.  LIVE_SLOTS = graphs held now (at most 8): xt_net_bind destroys them all. */
enum {
  XT_GRAPH_CACHE_CAPTURES = 0, XT_GRAPH_CACHE_LAUNCHES = 1, XT_GRAPH_CACHE_EVICTIONS = 2, XT_GRAPH_CACHE_LIVE_SLOTS = 3,
  XT_GRAPH_CACHE_WORDS = 4
};
int xt_net_graph_cache_info(const xt_net* net, int32_t* out, int32_t cap);

/* ------------------------------------------------------------------ noisy layers (NoisyNet; appended under ABI 12)
 * Factorised-Gaussian noisy Dense layers (Fortunato et al. 2018) beside the net, not inside it: the learner keeps a STORE
 * of n_net floats in the net's own layout -- holding the means mu at the noisy layers' offsets -- followed by one sigma
 * block per noisy layer, and binds the net (xt_net_bind) to a second buffer params_eff of n_net floats.  xt_noisy_compose
 * writes the effective parameters there before the step, xt_noisy_grads forms the sigma gradients behind it; no layer
 * kernel, step entry or optimiser knows about noise.
 *
 * xt_noisy_layer: the mean block [K, N] kernel + [N] bias at store[w_off ..), inside [0, n_net); the sigma block of the
 * same form at store[sigma_off ..), at or behind n_net; the layer's vectors in `noise`: f_in [K] at noise_off, f_out [N]
 * at noise_off + align4(K).  All three offsets are multiples of 4.  `index`: the layer's position among the model's
 * noisy layers (counter word c1 of its draws), so that a table holding one layer draws what the whole table draws.
 *
 * Definitions (float32, no contraction), Philox4x32-10 keyed by seed (k0 low word, k1 high word):
 *   element i of vector v (0: f_in, 1: f_out) of layer `index`:
 *     block = philox(c0 = i >> 1, c1 = 2 * index + v, c2 = (uint32)call, c3 = stream_id)
 *     u1, u2 = uniform(words 2 (i & 1), 2 (i & 1) + 1), uniform(w) = ((float)(w >> 9) + 0.5) * 2^-23
 *     x = sqrtf(-2 logf(u1)) * cosf(6.283185307179586f * u2);  f = copysignf(sqrtf(fabsf(x)), x)
 *   e[k, n] = f_in[k] * f_out[n];  W_eff[k, n] = mu[k, n] + sigma[k, n] * e[k, n];  b_eff[n] = mu_b[n] + sigma_b[n] * f_out[n]
 *   g_sigma[k, n] = dW_eff[k, n] * e[k, n];  g_sigma_b[n] = db_eff[n] * f_out[n] */
#define XT_NOISY_MAX_LAYERS 8
typedef struct xt_noisy_layer {
  int64_t w_off, sigma_off, noise_off;
  int32_t K, N, index, reserved;
} xt_noisy_layer;
/* One launch: params_eff[0, n_net) = store[0, n_net) bit for bit, but W_eff / b_eff over the mean blocks of `layers`; every
 * f_in / f_out drawn is stored in `noise` (the values used).  noise_in (may be NULL; laid out as `noise`): the vectors are
 * taken from it instead of drawn, and copied to `noise`.  mean_only != 0: a plain copy, nothing is drawn, `noise` is not
 * written.  Nothing outside params_eff[0, n_net) and the layers' vectors in `noise` is written.
 * Refused: a null pointer, store == params_eff or either not 16-byte aligned, n_layers outside [1, XT_NOISY_MAX_LAYERS],
 * n_net that is not a positive multiple of 4, a layer with K or N < 1 or (K + 1) * N >= 2^31, a misaligned or negative
 * offset, a mean block that leaves [0, n_net), a sigma block in front of n_net, overlapping mean blocks, sigma blocks or
 * noise ranges, stream_id or index negative. */
int xt_noisy_compose(const xt_noisy_layer* layers, int32_t n_layers, const float* store, float* params_eff, int64_t n_net,
                     float* noise, const float* noise_in, uint64_t seed, uint64_t call, int32_t stream_id,
                     int32_t mean_only, void* stream);
/* One launch behind the step's backward: grads[sigma_off ..) of every layer = g_sigma / g_sigma_b, from grads[w_off ..)
 * (dW_eff, db_eff: what the backward left; not modified) and the vectors xt_noisy_compose stored in `noise`.  `grads` is
 * laid out as the store.  Refused: what xt_noisy_compose refuses of a table, and a sigma block in front of the end of a
 * mean block. */
int xt_noisy_grads(const xt_noisy_layer* layers, int32_t n_layers, const float* noise, float* grads, void* stream);

/* The Dense instance of the fused backward launch (XT_BWD_PATH_PF_GENERIC of xt_layer_bwd; appended, the ABI version stays):
 * process-wide, default 1.  on == 1: its weight-gradient blocks address the rows of the 1x1, stride-1, unpadded layer
 * directly (row m at byte m * K * 4) instead of decoding them into an LDS table behind a barrier, and the blocks that own
 * the bias gradient take the fp32 dy rows from memory next to their operands; its input-gradient blocks skip the tap
 * decode of their loads (the layer has one tap); and the head weight-gradient tiles that ride in the launch share the
 * workgroup slots the other blocks leave (a head block walks several tiles) instead of queueing behind each other.  dx,
 * dW, db, the head slabs, the squared-norm partials and the reported path are bit for bit those of on == 0, which
 * launches the instance as it was.  Returns the PREVIOUS value
 * (0 or 1); anything but 0 or 1 is refused: returns 2, xt_last_error names the entry, nothing changes.  Set it before
 * graphs are captured outside a net (a net's own cached hipGraphs carry it in their key). */
int xt_bwd_dense_lean_set(int32_t on);

/* ------------------------------------------------------------------ MuZero: the unrolled model update (appended under ABI 12)
 * Three layer chains with shared weights in ONE flat parameter buffer (xt/model/muzero/muzero_model.py:103-140):
 *   rep   obs -> h_0                       n_rep Dense layers on float32 observations (relu, the last one N == hidden)
 *   dyn   [h_i | onehot(a_i)] -> t_i       n_dyn - 2 trunk layers (the first one has C == hidden + action_dim), then
 *         h_{i+1} = relu(Dense_h(t_i))     layer n_dyn - 2 (N == hidden)
 *         r_{i+1} = softmax(Dense_r(t_i))  layer n_dyn - 1 (N == reward_support)
 *   pred  h_k -> q_k                       n_pred - 2 trunk layers, then
 *         v_k = softmax(Dense_v(q_k))      layer n_pred - 2 (N == value_support)
 *         p_k = softmax(Dense_p(q_k))      layer n_pred - 1 (N == action_dim)
 * Every layer's block is [K, N] kernel + [N] bias at param_off; the rep chain runs on the trunk-layer kernels (C and N
 * multiples of 4, blocks 16-byte aligned), the Dense layers of dyn and pred on the kernels of xt_muzero.hip (any width).
 * The hidden states of all unroll + 1 steps are stacked as [(unroll + 1) * B, hidden], step k in rows [k B, (k + 1) B):
 * the prediction chain's forward, backward and weight gradient run once over the stack, the reward head and every dyn
 * layer's weight gradient once over the unroll * B rows of the dynamics steps; only the dyn chain itself is sequential.
 * No atomics; every sum has a fixed order, so a step is bit-identical from run to run.
 *
 * Loss (the weight-decay term of the reference is a constant of its graph and is left out):
 *   ce(p, t) = -(1 / (B N)) sum_b sum_j t_bj log(p_bj + 1e-10)
 *   L = ce(p_0, pi_0) + ce(v_0, z_0) + sum_{i < U} [ce(r_{i+1}, u_i) + ce(p_{i+1}, pi_{i+1}) + ce(v_{i+1}, z_{i+1})]
 * Gradient: the terms of unroll step i carry 1 / U; the gradient that dyn step k sends into h_k is halved for k >= 1. */
typedef struct xt_mz xt_mz;

#define XT_MZ_MAX_UNROLL 16
#define XT_MZ_MAX_CHAIN 8

typedef struct xt_mz_desc {
  int32_t n_rep, n_dyn, n_pred;
  const xt_layer_desc* rep;
  const xt_layer_desc* dyn;
  const xt_layer_desc* pred;
  int32_t hidden, action_dim, value_support, reward_support, unroll;
  int32_t obs_dim;               /* width of the float32 observation vector the first rep layer reads      */
  int64_t n_params;              /* floats of the flat buffer (a multiple of 4)                             */
  double value_min, value_max, reward_min, reward_max;
} xt_mz_desc;

typedef struct xt_mz_cfg {
  float lr, beta1, beta2, eps;   /* tf.train.AdamOptimizer(lr): 0.9, 0.999, 1e-8; no clipping               */
} xt_mz_cfg;

/* Refused with a message: unroll outside [1, XT_MZ_MAX_UNROLL], a support below 2, action_dim below 1, max <= min, a
 * chain that is too short, too long or whose widths do not meet, a rep layer that is not a Dense layer. */
int xt_mz_create(const xt_mz_desc* desc, int32_t max_batch, xt_mz** out);
void xt_mz_destroy(xt_mz* mz);
int64_t xt_mz_workspace_bytes(const xt_mz* mz);
/* Buffers stay caller-owned, as with xt_net_bind: params / grads / adam_m / adam_v hold n_params floats (grads zeroed by
 * the caller: the padding between blocks is never written), adam_state 8 floats (xt_adam_state_init). */
int xt_mz_bind(xt_mz* mz, float* params, float* grads, float* adam_m, float* adam_v, float* adam_state, void* workspace,
               int64_t workspace_bytes);
/* One whole gradient step, enqueued without synchronising: forward, loss, backward; grads is complete behind it.
 *   obs            float32 [., obs_dim]: the observation store; sample b is row idx[b] (idx may be NULL: row b)
 *   actions        int32 [B, unroll]; an action outside [0, action_dim) conditions on a zero row, as tf.one_hot does
 *   target_value   float64 [B, unroll + 1], target_reward the same: scalars, made two-hot on the device
 *   target_policy  float32 [B, unroll + 1, action_dim]
 *   loss_out       1 double: L */
int xt_mz_step(xt_mz* mz, const void* obs, const int32_t* idx, int32_t B, const int32_t* actions,
               const double* target_value, const double* target_reward, const float* target_policy, const xt_mz_cfg* cfg,
               double* loss_out, void* stream);
/* xt_adam_tf_clip over the flat gradient with a clip factor of exactly 1.0f */
int xt_mz_apply(xt_mz* mz, const xt_mz_cfg* cfg, void* stream);
/* Forward only.  policy [B, action_dim], value [B, value_support] (softmax outputs), hidden [B, hidden]. */
int xt_mz_initial(xt_mz* mz, const void* obs, const int32_t* idx, int32_t B, float* policy, float* value, float* hidden,
                  void* stream);
/* hidden_in [B, hidden], action int32 [B] -> hidden_out, reward [B, reward_support], policy, value */
int xt_mz_recurrent(xt_mz* mz, const float* hidden_in, const int32_t* action, int32_t B, float* hidden_out, float* reward,
                    float* policy, float* value, void* stream);

/* The loss head stand-alone: softmax + target + cross-entropy + d(logits) for nblk blocks of B rows, N wide.
 *   logits [nblk * B, N]; row r = k * B + b takes its target from column k of sample b:
 *   target_dense   (may be NULL) float32 [B, S, N]: row (b, k) as given
 *   target_scalar  (else) float64 [B, S]: the two-hot row of clip(t, tmin, tmax) - tmin, compressed by
 *                  c = sign(x) (sqrt(|x| + 1) - 1) + 0.001 x in float64: 1 - rest on floor(c), rest on floor(c) + 1, each
 *                  rounded once; a floor at or beyond N - 1 puts the whole mass on bin N - 1; nothing leaves the row
 *   p = softmax (float32, maximum subtracted);  w = t / (p + 1e-10);  dz_j = s / (B N) p_j (sum_i w_i p_i - w_j) with
 *   s = scale0 for block 0 and scale_rest behind it;  rowloss[r] = -(sum_j t_j log(p_j + 1e-10)) / (B N)  (float64)
 *   probs, dz (each may be NULL) [nblk * B, N]; rowloss float64 [nblk * B]; loss_out (may be NULL) 1 double: the rows'
 *   sum in a fixed order.  N <= 64: one wavefront per row, else one workgroup per row.  2 <= N <= 65536. */
int xt_mz_loss(const float* logits, int32_t nblk, int32_t B, int32_t N, int32_t S, const float* target_dense,
               const double* target_scalar, double tmin, double tmax, float scale0, float scale_rest, float* probs,
               float* dz, double* rowloss, double* loss_out, void* stream);

/* The conditioned first dynamics layer stand-alone, without materialising [h | onehot(a)]: w [hidden + A, N], bias [N].
 * Rows are nblk blocks of B: row r = i * B + b is conditioned on actions[b * a_stride + i].
 *   forward   y = act(((sum_{k ascending} h_k w[k]) + w[hidden + a]) + bias), float32 without contraction */
int xt_mz_cond_fwd(const float* h, const int32_t* actions, int32_t a_stride, int32_t nblk, int32_t B, int32_t hidden,
                   int32_t A, int32_t N, const float* w, const float* bias, int32_t act, float* y, void* stream);
/*   backward  dy [nblk * B, N] is d(pre-activation).
 *   dwb [(hidden + A + 1) * N]: dW[k] = sum_r h_rk dy_r, dW[hidden + a] = sum_{r: a_r == a} dy_r (zero where nobody took
 *   a), db = sum_r dy_r; rows summed in ascending r inside slabs of XT_MZ_WGRAD_ROWS rows, the slabs then in ascending
 *   order (slabs: scratch of ceil(rows / XT_MZ_WGRAD_ROWS) * (hidden + A + 1) * N floats, may be NULL for one slab)
 *   g [nblk * B, hidden] = relu'(h) * (g_pred + c * sum_{n ascending} dy_n w[k, n])   (the hidden-state join; g_pred may be
 *   NULL: 0;  wt: scratch of N * hidden floats for the transposed kernel) */
#define XT_MZ_WGRAD_ROWS 128
int xt_mz_cond_bwd(const float* h, const int32_t* actions, int32_t a_stride, int32_t nblk, int32_t B, int32_t hidden,
                   int32_t A, int32_t N, const float* w, const float* dy, const float* g_pred, float c, float* g, float* dwb,
                   float* slabs, float* wt, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* XT_MI355X_H_ */
