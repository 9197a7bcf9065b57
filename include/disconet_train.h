/*
 * disconet_train.h -- C ABI of the training-step kernels (same library,
 * libdisconet_hip.so).  SURVEY.md §8(f) "next" row 1.
 *
 * Replaces what autograd + torch.optim run under
 *   upstream:coperception/utils/CoDetModule.py :: CoDetModule.step
 *     (model(...) in train() mode; loss_calculator; loss.backward(); optimizer.step())
 *   upstream:coperception/utils/loss.py :: SoftmaxFocalClassificationLoss,
 *     WeightedSmoothL1LocalizationLoss
 * (invoked by the `python train_codet.py ... --com disco` line, /root/reference/README.md:54-63;
 * the sources are in the un-vendored submodule, /root/reference/.gitmodules:1-3, so there
 * are no line numbers to cite).
 *
 * Same conventions as disconet_hip.h: device pointers, fp32 NHWC maps with an explicit
 * row stride ("ld", in floats) where a tensor may be a channel slice of a wider one,
 * caller-owned buffers and workspaces, everything enqueued on `stream`, int status +
 * dn_last_error().
 */
#ifndef DISCONET_TRAIN_H
#define DISCONET_TRAIN_H

#include "disconet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- conv backward ------------------------------------------------------------------- */

/* dW of the layer `d` describes (the same descriptor its forward dn_conv2d used; d->ldo is
 * the row stride of dz).  dw[co][ci][ky][kx] with ci running over c0 + c1; `dw_cin_total`
 * (0 = c0 + c1) is the ci extent of the tensor dw points into, so a column block of a wider
 * weight (the attention MLP's [W_ego | W_nbr]) can be written in place.  Slices are summed
 * in a fixed order: deterministic.  accumulate != 0 adds to dw. */
size_t dn_conv_wgrad_workspace(const dn_conv_desc* d);
/* workspace of the per-channel reductions below (dn_bn_train_stats, dn_bn_train_backward, dn_channel_sum): the
 * folded sums AND every workgroup's partial.  The size depends on the library version (it grew with the
 * deterministic reductions of dn_version 112), so those entry points take the size of what was allocated
 * (`sums_bytes`) and refuse a workspace that is too small instead of writing past it. */
size_t dn_reduce_workspace_bytes(int n_groups, long rows_per_group, int c);
int dn_conv_wgrad(const dn_conv_desc* d, const float* src0, const float* src1, const float* dz,
                  void* workspace, float* dw, int dw_cin_total, int accumulate, void* stream);

/* dn_conv_wgrad on the f16 MFMA with split operands (csrc/wgrad_sp.inl): every dz and x value enters as an f16 hi + lo pair
 * (half(v) + half(v - half(v)), 22 significand bits) and a product is hi.hi + hi.lo + lo.hi on v_mfma_f32_32x32x16_f16 with
 * fp32 accumulation -- 5.3 x the fp32 MFMA's rate per product.  The maps stay what dn_conv_wgrad takes (float32 NHWC, same
 * descriptor, same gather: x2 upsample of source 0, concat); the kernel multiplies by the lifts, splits and transposes while
 * it stages (K = pixels: a lane's fragment is 8 consecutive pixels of one channel).
 *   dz_lift, x_lift: powers of two.  dz_lift brings max |dz| * dz_lift to ~2^8 (the lift of dn_bn_bwd_out.sp_lift);
 *   x_lift (activations: 16) keeps the lo halves of small activations out of the f16 subnormal range.  A lifted value beyond
 *   +-65504 is clamped and sets bit 0 of dn_sp_range_flags: that step's gradients are invalid.  1 / (dz_lift * x_lift) is
 *   applied by the fixed-order slice sum (exact).
 * Layers: 3x3; stride 2 with ONE 16-byte loadable source of 32 k channels and c_out >= 32 (the encoder's down-sampling layers: the
 * patch is staged as two column-parity planes so that a fragment is still consecutive dwords); stride 1 with 16-byte aligned dz
 * (and sources, with the exception below), and either c_out >= 64 with c0 and c1 multiples of 64 (a workgroup owns a
 * 64 x 64 (co, ci) block) or c_out >= 32 (32 x 32 blocks: the 32-channel layers of the full-resolution maps) with either two
 * sources of 32 k channels each or ONE source of any width, which then need not be 16-byte loadable (the 13-channel voxel
 * grid of conv_pre_1: dword loads, the last block partial).  dn_conv_wgrad_sp_supported returns that block size, 0 = no such
 * kernel for the layer.  Deterministic like dn_conv_wgrad.  Workspace: dn_conv_wgrad_sp_workspace(d) bytes. */
int dn_conv_wgrad_sp_supported(const dn_conv_desc* d);
size_t dn_conv_wgrad_sp_workspace(const dn_conv_desc* d);
int dn_conv_wgrad_sp(const dn_conv_desc* d, const float* src0, const float* src1, const float* dz, void* workspace, float* dw,
                     int dw_cin_total, int accumulate, float dz_lift, float x_lift, void* stream);
/* dn_conv_wgrad_sp with dz taken from its SP copy (round 6): dz_sp = dz * dz_lift as the SP tensor [n][c_out / 16][4][h_out][w_out]
 * that the BatchNorm backward writes for the data gradient (dn_bn_bwd_out.dz_sp; c_out % 16 == 0) -- the same hi / lo
 * halves the fp32 form derives while it stages dz, so dw is the same bits; the staging of the dz tile becomes byte permutes, and
 * a layer whose data gradient and bias gradient do not read the fp32 dz either can leave dn_bn_bwd_out.dz NULL and save the
 * fp32 copy's write (a quarter of that launch's bytes). */
int dn_conv_wgrad_sp_z(const dn_conv_desc* d, const float* src0, const float* src1, const void* dz_sp, void* workspace, float* dw,
                       int dw_cin_total, int accumulate, float dz_lift, float x_lift, void* stream);

/* tools and tests only: the plan of the weight gradient of layer `d` -- sp = 0: dn_conv_wgrad, sp != 0: dn_conv_wgrad_sp / _sp_z
 * (DN_ERR_ARG where the layer has no split-f16 kernel) -- from the very functions the launch uses.  Host only: launches nothing,
 * needs no GPU.  Writes up to n of 12 ints and returns 12:
 *   [0] ct (channels per side of a workgroup's block, 32 / 64)  [1] TH  [2] TW (output pixels of a tile)  [3] h_out  [4] w_out
 *   [5] tiles_x  [6] tiles_y  [7] n_tiles (all images)  [8] n_cot  [9] n_cit  [10] n_slices  [11] taps */
int dn_conv_wgrad_plan(const dn_conv_desc* d, int sp, int* out, int n);
/* tools and tests only: which kernel did the last weight-gradient launch of this process run?  Written by the entry points once
 * nothing can refuse the call any more (a refused call leaves the record as it was).  Writes up to n of 10 ints, returns 10:
 *   [0] entry (0 dn_conv_wgrad, 1 dn_conv_wgrad_sp, 2 dn_conv_wgrad_sp_z; -1: none yet)  [1] ksize  [2] stride
 *   [3] block (32 / 64)  [4] 1 = the ZSP instantiation  [5] vec0  [6] vec1  [7] vecz: 16-byte loads of source 0 / source 1 / dz
 *   (split-f16 kernels: vec0 = vec1 = their one vecx flag, vecz = 1)  [8] workgroups of the launch  [9] n_slices */
int dn_conv_wgrad_last_form(int* out, int n);

/* Weights of the data-gradient conv: wt[ci][co][2-ky][2-kx] = w[co][ci][ky][kx] for the
 * c_in columns starting at `ci_first` of a [c_out][cin_total][k][k] tensor.  dx is then
 * dn_conv2d(dz; pack(wt)) with stride 1 -- for a stride-2 layer with src0 read zero-stuffed
 * (dn_conv_desc.up0 = 2: source pixel (y/2, x/2) where y and x are even, 0 elsewhere). */
int dn_conv_dgrad_weights(const float* w_oihw, int c_out, int cin_total, int ci_first, int c_in,
                          int ksize, float* wt_oihw, void* stream);

/* Parity-phase data gradient of a STRIDE-2 3x3 layer (even h_in, w_in): input pixel (2 m + py, 2 n + px) receives
 * gradient only through the taps whose offset has its parity, so dx splits into four stride-1 convs over dz, one per
 * class (py, px), of 1, 2, 2 and 4 taps -- a quarter of the MFMAs of the zero-stuffed form (dn_conv_desc.up0 = 2, kept for
 * odd map sizes).  dn_conv_dgrad_class_weights writes class (py, px)'s 3x3 kernel v[ci][co][3][3] (unused taps zero) and
 * the mask of the taps it uses; dn_conv2d_taps (disconet_hip.h) runs it over dz [n][h_out][w_out][c_out] with only those
 * taps multiplied, writing output pixel (m, n) to dx[2 m + py][2 n + px] through the output strides. */
int dn_conv_dgrad_class_weights(const float* w_oihw, int c_out, int cin_total, int ci_first, int c_in, int py, int px,
                                float* v_oihw, int* tap_mask, void* stream);

/* ---- batch norm in training mode (+ ReLU) ---------------------------------------------- */

/* Statistics over `rows_per_group` pixels for each of `n_groups` consecutive groups of rows
 * (n_groups = 1: nn.BatchNorm2d over the batch; n_groups = calls: the attention MLP's BN
 * layers, which see one (ego, neighbour) pair of 1 x C x 32 x 32 per call).
 * sums: workspace of dn_reduce_workspace_bytes(n_groups, rows_per_group, c) bytes (the folded sums and every
 * workgroup's partial: the per-channel sums are DETERMINISTIC -- fixed thread, workgroup and fold order, no
 * atomics).  var is the biased variance.
 *   running_mean, running_var (both or neither; NULL = none; ONE group): the launch that finishes the statistics also applies
 *   the running-statistics update of dn_bn_update_running (momentum, unbiased variance with rows / (rows - 1)) -- one launch
 *   instead of three behind the reduction (round 6), bit for bit the separate calls.  momentum is read only then. */
int dn_bn_train_stats(const float* z, int n_groups, long rows_per_group, int c, int ldz, double* sums, size_t sums_bytes,
                      float* mean, float* var, float* running_mean, float* running_var, float momentum, void* stream);

/* Two-phase form for a BatchNorm batch that is spread over several ranks (agent-parallel training, disconet_amd/sharded.py):
 *   dn_bn_train_stats_partial   this rank's rows -> the folded sums [n_groups][2 c] doubles (sum z, sum z^2) at the START of `sums`
 *   (the caller all-reduces those n_groups * 2 * c doubles over the ranks)
 *   dn_bn_train_stats_finish    mean / biased var from the sums over `norm_rows` rows per group (the GLOBAL count).
 * dn_bn_train_stats is the two phases back to back with norm_rows = rows_per_group. */
int dn_bn_train_stats_partial(const float* z, int n_groups, long rows_per_group, int c, int ldz,
                              double* sums, size_t sums_bytes, void* stream);
int dn_bn_train_stats_finish(const double* sums, int n_groups, long norm_rows, int c, float* mean, float* var, void* stream);

/* y = act((z - mean) * rsqrt(var + eps) * gamma + beta), act = ReLU if relu.  Two optional outputs of the same launch:
 *   relu_mask (NULL = none; relu == 1, c % 4 == 0, 16-byte aligned tensors): the ReLU gate of the backward as ONE BYTE PER FOUR
 *     CHANNELS, relu_mask[(row * c + ch) / 4] bit (ch % 4) = (y[row][ch] > 0) -- rows * c / 4 bytes, 1/16 of y.  The backward
 *     takes it in place of y with dn_bn_bwd_desc.relu = 2: its two passes then read 1/4 byte per element where y costs 4 (same
 *     gate, same results bit for bit).
 *   y_sp (NULL = none; needs relu_mask, ONE group and DN_BN_FORM_SP_APPLY below; rows_per_group % hw == 0, hw = pixels per
 *     image; 16-byte aligned tensors): y ALSO as an SP tensor (include/disconet_hip.h "SP tensor": [image][c / 16][4 quarters]
 *     [hw][8 halves]; dn_sp_tensor_bytes(rows / hw, ., ., c) bytes) -- the operand of the NEXT layer's forward conv on the
 *     split-f16 LDS-DMA engine (dn_spconv2d_nhwc), so that the training forward runs the inference engine's kernels instead of
 *     splitting fp32 rows on the VALU while staging them (round 6).  The split is dn_sp_from_nhwc's (clamp to +-65504,
 *     hi = half(y), lo = half(y - hi)); a clamped value sets the engine's sticky range flag.  y (fp32) is still written: the
 *     weight gradient of the next layer and the skip consumers read it.  hw is read only with y_sp. */
int dn_bn_train_apply(const float* z, const float* mean, const float* var, const float* gamma, const float* beta, float eps,
                      int relu, int n_groups, long rows_per_group, int c, int ldz, float* y, unsigned char* relu_mask,
                      void* y_sp, int hw, void* stream);

/* running = (1 - momentum) * running + momentum * batch stat, group after group in the order
 * `order` lists them (null = 0..n_groups-1); running_var takes the unbiased variance. */
int dn_bn_update_running(const float* mean, const float* var, int n_groups, long rows_per_group,
                         int c, const int* order, float momentum, float* running_mean,
                         float* running_var, void* stream);

/* Backward of y = act(bn(z)), in two phases over the same description of the pass:
 *   g = (dy_a + dy_b) * (y > 0)      dbeta = sum g      dgamma = sum g * zhat                          (phase 1)
 *   dz = gamma * rstd * (g - mean(g) - zhat * mean(g * zhat))       (means per group)                  (phase 2)
 * Pointers first, then 32-bit fields: 96 bytes, no padding on any ABI with 8-byte pointers. */
typedef struct dn_bn_bwd_desc {
  const float* dy_a;   /* the incoming gradient, row stride ld_a; its resolution and layout: up_a */
  const float* dy_b;   /* NULL, or a second gradient at y's resolution (row stride ld_b) that is added to dy_a */
  const void* y;       /* relu = 1: the fp32 map y; relu = 2: dn_bn_train_apply's byte mask of (y > 0) instead (c % 4 == 0);
                        * relu = 0: not read */
  const float *z, *mean, *var;
  const float* gamma;  /* read by phase 2 only */
  int32_t ld_a;
  int32_t up_a;        /* 0: dy_a is [img][h][w][.].  1: dy_a lives at twice the resolution and its 2 x 2 block sum is taken (the
                        * backward of the decoder's nearest upsample).  2: dy_a is the SPACE-TO-DEPTH image of the gradient,
                        * [img][h / 2][w / 2][4 c] with pixel (y, x), channel ch at (y / 2, x / 2), channel
                        * ((y & 1) * 2 + (x & 1)) * c + ch -- what one split-f16 launch over the four parity classes of a
                        * stride-2 layer's data gradient writes (round 5; even h, w; ld_a >= 4 c). */
  int32_t ld_b, relu;
  int32_t n_groups, h, w, images_per_group, c;      /* h, w: y's dims; rows per group = images_per_group * h * w */
  float eps;
} dn_bn_bwd_desc;

/* What phase 2 writes.  Every member is optional (0 / NULL = not asked for); at least one of dz, dz_sp is given.  56 bytes. */
typedef struct dn_bn_bwd_out {
  float* dz;           /* the fp32 dz.  NULL (needs dz_sp and DN_BN_FORM_DZ_NULL below): only the SP copy is written -- for a layer
                        * whose weight gradient (dn_conv_wgrad_sp_z), data gradient and bias gradient all read dz through this
                        * launch's other outputs; saves a quarter of the launch's bytes */
  void* dz_sp;         /* dz * sp_lift ALSO as the SP tensor [n][c / 16][4][h][w] x 16 bytes of the inference conv engine
                        * (disconet_hip.h "SP tensor") -- the pre-split operand of the split-f16 data gradient (dn_spconv2d_nhwc)
                        * and of dn_conv_wgrad_sp_z: the split is paid once, by the kernel that produces dz, not by the convs'
                        * staging.  One group, c % 16 == 0, 16-byte aligned tensors. */
  float* dbias;        /* the BIAS GRADIENT of the conv in front of this BatchNorm (round 6): dbias[ch] = sum over this call's
                        * rows of dz[.][ch], written by the same launch that writes dz (a thread adds its own values in fp32, a
                        * workgroup its threads in double, fold in a fixed order: deterministic) -- in place of a dn_channel_sum
                        * pass that reads dz again.  Needs DN_BN_FORM_BIAS below, aligned tensors and bias_ws. */
  double* bias_ws;     /* workspace of the bias gradient, dn_bn_bias_workspace_bytes(rows, c) bytes: [c] doubles for the folded
                        * sums, then [blocks][c] partials.  Never the reduction's `sums` (the same launch reads those). */
  int* n_blocks;       /* non-NULL (dbias must then be NULL): the bias gradient with its FOLD DEFERRED -- the partials stay in
                        * bias_ws, *n_blocks receives their count, and a dn_fold_job of dn_channel_sum_fold_multi folds them
                        * later (see there); the same bits as dbias */
  uint64_t bias_ws_bytes;
  float sp_lift;       /* with dz_sp: a power of two that brings max |dz| * sp_lift to ~2^8 -- a value is stored as
                        * half(x) + half(x - half(x)): 2^-22 relative while 2^-3 <= |x| <= 65504, so the top 19 binades of the
                        * tensor keep full precision, smaller elements an absolute floor of 2^-25 / sp_lift, and 256 x of head
                        * room remains before the clamp (which sets bit 0 of dn_sp_range_flags: the gradients of that step are
                        * invalid).  The caller folds 1 / sp_lift into the data gradient's scale vector (exact). */
  int32_t reserved;
} dn_bn_bwd_out;
size_t dn_bn_bias_workspace_bytes(long rows, int c);

/* The two phases, for a BatchNorm batch that is spread over several ranks (see dn_bn_train_stats_partial): `_partial` leaves this
 * rank's folded sums of g and g * zhat at the start of `sums` (workspace of dn_reduce_workspace_bytes(n_groups,
 * images_per_group * h * w, c) bytes) and writes dgamma / dbeta out of THESE rows (plain sums over rows and groups, ADDED when
 * accumulate != 0: the ranks' shares meet in the gradient all-reduce); the caller all-reduces the n_groups * 2 * c doubles;
 * `_finish` writes `out` for this rank's rows with the means taken over `norm_rows` rows per group.
 * dn_bn_train_backward is the two phases back to back with norm_rows = images_per_group * h * w, for every form of `out`. */
int dn_bn_train_backward_partial(const dn_bn_bwd_desc* d, double* sums, size_t sums_bytes, float* dgamma, float* dbeta,
                                 int accumulate, void* stream);
int dn_bn_train_backward_finish(const dn_bn_bwd_desc* d, const double* sums, long norm_rows, const dn_bn_bwd_out* out,
                                void* stream);
int dn_bn_train_backward(const dn_bn_bwd_desc* d, double* sums, size_t sums_bytes, const dn_bn_bwd_out* out, float* dgamma,
                         float* dbeta, int accumulate, void* stream);

/* out[c] (+)= sum over rows of x[row][c] (bias gradients); sums: dn_reduce_workspace_bytes(1, rows, c) bytes */
int dn_channel_sum(const float* x, long rows, int c, int ld, double* sums, size_t sums_bytes, float* out,
                   int accumulate, void* stream);

/* The same sums with their FOLDS DEFERRED (round 6).  A bias gradient is a leaf of the backward: nothing reads it before the
 * optimizer step, so the launch that leaves the per-workgroup partials need not be followed by a fold of its own (26 launches of
 * ~5 us per training step on a stream with nothing to run beside them).  dn_bn_bwd_out.n_blocks / dn_channel_sum_partial are
 * dn_bn_bwd_out.dbias / dn_channel_sum without the fold: the partials stay in the
 * workspace ([c] doubles for the folded sums, then [*n_blocks][c] partials), which must stay untouched until
 * dn_channel_sum_fold_multi has folded it: one launch for every job (32 per launch), each in dn_channel_sum's fixed order --
 * out[ch] = (accumulate ? out[ch] : 0) + (float) sum, the same bits as the undeferred calls. */
typedef struct dn_fold_job {
  const double* partials; /* workspace + c */
  double* sums;           /* workspace: receives the folded doubles */
  float* out;
  int32_t n_blocks, c, accumulate, reserved;
} dn_fold_job;
int dn_channel_sum_partial(const float* x, long rows, int c, int ld, double* sums, size_t sums_bytes, int* n_blocks, void* stream);
int dn_channel_sum_fold_multi(const dn_fold_job* jobs, int n_jobs, void* stream);

/* Does the fused BatchNorm form `form` take this shape?  1 or 0: exactly the shape condition the entry points enforce on the
 * member that selects the form (they ask this function), so a caller can leave that member NULL instead of meeting an error.
 * The tensors' alignment (16 bytes, row strides % 4) is not part of it: the call still checks that.
 *   DN_BN_FORM_SP_APPLY  dn_bn_train_apply's y_sp: one group, c % 16 == 0, c / 4 a power of two, c <= 512,
 *                        rows_per_group * c / 4 < 2^31.  DN_BN_LEGACY=1 does not change it (the SP apply has no general twin).
 *   DN_BN_FORM_BIAS      dn_bn_bwd_out's dbias / n_blocks: one group, c % 4 == 0, c / 4 a power of two, c <= 512,
 *                        rows_per_group * c / 4 < 2^31, DN_BN_LEGACY unset (the one-group fast kernels).
 *   DN_BN_FORM_DZ_NULL   dn_bn_bwd_out's dz = NULL (only the SP copy of dz written): DN_BN_FORM_BIAS and c % 16 == 0.
 * Any other n_groups, a non-positive size or an unknown form: 0. */
enum { DN_BN_FORM_SP_APPLY = 0, DN_BN_FORM_BIAS = 1, DN_BN_FORM_DZ_NULL = 2 };
int dn_bn_train_form_supported(int form, int n_groups, long rows_per_group, int c);

/* tools and tests only: which kernels did the last call of BatchNorm pass `pass` run in this process?  Host side: written by
 * the entry points once nothing can refuse the call any more (a refused call leaves the record as it was), no kernel knows of it;
 * not thread-safe.  Writes up to n of 8 ints and returns 8 (DN_ERR_ARG: null pointer, no room, unknown pass):
 *   [0] kernel class: 0 general (any c, stride, alignment), 1 float4, 2 the one-group fast float4 kernels; -1: no call yet
 *   [1] U: rows (reductions) a thread fetches before it adds them; the running update: groups per fetch (8); an apply: 1
 *   [2] flags: DN_BN_REC_SP the SP copy is written | DN_BN_REC_BIAS the fused bias partials | DN_BN_REC_MASK the byte mask is
 *       written (apply) or read (backward, relu = 2) | DN_BN_REC_DZ_NULL | DN_BN_REC_RUNNING the running update fused into the
 *       finish | DN_BN_REC_ORDER dn_bn_update_running was given `order`
 *   [3] what finished the sums: DN_BN_FOLD_* below (0: the pass has no fold)
 *   [4] workgroups per group of a reduction, the grid of an apply or of a finish
 *   [5] groups  [6] c  [7] the row count the pass normalised by or reduced over, saturated at INT32_MAX
 * DN_BN_PASS_STATS_FINISH is written by dn_bn_train_stats_partial (fold_partials, statistics pending), dn_bn_train_stats_finish
 * and dn_bn_train_stats; DN_BN_PASS_CHANNEL_SUM by dn_channel_sum_partial (deferred) and dn_channel_sum;
 * dn_channel_sum_fold_multi writes DN_BN_PASS_FOLD_MULTI: [1] partials a lane fetches per batch, [4] jobs of its last launch,
 * [5] launches, [6] wavefronts of the last launch. */
enum { DN_BN_PASS_STATS_REDUCE = 0, DN_BN_PASS_STATS_FINISH = 1, DN_BN_PASS_APPLY = 2, DN_BN_PASS_BWD_REDUCE = 3,
       DN_BN_PASS_BWD_APPLY = 4, DN_BN_PASS_CHANNEL_SUM = 5, DN_BN_PASS_RUNNING = 6, DN_BN_PASS_FOLD_MULTI = 7, DN_BN_PASSES = 8 };
enum { DN_BN_REC_SP = 1, DN_BN_REC_BIAS = 2, DN_BN_REC_MASK = 4, DN_BN_REC_DZ_NULL = 8, DN_BN_REC_RUNNING = 16, DN_BN_REC_ORDER = 32 };
enum { DN_BN_FOLD_NONE = 0, DN_BN_FOLD_PARTIALS_FINALIZE = 1, DN_BN_FOLD_STATS_FINISH = 2, DN_BN_FOLD_PARAM_GRAD = 3,
       DN_BN_FOLD_PARTIALS_PARAM_GRAD = 4, DN_BN_FOLD_CHANNEL_SUM = 5, DN_BN_FOLD_DEFERRED = 6, DN_BN_FOLD_MULTI = 7 };
int dn_bn_train_last_form(int pass, int* out, int n);

/* Backward of the decoder's nearest x2 upsample as a pass of its own (only needed where no
 * BatchNorm backward follows directly: the fusion on layer 4): out [n, h, w, c] dense = 2 x 2
 * block sums of g [n, 2h, 2w, c'] read with row stride ld. */
int dn_upsample2_sum(const float* g, int ld, int n_images, int h, int w, int c, float* out,
                     void* stream);

/* a[row][0..c) += b[row][0..c) */
int dn_add_rows(float* a, int ld_a, const float* b, int ld_b, long rows, int c, void* stream);

/* ---- DiscoGraph fusion, training mode ------------------------------------------------------ */

/* z1[p] += e[ego_image[p]] for every pair p (rows_per_image pixels of c channels each) */
int dn_pair_add_ego(float* z1, const float* e, const int* ego_image, int n_pairs,
                    int rows_per_image, int c, void* stream);
/* de[img] = sum of dz1[p] over the pairs listed for img: pairs[first[img] .. first[img + 1]) */
int dn_pair_sum_ego(const float* dz1, const int* first, const int* pairs, int n_images,
                    int rows_per_image, int c, float* de, void* stream);

/* Softmax over a scene-agent's neighbour list and the weighted sum (forward), per pixel:
 *   s_k = relu(z4[pair_k]);  w_k = exp(s_k) / sum_j exp(s_j);  fused = sum_k w_k * maps[nbr_k]
 * lists: for ego e in [0, n_egos): entries first[e] .. first[e+1) of (pair_index, map_image);
 * ego_out[e] = image of `fused` to write.  maps holds own and warped maps in one buffer.
 * pair_index < 0: an entry without a logit (s = 0, no weight written) -- an ego that is not live; it must be its list's only
 * entry (weight 1): the backward takes that weight as 1. */
int dn_fuse_combine(const float* z4, const float* maps, const int* first, const int* pair_index,
                    const int* map_image, const int* ego_out, int n_egos, int hw, int c,
                    float* weights, float* fused, void* stream);
/* backward: dmaps[map_image_k] = w_k * dfused (assignment: every map is in one list),
 * dz4[pair_k] = w_k * (<dfused, map_k> - sum_j w_j <dfused, map_j>) * (z4 > 0) */
int dn_fuse_combine_backward(const float* dfused, int ld_df, const float* z4, const float* weights,
                             const float* maps, const int* first, const int* pair_index,
                             const int* map_image, const int* ego_out, int n_egos, int hw, int c,
                             float* dmaps, float* dz4, void* stream);

/* The reductions of dn_fuse_reduce (disconet_hip.h: DN_FUSE_SUM / MEAN / MAX, the same rules and the same order) over
 * explicit lists of maps the training forward keeps (dn_warp_list wrote the warps): for ego e in [0, n_egos) the entries
 * first[e] .. first[e+1) of map_image, the ego's own map first; fused[ego_out[e]] is written.  A padded ego is a list
 * of one: its map passes through, the same bits. */
int dn_fuse_reduce_lists(const float* maps, const int32_t* first, const int32_t* map_image, const int32_t* ego_out,
                         int n_egos, int hw, int c, int mode, float* fused, void* stream);
/* backward: one row of dmaps per listed map (assignment: every map is in one list) --
 *   sum: dfused;  mean: dfused / (float)len;  max: dfused on the winner of the element under the forward's rule (the
 *   first NaN, else the first maximum; re-derived from `maps`) and 0 elsewhere;  a padded ego's row: dfused.
 * ld: row stride of dfused in floats (a channel slice of a wider map), a multiple of 4.  fused: the forward's result,
 * may be NULL (not read). */
int dn_fuse_reduce_lists_backward(const float* dfused, int ld, const float* maps, const float* fused,
                                  const int32_t* first, const int32_t* map_image, const int32_t* ego_out, int n_egos,
                                  int hw, int c, int mode, float* dmaps, void* stream);

/* `--com agent` over the training lists (disconet_hip.h :: dn_agent_fuse: the same scalars, the same order of every sum):
 * for ego e in [0, n_egos) the entries first[e] .. first[e+1) of (pair_index, map_image), the ego's own map first;
 *   s_k = relu(z4[pair_k]) [hw];  a_k = relu(b5 + sum_p w5[p] s_k[p]);  w_k = softmax over the list;
 *   fused[ego_out[e]] = sum_k w_k * maps[map_image_k], product by product in list order (no fused multiply-add)
 * weights: one float per list entry, at the entry's place in the lists (first[n_egos] floats).  pair_index < 0: an ego
 * that is not live, alone in its list: weight 1, its map passes through.  Two launches; lists of at most 16 entries. */
int dn_agent_combine_lists(const float* z4, const float* w5, const float* b5, const float* maps, const int32_t* first,
                           const int32_t* pair_index, const int32_t* map_image, const int32_t* ego_out, int n_egos, int hw,
                           int c, float* weights, float* fused, void* stream);
/* backward: dmaps[map_image_k] = w_k * dfused[ego_out[e]] (assignment: every map is in one list, every row is written
 * exactly once).  The weights are constants, as upstream's torch.tensor(list of scalars) makes them: nothing flows into
 * z4, w5 or b5.  ld: row stride of dfused in floats, a multiple of 4. */
int dn_agent_combine_lists_backward(const float* dfused, int ld, const float* weights, const int32_t* first,
                                    const int32_t* map_image, const int32_t* ego_out, int n_egos, int hw, int c,
                                    float* dmaps, void* stream);

/* Backward of dn_warp_neighbors for a list of warps: the gradient of warp w (source image
 * src_image[w] in [0, n_src_images), 4x4 pose at poses + 16 * w, row-major, neighbour -> ego) goes
 * back through both bilinear passes and is ADDED to d_src[src_image[w]].  scratch: n_warps maps.
 * rigid != 0 (every pose a rotation + translation, which V2X poses are) on square maps: gather
 * form, deterministic, no atomics.  Otherwise: scatter with float atomics. */
int dn_warp_backward(const float* d_warped, const float* poses, const int* src_image, int n_warps,
                     int n_src_images, int h, int w, int c, int rigid, float* scratch, float* d_src,
                     void* stream);
/* forward over the same list (training keeps every warp, in list order) */
int dn_warp_list(const float* src, const float* poses, const int* src_image, int n_warps, int h,
                 int w, int c, float* warped, void* stream);

/* ---- loss and optimiser --------------------------------------------------------------------- */

/* Focal softmax classification loss + masked smooth-L1 localisation loss, forward and the
 * gradient w.r.t. the logits / box codes in one pass:
 *   cls [n, 2] logits, labels [n, 2] one-hot;  loc, targets [n, code] ; mask [n] (0/1 floats)
 *   loss_cls = sum_n alpha_t (1 - p_t)^gamma (-log p_t) / norm
 *   loss_loc = sum_n mask * sum_code smoothL1_sigma(loc - target) / norm
 * losses: 2 doubles (cls, loc), zeroed by the call. */
int dn_det_loss(const float* cls, const float* labels, const float* loc, const float* targets,
                const float* mask, long n, int code, float alpha, float gamma, float sigma,
                float norm, double* losses, float* dcls, float* dloc, void* stream);

/* The same call with the CORNER localisation loss (Config.loss_type = "corner_loss"; dn_version 150) in place of the
 * smooth-L1: upstream coperception/utils/CoDetModule.py :: corner_loss over bev_box_decode_torch and
 * center_to_corner_box2d_torch for code_type "faf" -- RECALLED, NOT PINNED: upstream's source was not at hand, the contract
 * below is this library's (disconet_amd.train_ops.host_corner_loss states it in torch).
 *   cls, labels [n, 2], mask [n] as above;  loc, targets [n, 6] box codes;  anchors [per_image, 6] rows (x, y, w, h, sin, cos)
 *   as postprocess.make_anchors makes them; anchor i uses the row i % per_image (n % per_image == 0).
 *   1. decode: loc[i] and targets[i] are both decoded against the anchor row a with dn_decode_boxes' expression:
 *      centre (a0 + t0 a2, a1 + t1 a3), size (a2 exp t2, a3 exp t3), pair sin = a4 t5 + a5 t4, cos = a5 t5 - a4 t4.
 *   2. corners: local offsets (+-w/2, +-h/2) in the order (-,-) (+,-) (+,+) (-,+), x = dx cos - dy sin + cx,
 *      y = dx sin + dy cos + cy with the RAW pair (no normalisation: the loss also pulls the pair's length to 1).
 *   3. loss_loc = sum_i mask[i] * sum_{k<4} |pc[i,k] - tc[i,k]|_2 / norm;  dloc = d loss_loc / d loc through 2. and 1.
 *      A corner at distance exactly 0 contributes gradient 0 (never 0/0).  An anchor with mask[i] == 0 contributes nothing,
 *      its dloc row is written as zeros (all rows are written: no memset is needed in front) and its loc / targets / anchor
 *      row are NOT READ: a NaN there does not reach any output.  Nothing is clamped: a non-finite value under mask != 0 gives
 *      a non-finite result.
 *   4. loss_cls and dcls are dn_det_loss's, bit for bit, for the same cls / labels / alpha / gamma / norm.
 * losses: 2 doubles (cls, loc), zeroed by the call, one f64 atomic per workgroup and loss: the reported scalars may differ in
 * their last bits from run to run; dcls and dloc involve no atomics and are the same bits every run, and the same bits from
 * both kernel forms (flat float4 streams for even n and 16-byte aligned cls / labels / loc / targets / dcls / dloc -- dn_det_loss'
 * rule -- else a lane per anchor). */
int dn_det_loss_corner(const float* cls, const float* labels, const float* loc, const float* targets,
                       const float* mask, const float* anchors, long per_image, long n, float alpha,
                       float gamma, float norm, double* losses, float* dcls, float* dloc, void* stream);

/* Knowledge distillation term of CoDetModule.step (kd_flag = 1): for NHWC maps viewed as
 * [rows, c], nn.KLDivLoss(size_average=True)(log_softmax(student, 1), softmax(teacher, 1)) -- the
 * mean over ALL rows * c elements -- times kd_weight: pass scale = kd_weight / (rows * c).
 * *loss (double) is zeroed first if zero_loss, then the term is added; dstudent = d(term)/d(student). */
int dn_kd_kl_loss(const float* student, const float* teacher, long rows, int c, float scale,
                  double* loss, float* dstudent, int zero_loss, void* stream);

/* torch.optim.Adam (no amsgrad) on a flat parameter buffer; step counts from 1.  The hyper-parameters are doubles, as
 * torch keeps them: 1 - beta, the bias corrections and lr / bias_correction1 are formed in double and rounded to float once
 * (dn_version 140; as floats, 1 - 0.999f was 1.3e-5 off). */
int dn_adam_step(float* p, const float* g, float* m, float* v, long n, double lr, double beta1,
                 double beta2, double eps, double weight_decay, int step, void* stream);

#ifdef __cplusplus
}
#endif
#endif
