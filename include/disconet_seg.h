/*
 * disconet_seg.h -- C ABI of the segmentation variant of `--com disco`
 * (BASELINE.json configs[3]: "DiscoNet seg head, 5-agent, 256x256 BEV").
 *
 * The reference's seg path is upstream:coperception/models/seg/{SegModelBase,DiscoNet}.py +
 * upstream:coperception/utils/SegModule.py, reached by upstream:tools/seg/{train,test}_seg.py;
 * none of it is in the mount (/root/reference/coperception is an empty submodule directory,
 * /root/reference/.gitmodules:1-3) -- the only mounted mention of the task is
 * /root/reference/README.md:15 -- so every entry point cites the upstream call it replaces by path.
 *
 * The UNet's convolutions run on the SP conv engine of disconet_hip.h (dn_spconv2d), the
 * DiscoGraph fusion at the 512-channel bottleneck on dn_warp_neighbors + dn_conv2d (layer 1 of the
 * attention MLP) + dn_disco_fuse_tail.  This header adds the three ops that are new:
 * conventions (device pointers, caller-owned buffers, stream, int status) as disconet_hip.h.
 */
#ifndef DISCONET_SEG_H
#define DISCONET_SEG_H

#include "disconet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* nn.MaxPool2d(2) of the Down blocks (upstream SegModelBase.py :: Down.maxpool_conv[0]) on a
 * split-planar tensor [n][ceil(c/16)][4][h][w] x 16 B -> [n][..][4][h/2][w/2]; h, w even.  The
 * (hi, lo) pair of the largest of the four values is copied: exact. */
int dn_sp_maxpool2(const void* src_sp, int n_images, int h, int w, int channels, void* dst_sp,
                   void* stream);

/* nn.Upsample(scale_factor=2, mode="bilinear", align_corners=True) of the Up blocks
 * (upstream SegModelBase.py :: Up.up), SP in -> SP out [n][..][4][2h][2w]; ATen's lerp order with
 * src = dst * (in - 1) / (out - 1) taken as the exact rational (quotient = tap, remainder = weight,
 * one rounding; dn_version 140), fp32 lerp weights.  The fp32 NHWC forms of the training step
 * (dn_upsample2_bilinear_nhwc / _backward) use the same coordinates. */
int dn_sp_upsample2_bilinear(const void* src_sp, int n_images, int h, int w, int channels,
                             void* dst_sp, void* stream);

/* Label census for the mean reduction of nn.CrossEntropyLoss (ignore_index = -100):
 *   counts[0] = labels in [0, classes)  (the divisor of the mean),
 *   counts[1] = labels that are neither valid nor -100 (torch raises on these; they are treated as
 *               ignored here and reported so that the host can refuse them).
 * counts: 2 device int32, zeroed by the call. */
int dn_seg_label_count(const int32_t* labels, long pixels, int classes, int32_t* counts, void* stream);

/* Per-pixel cross entropy over `classes` logits (upstream SegModule.py :: step,
 * nn.CrossEntropyLoss): logits [pixels][ld] float32, labels [pixels] int32 (outside [0, classes) = ignored).
 *   loss_sum (device double, zeroed by the call) += sum over the live pixels of (logsumexp(z_p) - z_p[y_p])
 *   dlogits [pixels][ld] (may be NULL) = (softmax(z_p) - onehot(y_p)) * g, zero rows for ignored pixels;
 *   g = grad_scale, or grad_scale / counts[0] when `counts` (from dn_seg_label_count, may be NULL) is given:
 *   the reference's mean is over the NON-IGNORED pixels, loss = loss_sum / counts[0]. */
int dn_seg_ce_loss(const float* logits, const int32_t* labels, long pixels, int classes, int ld,
                   float grad_scale, const int32_t* counts, double* loss_sum, float* dlogits, void* stream);

/* Evaluation of the seg variant: the per-pixel prediction and each image's confusion matrix, from which the variant's
 * figure of merit, mean IoU, follows (disconet_amd/seg.py :: MeanIoU.compute).  Upstream's tools/seg/test_seg.py keeps
 * this bookkeeping on the host; its source is not available to this project, so what it computes is RECALLED, NOT PINNED:
 * the contract below is this project's own, stated here and in numpy by seg.HostMeanIoU, which the device equals bit
 * for bit.
 *   logits  [n_images * pixels_per_image][ld] float32, the first `classes` columns are read (dn_seg_ce_loss's layout);
 *           2 <= classes <= 32, ld >= classes.
 *   prediction, per pixel: the index of the first NaN if the row has one, else the index of the first maximum; -0.0 and
 *           +0.0 compare equal; a row of all -inf gives 0.  This is torch.argmax / numpy.argmax (checked on the CPU for
 *           ties, NaN, +-inf and signed zeros): pred == logits.argmax(-1) exactly.
 *   labels  [n_images * pixels_per_image] int32; a label outside [0, classes), the ignore index -100 included, makes
 *           the pixel ignored (as in dn_seg_ce_loss).
 *   live    may be NULL; one byte per image, 0 = every pixel of that image is ignored (upstream drops the empty BEVs of
 *           padded agent slots before the criterion; SegTrainStep.step follows the same rule).
 *   state   [n_images][classes * classes + 1] int64, 8-byte aligned, ACCUMULATED INTO and never zeroed by the call:
 *           state[img][y * classes + p] += #{live pixels of img with label y and prediction p}; the last word counts the
 *           image's ignored pixels.  Integer counts: the order of the atomics does not matter, the result is
 *           deterministic.  It stays on the device for the whole evaluation.
 *   pred    may be NULL; [n_images * pixels_per_image] int32, written for EVERY pixel, ignored ones included.
 * One launch, no host sync, no allocation: it can be captured in a graph behind the forward.  classes == 8 && ld == 8
 * on a 16-byte aligned map reads a row as two 16-byte loads; everything else (ld != classes: rows unaligned) takes the
 * general path with scalar loads.  n_images <= 65535, pixels_per_image <= 2^40. */
int dn_seg_confusion(const float* logits, int ld, const int32_t* labels, const uint8_t* live, int n_images,
                     long pixels_per_image, int classes, int64_t* state, int32_t* pred, void* stream);

/* ---- training forms on float32 NHWC maps (SegModule.step: the UNet's reverse pass; conventions of
 * disconet_train.h -- a gradient argument may be a channel slice of a wider map: pointer at its first
 * channel + the pixel stride ld in floats).  c % 4 == 0, 16-byte aligned buffers. ---- */
/* nn.MaxPool2d(2): x [n][h][w][c] -> y [n][h/2][w/2][c] */
int dn_maxpool2_nhwc(const float* x, int n_images, int h, int w, int c, float* y, void* stream);
/* its backward: dx [n][h][w][c] = dy routed to each window's FIRST maximum in scan order (ATen's recorded
 * index), zero elsewhere; every element written once (no zero fill, deterministic). */
int dn_maxpool2_nhwc_backward(const float* x, const float* dy, int ld_dy, int n_images, int h, int w, int c,
                              float* dx, void* stream);
/* nn.Upsample(x2, bilinear, align_corners=True): x [n][h][w][c] -> y [n][2h][2w][c] */
int dn_upsample2_bilinear_nhwc(const float* x, int n_images, int h, int w, int c, float* y, void* stream);
/* its backward in gather form: dy [n][2h][2w] (stride ld_dy) -> dx [n][h][w][c]; fixed summation order. */
int dn_upsample2_bilinear_nhwc_backward(const float* dy, int ld_dy, int n_images, int h, int w, int c,
                                        float* dx, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DISCONET_SEG_H */
