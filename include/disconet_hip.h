/*
 * disconet_hip.h -- C ABI of libdisconet_hip.so, the MI355X (gfx950) kernels of
 * the coperception `--com disco` detector hot path.
 *
 * The reference has NO FFI for this path: it is pure Python over torch ops
 * (SURVEY.md §2.2, §8(b)); its source is not in the mount
 * (/root/reference/coperception/ is an empty submodule dir,
 * /root/reference/.gitmodules:1-3), so each entry point cites the upstream
 * function it replaces by path (no line numbers exist to cite) and the mounted
 * call sites that reach it: /root/reference/README.md:54-63 (train_codet.py
 * --com disco) and README.md:68-75 (test_codet.py --com disco).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the name ends in _host;
 *   - the caller owns every buffer (incl. workspaces); nothing is allocated,
 *     nothing synchronises; all work is enqueued on `stream` (a hipStream_t
 *     passed as void*, NULL = the default stream);
 *   - activations are channels-last.  Two storage forms: float32 NHWC [image][y][x][channel]
 *     (dn_conv2d*, the warp / fusion kernels' maps, the heads' outputs, everything in
 *     disconet_train.h) and the split-planar "SP" form of the inference conv engine
 *     (dn_spconv2d*, see "SP tensor" below: f16 hi/lo planes, opaque bytes);
 *     dn_sp_from_nhwc / dn_sp_to_nhwc convert.  Images of a batch are agent-major
 *     (image = agent * B + b), the order the reference's tools build with torch.cat over agents;
 *   - ONE stream per device: kernels of this library must not run CONCURRENTLY with each other
 *     (two streams, two graphs in flight).  Beside the split-f16 conv kernels another kernel has
 *     been observed to compute with corrupted VGPR lanes; calls enqueued on
 *     one stream, or ordered by events, are safe;
 *   - return 0 on success, negative on error; dn_last_error() returns a
 *     thread-local message for the last failing call on this thread;
 *   - re-entrant.  Process-wide state is limited to launch-time caches filled on first use
 *     (kernel attributes / occupancy per instantiation), the tools-only hooks dn_spconv_force_config(),
 *     dn_spconv_set_upmode(), dn_spconv_last_form(), dn_spconv_last_resident(), dn_conv_force_config(), dn_conv_last_form(), dn_conv_wgrad_last_form(), dn_bn_train_last_form() (disconet_train.h) and dn_fuse_mlp_set_waves(), and the test switches DN_SP_B3, DN_BN_LEGACY and
 *     DN_WARP_GATHER_LEGACY (environment, read once: the other side of a bitwise / agreement test).
 */
#ifndef DISCONET_HIP_H
#define DISCONET_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DN_OK 0
#define DN_ERR_ARG (-1)
#define DN_ERR_LAUNCH (-2)
#define DN_ERR_UNSUPPORTED (-3)

int dn_version(void);
/* 16 hex digits: SHA-256 over every csrc source / header, include/*.h and the compiler flags the library was built
 * from (disconet_amd/csrc/build.py :: tree_hash).  The Python binding refuses a library whose id differs from the
 * tree it sits in -- a stale .so fails loudly instead of running kernels no commit reproduces. */
const char* dn_build_id(void);
const char* dn_last_error(void);

/* Range guard of the split-f16 engines (dn_spconv2d*, dn_sp_from_nhwc, dn_disco_fuse_mlp).  A value is
 * stored as hi + lo f16 halves, so the format has the f16 EXPONENT range:
 *   - a split clamps at +-65504 (the result then no longer follows the fp32 reference);
 *   - PRECISION FLOOR: `lo = half(x - hi)` is a subnormal once |x| < ~0.125, so below that magnitude an operand
 *     carries an ABSOLUTE error floor of 2^-25 (~3e-8) instead of 2^-22 relative (18 significant bits at
 *     |x| ~ 0.02, 14 at ~1e-3).  Weights are lifted out of that range at pack time by a power of two folded
 *     into the layer's scale (exact); activations are not lifted -- post-ReLU maps of O(1) meet the 1e-4 parity
 *     bar with three orders of margin, maps that are uniformly tiny (|x| << 1e-3) should be rescaled through
 *     their BatchNorm.
 * Every kernel that splits values keeps a sticky word in device memory:
 *   bit 1 (2): a value with |x| > 2^14 was split -- within two binades of the limit, rescale;
 *   bit 0 (1): a value was clamped to +-65504 -- results of this device since the last reset are wrong;
 *   bit 2 (4): a NaN was split by dn_sp_from_nhwc (input) or came out of dn_disco_fuse_mlp (inf / inf in the softmax).
 *              ReLU and the clamp turn a NaN into a finite number, so without this bit it would vanish.  The conv
 *              epilogues do NOT test (it cost ~1 % of the step): out of finite operands they cannot produce a NaN
 *              (overflow is clamped and flagged by bit 0) -- the caller must not pack non-finite weights / scale /
 *              shift (the Python host refuses them when it packs a plan).
 * dn_sp_range_flags: the OR over the library's kernels on the current device; with reset != 0 it clears them.
 *   BLOCKING (hipDeviceSynchronize + a device -> host copy): validation time.  Bit 31 (0x80000000) set = the READ
 *   failed (synchronisation, allocation or copy error): the flags are unknown -- treat as an error, never as "clean"
 *   (the Python host raises).
 * dn_sp_range_flags_async: the same OR enqueued on `stream` into *dst_device (a device word the caller zeroed, or
 *   `reset` bit 1 set: zeroed here first by a kernel launch -- what a CAPTURED step uses, a memset node does not replay
 *   reliably on ROCm 7.2); `reset` bit 0 clears the sticky flags.  No synchronisation, legal inside a stream capture.
 *   A flagged forward's OUTPUTS ARE INVALID (bit 0: clamped values; bit 2: a NaN was turned into a finite number): the
 *   caller must discard them, not only log the flag.  The Python host enqueues it behind a forward, copies the
 *   word to pinned memory and raises at the next call once the copy has landed: the guard is on by default and
 *   costs nothing but four tiny launches (DN_SP_CHECK=0 switches it off, =1 makes every forward block and check). */
unsigned dn_sp_range_flags(int reset);
int dn_sp_range_flags_async(unsigned* dst_device, int reset, void* stream);

/* ------------------------------------------------------------------------
 * K1 -- point cloud -> BEV occupancy.
 * Replaces upstream:coperception/utils/data_util.py :: voxelize_occupy
 * (Appx A.2): strict extent filter on raw floats,
 * floor(xyz / voxel_size) with a float64 divide, index = q - floor(lo/voxel).
 *   pts        [n_pts][pt_stride] float32, x,y,z in columns 0..2
 *   voxel_size_host[3], extents_host[6] = {xlo,xhi,ylo,yhi,zlo,zhi}  (host doubles)
 *   dims_host[3]   = grid dims (X, Y, Z); dense is [X][Y][Z] float32, set to
 *                    0/1 by this call (it zero-fills first).
 * A point with a NaN, infinite or out-of-extent x, y or z fails the strict test and is dropped, as in numpy (the four
 * quiet NaNs dn_lidar_scan writes for a missed ray among them); columns past 2 are never read.
 * ------------------------------------------------------------------------ */
int dn_voxelize_occupy(const float* pts, int n_pts, int pt_stride,
                       const double* voxel_size_host, const double* extents_host,
                       const int* dims_host, float* dense, void* stream);

/* Many clouds under many poses into many grids, ONE launch: the distillation teacher's holistic views (every agent's
 * cloud merged into each ego's frame; the reference's bev_seq_teacher) and, with them or alone, the students' own views.
 * A SOURCE is one cloud under one pose, a VIEW (one output image) the union of its sources.
 *   pts        [n_pts][pt_stride] float32: every cloud, concatenated; x, y, z in columns 0..2, pt_stride >= 3
 *   src_begin, src_count  [n_src] int32 (device): the rows of pts a source reads
 *   src_view   [n_src] int32 (device): the view that receives the source, in [0, n_views)
 *   src_pose   [n_src] int32 (device): index into poses, or -1 = the points are taken as they are
 *   poses      [n_pose][4][4] float32 row-major (trans_matrices [B][A][A][4][4] flattened: no gather is needed)
 *   max_count  the largest src_count (host): it sizes the grid only, a longer source is still read to its end
 *   voxel_size_host, extents_host, dims_host: as dn_voxelize_occupy, with the same dims check
 *   dense      nullable: [n_views][X][Y][Z] float32, 0/1
 *   bits       nullable: [n_views][X][Y] uint32, bit z = height bin z holds a point (dn_scatter_dense_bits' form, Z <= 32)
 * At least one of dense / bits is given; the call zero-fills what it was given, then runs one kernel over all (source,
 * point) pairs: a plain idempotent store into dense, an atomic OR into bits, so duplicated sources, their order and the
 * order of the points cannot change a byte.  No host synchronisation and no allocation: it can be captured into a graph.
 * n_src == 0 zero-fills and returns DN_OK.  A view without sources is all zero.  The lists live on the device, so the
 * host cannot refuse a bad entry: a source whose rows, view or pose index point outside [0, n_pts) / [0, n_views) /
 * [-1, n_pose) writes nothing.
 *
 * THE ARITHMETIC (the contract; the tests are bit-exact against it).  A source with pose T maps a point (x, y, z)
 * (float32) to three coordinates, r = 0, 1, 2:
 *     c_r = float32( ((T[r][0]*x + T[r][1]*y) + T[r][2]*z) + T[r][3] )
 * every operand widened to float64, the sums taken in that order in float64.  A product of two float32 values is exact
 * in float64, so whether the compiler fuses a product into the add that follows cannot change a bit: only the order of
 * the three additions matters (the build has no fast-math flag; keep it that way).  The result is rounded ONCE to
 * float32 -- deliberately: a stored cloud is float32 and the voxel rule compares float32 coordinates.  The float32
 * coordinates then go through exactly dn_voxelize_occupy's rule: strict extent test against the float64 extents,
 * floor(c / voxel) with a float64 divide, minus floor(lo / voxel).  A source with pose -1 skips the transform: a view
 * with that single source is bit for bit dn_voxelize_occupy of its cloud.  NaN and infinite coordinates fail the strict
 * test and are dropped, as in numpy.
 *
 * NOT PINNED to the upstream dataset builder's merge (create_data_det.py is not among the sources this project was
 * written from; what follows is recollection): which poses it uses, whether the ego's own points go through an identity
 * transform, and whether it transforms in float32 or float64.  The contract above is this project's own, in the spirit
 * of SURVEY.md Appendix C; disconet_amd/holistic.py :: host_holistic_views is its numpy statement. */
int dn_voxelize_views(const float* pts, long n_pts, int pt_stride, const int32_t* src_begin, const int32_t* src_count,
                      const int32_t* src_view, const int32_t* src_pose, const float* poses, int n_pose, int n_src,
                      int max_count, int n_views, const double* voxel_size_host, const double* extents_host,
                      const int* dims_host, float* dense, uint32_t* bits, void* stream);

/* Sorted-unique voxel index list of a dense grid, in the reference's
 * lexsort(x, then y, then z) order (= linear order of the [X][Y][Z] grid).
 * A cell is OCCUPIED when dense != 0: any non-zero value, negative ones, float32 subnormals and NaN included; 0.0 and
 * -0.0 are empty (numpy's argwhere(dense != 0)).
 *   indices   [capacity][3] int32 out;  count: int32 out (device)
 *   workspace: dn_voxel_compact_workspace(dims) bytes.
 * count is ALWAYS the number of occupied cells of the grid, whatever the capacity.  When capacity < count the first
 * `capacity` rows of the list are written and nothing from row `capacity` on: the caller compares count with its
 * capacity to learn that the list was cut.  capacity == 0 (indices may then be null) only counts. */
size_t dn_voxel_compact_workspace(const int* dims_host);
int dn_voxel_compact(const float* dense, const int* dims_host, int32_t* indices,
                     int capacity, int32_t* count, void* workspace, void* stream);

/* Replaces upstream:coperception/datasets/V2XSimDet.py :: __getitem__ (dense
 * rebuild) for a whole batch: image g owns rows
 * offsets[g]..offsets[g+1] of indices[.][3]; dense[g][X][Y][Z] = 1 there, else 0.
 *   offsets   [n_images + 1] int32 (device), ascending; an image with offsets[g] == offsets[g+1] is all zero
 * Rows outside [offsets[0], offsets[n_images]) belong to no image and write nothing.  A row whose cell lies outside the
 * grid (a negative coordinate, ix >= X, iy >= Y or iz >= Z) writes nothing either; duplicated rows and the order of the
 * rows cannot change a byte.  The call zero-fills its output first; n_indices_total == 0 leaves it zero. */
int dn_scatter_dense(const int32_t* indices, const int32_t* offsets, int n_images,
                     int n_indices_total, const int* dims_host, float* dense, void* stream);
/* The same rebuild written in the conv engine's split-planar layout (see "SP tensor" below):
 * dense_sp is the SP tensor [n_images][ceil(Z/16)][4][X][Y] x 16 bytes of the bevs batch.  Rows outside
 * [offsets[0], offsets[n_images]) belong to no image and write nothing. */
int dn_scatter_dense_sp(const int32_t* indices, const int32_t* offsets, int n_images,
                        int n_indices_total, const int* dims_host, void* dense_sp, void* stream);
/* ... and as a HI-ONLY SP tensor [n_images][ceil(Z/16)][2 octets][X][Y] x 16 bytes (half the bytes): an
 * occupancy grid is exact in binary16, its lo planes would be all zero.  dn_spconv2d reads it as
 * source 0 of a 3x3 stride-1 layer when dn_conv_desc.math == 3 (half the operand traffic, two MFMAs per
 * product instead of three; the results are bit-identical to the full form).  The same rows as dn_scatter_dense_sp
 * (one kernel writes both forms). */
int dn_scatter_dense_sp_hi(const int32_t* indices, const int32_t* offsets, int n_images,
                           int n_indices_total, const int* dims_host, void* dense_sp_hi, void* stream);
/* ... and as an occupancy BIT grid bits[n_images][X][Y] (uint32; bit z = height bin z holds a point; Z <= 32):
 * 1/32 of the float32 grid ("520 KB/scene as bits").  dn_spconv2d reads it as source 0 of a 3x3
 * stride-1 layer with c_out <= 32 when dn_conv_desc.math == 4: the words are expanded to the hi-only form's halves on
 * their way into LDS, the arithmetic and every result are those of math == 3 on the expanded grid.  Rows outside
 * [offsets[0], offsets[n_images]) belong to no image and write nothing. */
int dn_scatter_dense_bits(const int32_t* indices, const int32_t* offsets, int n_images,
                          int n_indices_total, const int* dims_host, uint32_t* bits, void* stream);

/* ------------------------------------------------------------------------
 * K2/K3/K7 -- implicit-GEMM convolution on fp32 MFMA with fused
 * (bias + eval-BatchNorm) affine and ReLU epilogue.
 * Replaces the conv2d/conv3d(1,1,1) + batch_norm + relu (+ interpolate x2
 * nearest + cat) sequences of upstream:coperception/models/det/backbone/
 * Backbone.py :: Backbone.encode / .decode and of ClassificationHead /
 * SingleRegressionHead (Appx A.6).
 *
 * The logical input is cat([up(src0), src1], channel): src0 has c0 channels
 * and, when up0 != 0, is stored at (h_in/2, w_in/2) and nearest-upsampled x2
 * on the fly; src1 (c1 channels, may be 0/NULL) is at (h_in, w_in).
 * ------------------------------------------------------------------------ */
typedef struct dn_conv_desc {
  int32_t n_images;
  int32_t h_in, w_in;    /* logical conv input size (after the x2 upsample) */
  int32_t c0, c1;        /* channels taken from src0 / src1 */
  int32_t up0;           /* src0 is half resolution, upsample x2 nearest */
  int32_t c_out;
  int32_t ksize;         /* 1 or 3 (padding = ksize/2) */
  int32_t stride;        /* 1 or 2 */
  int32_t relu;          /* apply ReLU after the affine */
  int32_t ld0, ld1, ldo; /* floats per pixel of src0 / src1 / out (>= channels).  With ld > channels the
                            columns beyond a source's own must hold finite values in math 0: the last
                            chunk reads them against zero weights. */
  int32_t math;          /* 0 = exact fp32 MFMA; 1 = split-f16 (x = hi + lo halves, hi*hi + hi*lo +
                            lo*hi on the f16 MFMA, fp32 accumulate, ~2^-22 per product).  The
                            packed weights are math-specific: pack and run with the same value. */
} dn_conv_desc;

/* floats needed for the packed weights of this conv */
size_t dn_conv_packed_weight_floats(const dn_conv_desc* d);
/* weight_oihw: [c_out][c0+c1][ksize][ksize] float32 (torch Conv2d layout; a
 * Conv3d (1,1,1) weight has the same bytes) -> packed tile-major layout. */
int dn_conv_pack_weights(const dn_conv_desc* d, const float* weight_oihw,
                         float* packed, void* stream);
/* scale/shift of y = relu?(acc * scale + shift) from conv bias and BatchNorm
 * running stats; gamma/beta/mean/var may all be NULL (no BN: scale=1,
 * shift=bias); bias may be NULL (0). */
int dn_fold_bn(const float* bias, const float* gamma, const float* beta,
               const float* mean, const float* var, float eps, int channels,
               float* scale, float* shift, void* stream);
int dn_conv2d(const dn_conv_desc* d, const float* src0, const float* src1,
              const float* packed, const float* scale, const float* shift,
              float* out, void* stream);
/* dn_conv2d of a 3x3 layer restricted to the taps of `tap_mask` (bit ky * 3 + kx; the others are skipped, not
 * multiplied by zero) with an explicitly strided output: pixel (oy, ox) of image n is written at
 * out + n * out_img_stride + oy * out_row_stride + ox * out_px_stride floats (+ channel).  The training step's
 * parity-phase stride-2 data gradient (disconet_train.h :: dn_conv_dgrad_class_weights) is four of these. */
int dn_conv2d_taps(const dn_conv_desc* d, const float* src0, const float* src1, const float* packed,
                   const float* scale, const float* shift, float* out, int tap_mask, long out_img_stride,
                   int out_row_stride, int out_px_stride, void* stream);

/* Fused "3x3 conv + affine + ReLU, then 1x1 conv + affine (+ReLU)" in one launch:
 * the activated 64-channel tile stays in LDS between the two layers.  Used for
 * the detection heads (conv1 of the cls and reg heads as one 64-channel conv,
 * their 1x1 conv2 as one block-diagonal second stage with two outputs) and for
 * conv*_2 + the (1,1,1) Conv3D of the encoder -- upstream ClassificationHead /
 * SingleRegressionHead / Backbone.encode.  Split-f16 math,
 * 3x3 stride 1, c_out == 64 only.  Columns [0, split) of the second stage go to
 * out_a (pixel stride ldo_a), columns [split, c_out2) to out_b (ldo_b). */
typedef struct dn_post1x1_desc {
  int32_t c_out2;        /* outputs of the 1x1 stage, multiple of 4, <= 64 */
  int32_t relu2;
  int32_t split;         /* multiple of 4; == c_out2 for a single output */
  int32_t ldo_a, ldo_b;
  int32_t block_diag;    /* dn_spconv2d_post1x1 only (dn_conv2d_post1x1 ignores it): the 1x1 stage is
                            block-diagonal -- outputs [0, split) read stage-1 channels 0..31, the rest
                            channels 32..63 (two detection heads side by side).  Needs out_f32, two
                            outputs, packed2 from dn_sp_post1x1_pack_heads. */
} dn_post1x1_desc;
size_t dn_post1x1_packed_floats(void);
/* w2: [c_out2][c_in2] float32, c_in2 <= 64 = channels of the first stage */
int dn_post1x1_pack_weights(const float* w2, int c_out2, int c_in2, float* packed, void* stream);
int dn_conv2d_post1x1(const dn_conv_desc* d, const dn_post1x1_desc* p, const float* src0,
                      const float* src1, const float* packed, const float* scale,
                      const float* shift, const float* packed2, const float* scale2,
                      const float* shift2, float* out_a, float* out_b, void* stream);

/* ------------------------------------------------------------------------
 * K2/K3/K7, split-planar ("SP") form -- the inference engine's conv path.
 * Same layers and same arithmetic as dn_conv2d with math = 1 (x = hi + lo f16
 * halves, hi*hi + hi*lo + lo*hi on the f16 MFMA, fp32 accumulate), but the
 * activations stay PRE-SPLIT in HBM and are staged by LDS-DMA, so the kernel's
 * loop is ds_read + MFMA only (disconet_amd/csrc/conv_sp.hip, sp_layout.h).
 *
 * SP tensor (opaque bytes, 16-byte aligned, dn_sp_tensor_bytes() long):
 *   [image][ceil(C/16) chunk][4 quarter][H][W] x 16 bytes; a piece = 8 halves =
 *   channels 16*chunk + 8*oct + 0..7 of one pixel; quarter = 2*part + oct,
 *   part 0 = half(x), part 1 = half(x - half(x)).  Channels past C are zero.
 * dn_conv_desc is reused: ld0/ld1/ldo are ignored; up0 is 0 or 1; math is ignored except
 * math == 3: source 0 is a HI-ONLY SP tensor (dn_scatter_dense_sp_hi; 3x3, stride 1, c1 == 0).
 * math == 4: source 0 is an occupancy BIT grid (dn_scatter_dense_bits; 3x3, stride 1, c1 == 0, c0 <= 32, c_out <= 32;
 * DN_ERR_UNSUPPORTED when the layer's weights do not fit the LDS); weights packed as for any other source.
 * Packed weights are specific to this engine (dn_spconv_pack_weights); `wmul`
 * is multiplied into the weights before the split -- pass a power of two that
 * lifts the layer's weights out of the f16 subnormal range and fold 1/wmul into
 * `scale` (exact in fp32).
 * The packed image depends on the layer's SOURCES as well as on its weights: pack
 * with the descriptor the layer will run with.  A 3x3 stride-1 layer whose first
 * source is nearest-upsampled (up0 = 1, c0 a multiple of 16, even h_in / w_in) is
 * packed TAP-MERGED: the kernel taps that read the same low-resolution pixel of
 * that source are summed per output-pixel parity class (16 blocks per 16-channel
 * chunk of source 0 -- 4 merged taps x 4 classes -- instead of 9) and dn_spconv2d
 * runs 2 x 2 taps over those chunks (disconet_amd/csrc/conv_spq.hip).
 * dn_spconv_packed_weight_bytes() accounts for it.
 * ------------------------------------------------------------------------ */
size_t dn_sp_tensor_bytes(int n_images, int h, int w, int channels);
/* fp32 NHWC [n][h][w][ld] (first `channels` of each pixel) <-> SP */
int dn_sp_from_nhwc(const float* src, int n_images, int h, int w, int channels, int ld,
                    void* dst_sp, void* stream);
int dn_sp_to_nhwc(const void* src_sp, int n_images, int h, int w, int channels, int ld,
                  float* dst, void* stream);
size_t dn_spconv_packed_weight_bytes(const dn_conv_desc* d);
int dn_spconv_pack_weights(const dn_conv_desc* d, const float* weight_oihw, float wmul,
                           void* packed, void* stream);
/* Many plain-layout packs in ONE launch (a training step packs every layer's weights once for its forward and once, flipped
 * and transposed, for its data gradient: ~70 launches of 4-7 us on a stream that has nothing else to run beside them).
 * A job packs, for the conv `desc`, the weight tensor W[c_out][c0 + c1][k][k] that a VIEW of `weight` defines:
 *   mode 0: W[n][ci][t] = weight[n][ci_first + ci][t], weight [c_out][cin_total][k][k]
 *           (= dn_spconv_pack_weights; of a column cut when cin_total > c0 + c1)
 *   mode 1: W[n][ci][t] = weight[ci][ci_first + n][k*k - 1 - t], weight [.][cin_total][k][k]
 *           (= dn_conv_dgrad_weights (disconet_train.h) then dn_spconv_pack_weights: the data gradient's conv)
 *   mode 2: W[cls n_in + j] = class (cls / 2, cls % 2) of dn_conv_dgrad_class_weights over column ci_first + j, desc.c_out = 4 n_in
 *           (the one-launch stride-2 data gradient: four classes as output-channel groups)
 * -- the same bytes as those calls write.  dn_spconv_pack_multi_prepare validates the jobs and fills the HOST image of the
 * device table (dn_spconv_pack_multi_table_bytes(n_jobs) bytes; DN_ERR_UNSUPPORTED for a layer that is packed tap-merged);
 * the caller copies it to the device once and calls dn_spconv_pack_weights_multi(table, n_jobs, total_blocks) whenever the
 * weights have changed (a job's wmul is part of the table). */
typedef struct dn_pack_job {
  dn_conv_desc desc;
  const float* weight;
  void* packed;
  int32_t mode, cin_total, ci_first, n_in;
  float wmul;
  int32_t reserved;
} dn_pack_job;
size_t dn_spconv_pack_multi_table_bytes(int n_jobs);
int dn_spconv_pack_multi_prepare(const dn_pack_job* jobs, int n_jobs, void* table_host, int* total_blocks);
int dn_spconv_pack_weights_multi(const void* table_device, int n_jobs, int total_blocks, void* stream);
/* The same for the fp32-NHWC engine's packs (dn_conv_pack_weights; desc.math == 1: the split-f16 rows): modes 0 and 1, and the
 * values are multiplied by the job's wmul first (a power of two: what a caller of dn_conv_pack_weights multiplies in itself). */
size_t dn_conv_pack_multi_table_bytes(int n_jobs);
int dn_conv_pack_multi_prepare(const dn_pack_job* jobs, int n_jobs, void* table_host, int* total_blocks);
int dn_conv_pack_weights_multi(const void* table_device, int n_jobs, int total_blocks, void* stream);
/* out: SP tensor [n_images][ceil(c_out/16)][4][h_out][w_out] */
int dn_spconv2d(const dn_conv_desc* d, const void* src0_sp, const void* src1_sp,
                const void* packed, const float* scale, const float* shift, void* out_sp,
                void* stream);
/* K-SLICED form of dn_spconv2d (3x3 layers; conv_sp.hip / conv_spq.hip `KSL` kernels).  `kslices` (1, 2 or 4) is a
 * property of the LAYER: every output is defined as the fp32 sum, in slice order and starting from zero, of
 * `kslices` accumulation chains over equal shares of the K loop (16-channel chunks; on the tap-merged up-conv equal
 * shares of its work).  How a launch distributes the slices does not change a bit of the result: a workgroup that
 * owns a whole tile folds them in registers, the tiles of the launch's last, under-filled round (every tile of a
 * launch smaller than the chip) are handed out slice by slice through `workspace` and added by a second, tiny launch
 * of the same kernel in the same order.  So the outputs of an image are bit-identical whatever the batch it is part
 * of (tests/test_gpu_conv.py), a 640-tile layer no longer runs two rounds on 512 resident workgroups, and the
 * 4-image launches of an agent-sharded rank fill the chip.  kslices = 1 is dn_spconv2d.  workspace may be NULL
 * (nothing is split) or smaller than dn_spconv_workspace_bytes() (fewer tiles are split).  Same packed weights as
 * dn_spconv2d.  Refused (DN_ERR_ARG): 1x1 layers, hi-only and bit-grid sources (math = 3, 4), the row-merged image
 * (dn_spconv_set_upmode(1)), layers with fewer chunks than slices. */
size_t dn_spconv_workspace_bytes(const dn_conv_desc* d, int kslices);
/* 1 if the layer can run with `kslices` canonical K slices (1, 2 or 4) in this process -- 3x3, no hi-only / bit-grid
 * source, not the row-merged up-conv image (dn_spconv_set_upmode(1)), at least `kslices` 16-channel chunks -- else 0.  Depends on
 * the layer and the process-wide up-conv form only, never on the batch. */
int dn_spconv_ks_supported(const dn_conv_desc* d, int kslices);
int dn_spconv2d_ks(const dn_conv_desc* d, int kslices, const void* src0, const void* src1, const void* packed,
                   const float* scale, const float* shift, void* out, float* out_nhwc /* may be NULL: the second,
                   fp32 NHWC output of dn_spconv2d_dual */, int ld_nhwc,
                   void* workspace, size_t workspace_bytes, void* stream);

/* The encoder stem's first two layers in one launch (conv_pre_1 -> conv_pre_2, both 3x3 + BN + ReLU at the
 * full map): d1 / d2 describe the two layers (3x3, stride 1, one source each; c0 <= 16 -> 32 -> c_out <= 32, same images and
 * map), `bits` is the occupancy bit grid of dn_scatter_dense_bits, packed1 / packed2 the layers' dn_spconv_pack_weights
 * images, out the SP tensor of layer 2.  The intermediate map stays in LDS (it is never written); the result is
 * bit-identical to dn_spconv2d(d1 with math = 4) followed by dn_spconv2d(d2).  dn_spconv2d_pre_pair_supported: 1 if the pair
 * of descriptors fits this form (else DN_ERR_ARG from the launch). */
int dn_spconv2d_pre_pair_supported(const dn_conv_desc* d1, const dn_conv_desc* d2);
int dn_spconv2d_pre_pair(const dn_conv_desc* d1, const dn_conv_desc* d2, const uint32_t* bits, const void* packed1,
                         const float* scale1, const float* shift1, const void* packed2, const float* scale2,
                         const float* shift2, void* out_sp, void* stream);
/* The same conv with a SECOND copy of its output as float32 NHWC rows [n][h_out][w_out][ld_nhwc] (first c_out
 * columns; c_out % 4 == 0), written from the same epilogue registers before the f16 split: the level a
 * consumer outside the conv engine reads (the fusion kernels' maps, the agent all-gather) needs no
 * dn_sp_to_nhwc pass.  (Round 6: also on the tap-merged up-conv kernel, up0 = 1 layers.) */
int dn_spconv2d_dual(const dn_conv_desc* d, const void* src0_sp, const void* src1_sp, const void* packed,
                     const float* scale, const float* shift, void* out_sp, float* out_nhwc, int ld_nhwc,
                     void* stream);
/* dn_spconv2d whose ONLY output is the float32 NHWC copy (no SP tensor is written, nothing is split, no magnitude is
 * tracked): the training step's split-f16 data gradient -- src0 = dz as an SP tensor (dn_bn_bwd_out.dz_sp, disconet_train.h),
 * packed = the flipped / transposed weights, scale = 1 / (sp_lift * wmul), shift = 0, relu = 0 -- and (round 6) the training
 * step's FORWARD convs: src = the previous layer's y as the SP tensor dn_bn_train_apply's y_sp receives, scale = 1 / wmul,
 * shift = bias, out = z (what the BatchNorm statistics read).  Same restrictions as dn_spconv2d_dual. */
int dn_spconv2d_nhwc(const dn_conv_desc* d, const void* src0_sp, const void* src1_sp, const void* packed,
                     const float* scale, const float* shift, float* out_nhwc, int ld_nhwc, void* stream);
/* Fused 3x3 (64 channels) + affine + ReLU, then 1x1 + affine (+ReLU): the 64-channel tile
 * never leaves the registers between the two layers (cf. dn_conv2d_post1x1).
 * out_f32 == 0: out_a is an SP tensor of c_out2 channels (p->split, ldo_* ignored);
 * out_f32 != 0: fp32 NHWC, columns [0, split) -> out_a (ldo_a), the rest -> out_b (ldo_b). */
size_t dn_sp_post1x1_packed_bytes(void);
int dn_sp_post1x1_pack_weights(const float* w2, int c_out2, int c_in2, float wmul, void* packed,
                               void* stream);
/* w2 [c_out2][64] of a block-diagonal stage (see dn_post1x1_desc.block_diag); dn_sp_post1x1_packed_bytes() */
int dn_sp_post1x1_pack_heads(const float* w2, int c_out2, int split, float wmul, void* packed,
                             void* stream);
int dn_spconv2d_post1x1(const dn_conv_desc* d, const dn_post1x1_desc* p, const void* src0_sp,
                        const void* src1_sp, const void* packed, const float* scale,
                        const float* shift, const void* packed2, const float* scale2,
                        const float* shift2, int out_f32, void* out_a, float* out_b, void* stream);
/* tools only: force tile configuration `cfg` (an index of conv_sp.hip's menu) where it
 * applies to the layer, -1 = automatic selection.  Process-wide, not thread-safe. */
int dn_spconv_force_config(int cfg);
/* tools only: form of the packed image / kernel of layers whose first source is upsampled: 0 = plain taps,
 * 1 = row-merged, 2 = row- and column-merged per parity class, -1 = the default (2).  Process-wide; weights packed under one mode must run under the same mode. */
int dn_spconv_set_upmode(int mode);
/* tools and tests only: which kernel did the last SP conv launch of this process run?  Written by the launchers
 * themselves (host side; nothing on the device knows of it).  Fills out[0 .. min(n, 20)) with
 *   0 family (0 = conv_sp_kernel, 1 = conv_spq_kernel: the quad-merged up-conv, 2 = conv_pre_pair_kernel: the stem
 *     pair; -1 = no launch yet)
 *   1..13  KS, STRIDE, TH, TW, BN, TG, CA, POST, BSTAT, UPM, AHI, KSL, NB -- the template parameters of conv_sp.hip's
 *     SpTile (family 1: KS = 3, STRIDE = 1, the 8 x 32 tile, BN, UPM = 2, KSL; family 2: the 16 x 32 tile, BN = 32,
 *     BSTAT = 1, AHI = 2; what a family has no such parameter for is 0)
 *   14 DEEP (family 1: the one-step-per-chunk form)
 *   15 grid, 16 total_items  -- workgroups and work items of the launch (K-sliced: whole tiles + slices)
 *   17 n_whole, 18 n_split   -- K-sliced launches: tiles run whole / handed out slice by slice (else total_items, 0)
 *   19 fixup_grid            -- workgroups of the K-sliced fix-up launch, which belongs to the same record (0: none)
 * and returns 20.  A call that fails its argument checks before the launch leaves the record as it was.
 * Process-wide, not thread-safe (like dn_spconv_force_config). */
int dn_spconv_last_form(int* out, int n);

/* tools and tests only: 1 when the launch that dn_spconv_last_form() describes ran conv_spq_kernel's resident-weights form
 * (BN = 32; the weights of a layer of <= 4 + 2 chunks and c_out <= 32 stay in registers / LDS for the whole launch:
 * dn_spconv_force_config(26), or the dispatch's own choice when such a layer has more work items than CUs), else 0.  The
 * record of dn_spconv_last_form() is the same for both BN = 32 forms. */
int dn_spconv_last_resident(void);

/* tools and tests only, the fp32-NHWC engine (dn_conv2d, dn_conv2d_taps): run tile configuration `cfg` -- a CfgId of
 * conv_mfma.hip: 0 T3_256x32, 1 T3_256x64, 2 T3_128x64, 3 T3_64x64, 4 T3S2_64x64, 5 T1_256x32, 6 T1_256x64,
 * 7 T1_128x128, 8 T1_64x64 -- instead of the cost model's choice; -1 = off.  Honoured only where the id is one of the
 * layer's own candidates (3x3 stride 1: 0..3, 3x3 stride 2: 4, 1x1: 5..8), otherwise the cost model decides as without
 * it; packed weights do not depend on the tile.  dn_conv2d_post1x1 has one form and ignores it.
 * Process-wide, not thread-safe. */
int dn_conv_force_config(int cfg);
/* tools and tests only: which kernel did the last launch of the fp32-NHWC engine run?  Written by the launcher itself
 * (host side).  Fills out[0 .. min(n, 11)) with
 *   0 entry (0 = dn_conv2d, 1 = dn_conv2d_taps, 2 = dn_conv2d_post1x1; -1 = no launch yet)
 *   1..8  KS, STRIDE, TH, TW, BN, KC, MATH, POST -- the template parameters of the conv_mfma_kernel instantiation
 *   9 grid, 10 total_items -- workgroups and work items of the launch (grid < total_items: the persistent loop ran)
 * and returns 11.  A call that fails its argument checks before the launch leaves the record as it was.
 * Process-wide, not thread-safe. */
int dn_conv_last_form(int* out, int n);

/* ------------------------------------------------------------------------
 * K4 -- pose-based two-pass bilinear warp of neighbour feature maps.
 * Replaces upstream:coperception/models/det/base/* :: feature_transformation
 * (+ build_neighbors_feature_list) (Appx A.4): rotate
 * (affine_grid + grid_sample, bilinear, zeros, align_corners=False), zero-pad,
 * then translate by (4*t_x/128, -4*t_y/128) in normalised units.
 *   feat   [A*B][H][W][C]  agent-major layer-`layer` maps
 *   trans  [B][A][A][4][4] float32,  trans[b][i][j] maps j -> i
 *   num_agent [B] int32 live-agent count per sample
 *   ego_first, ego_count: the egos i in [ego_first, ego_first + ego_count) this
 *          call serves (all of them on one GPU: 0, A; one agent per GPU when the
 *          agents of a scene are sharded across ranks).
 *   warped [B][ego_count][A-1][H][W][C]; slot (b, i - ego_first, jj),
 *          jj = j - (j > i), receives warp(j -> i); slots of dead agents are
 *          zero-filled.
 *   only_v2i != 0: only pairs with i == 0 or j == 0 are warped (others zero).
 * ------------------------------------------------------------------------ */
int dn_warp_neighbors(const float* feat, const float* trans, const int32_t* num_agent,
                      int batch, int agents, int h, int w, int c, int only_v2i,
                      int ego_first, int ego_count, float* warped, void* stream);

/* ------------------------------------------------------------------------
 * The parameter-free collaboration baselines `--com sum | mean | max` (upstream SumFusion, MeanFusion, MaxFusion over
 * FusionBase.forward; recalled from upstream, not pinned against its source): the pose warp of
 * every listed neighbour and the reduction over the list in ONE launch -- no warped buffer, no workspace, no atomics, no
 * host synchronisation; graph-capturable and bit-identical from run to run.
 *   feat, trans, num_agent, only_v2i, ego_first, ego_count: as dn_warp_neighbors
 *   mode   DN_FUSE_SUM, DN_FUSE_MEAN or DN_FUSE_MAX
 *   fused  [ego_count*B][H][W][C] float32 NHWC, image (i - ego_first) * B + b
 * The list.  For scene b with n = clamp(num_agent[b], 0, A) live agents and ego i < n: the ego's own map first, then
 * for j = 0 .. n-1, j != i, ascending, the two-pass warp of agent j's map under trans[b][i][j]; only_v2i drops the
 * pairs with i != 0 and j != 0.  (The order of oracle/disconet_ref.py :: DiscoNetRef.forward and train.fusion_lists.)
 * The reductions, per element:
 *   sum   fp32 adds, one after the other in list order (= torch.stack(list).sum(0) on the CPU, bit for bit, for 2..8
 *         maps of a feature map's size)
 *   mean  that sum divided by (float)len(list), an IEEE division (= .mean(0))
 *   max   the first NaN of the list, else its first maximum (= torch.max(dim=0): the first index among ties)
 * A padded ego (i >= n) passes through: fused = its own map, the same bits.  A dead neighbour's map is never read.
 * agents == 1 copies the egos' maps.
 * The warp is dn_warp_neighbors' arithmetic (csrc/warp_device.h: bilinear_taps, sample_src in the order nw, ne, sw, se,
 * the pass-2 blend in tap order); a different kernel gives those values up to the compiler's per-kernel contraction (a
 * few ulp), so nothing promises bit equality with dn_warp_neighbors followed by a reduction.
 * DN_ERR_ARG: c % 4 != 0, a bad ego range, a null pointer, an unknown mode.  c % 64 == 0 (every model): one 8 x 8 tile
 * x 64 channels of one ego image per workgroup, the neighbour loop inside it; other c: one pixel per wave.
 * ------------------------------------------------------------------------ */
#define DN_FUSE_SUM 0
#define DN_FUSE_MEAN 1
#define DN_FUSE_MAX 2
int dn_fuse_reduce(const float* feat, const float* trans, const int32_t* num_agent, int batch, int agents, int h, int w,
                   int c, int only_v2i, int ego_first, int ego_count, int mode, float* fused, void* stream);

/* ------------------------------------------------------------------------
 * K5 tail + K6 -- per-pixel attention MLP tail, softmax over agents, weighted
 * sum.  Replaces PixelWeightedFusionSoftmax.forward layers 2-4 and the fusion
 * loop body of upstream:coperception/models/det/DiscoNet.py :: DiscoNet.forward
 * (Appx A.5).  Layer 1 (1x1 conv 2C -> 128) is split as
 * W1 = [W1_ego | W1_nbr] and evaluated with dn_conv2d:
 *   g      [ego_count*B][H*W][256] = [ x.W1_ego^T + b1 | x.W1_nbr^T ] of the served
 *          egos' own maps (image = (i - ego_first) * B + b)
 *   fw     [B][ego_count][A-1][H*W][128] = warped . W1_nbr^T
 *   feat   [A*B][H*W][C] maps of ALL agents; fused [ego_count*B][H*W][C]
 * The tail computes, per ego i < num_agent[b], per pixel, for neighbours
 * k = ego, then j ascending (j != i):
 *   h1 = relu(bn1(E + F_k)); h2 = relu(bn2(W2 h1 + b2)); h3 = relu(bn3(W3 h2 + b3));
 *   s_k = relu(W4 h3 + b4); w_k = exp(s_k) / sum exp(s_.)   (no max-shift)
 *   fused = sum_k w_k * nbr_k
 * and copies feat for dead agents.  mlp params (device, float32):
 *   bn1_scale/shift[128] (BN affine only, bias b1 is already in E),
 *   w2[32][128], s2/t2[32] (bias+BN folded), w3[8][32], s3/t3[8], w4[8], b4[1].
 * ------------------------------------------------------------------------ */
typedef struct dn_mlp_tail_params {
  const float* bn1_scale; const float* bn1_shift;
  const float* w2; const float* s2; const float* t2;
  const float* w3; const float* s3; const float* t3;
  const float* w4; const float* b4;
} dn_mlp_tail_params;

int dn_disco_fuse_tail(const float* feat, const float* warped, const float* g,
                       const float* fw, const int32_t* num_agent,
                       const dn_mlp_tail_params* p, int batch, int agents, int hw, int c,
                       int only_v2i, int ego_first, int ego_count, float* fused,
                       float* weights_out, /* <- may be NULL; [B][ego_count][A][hw] softmax
                       weights in neighbour-list order */ void* stream);

/* ------------------------------------------------------------------------
 * K5 + K6 in ONE launch (disconet_amd/csrc/fuse_mlp.hip): all four layers of the pairwise
 * attention MLP on the f16 MFMA (split-f16 x3, fp32 accumulate), exp / sum over the agents
 * and the weighted sum, lanes over pixels, no intermediate tensors.  Same semantics, inputs
 * (feat, warped, num_agent, ego range, only_v2i) and neighbour order as dn_disco_fuse_tail;
 * replaces the dn_conv2d (layer 1) + dn_disco_fuse_tail pair for c in {64, 128, 256}.
 *   packed: dn_fuse_mlp_pack() of conv1_1.weight [128][2c] (= [W_ego | W_nbr]),
 *           conv1_2.weight [32][128], conv1_3.weight [8][32]; each matrix is multiplied by
 *           its wmul (a power of two, see dn_spconv_pack_weights) before the f16 split;
 *   s1/t1[128]: y = relu(acc * s1 + t1) after layer 1 (bias, BN and 1/wmul1 folded),
 *   s2/t2[32], s3/t3[8] likewise; w4[8], b4[1] of the last layer (fp32 dot, ReLU).
 *   fused_sp (SP tensor [ego_count*batch][c/16][4][hw] x 16 B) and/or fused_nhwc
 *   ([ego_count*batch][hw][c] float32); weights_out as dn_disco_fuse_tail.
 * ------------------------------------------------------------------------ */
typedef struct dn_fuse_mlp_params {
  const void* packed;
  const float* s1; const float* t1;
  const float* s2; const float* t2;
  const float* s3; const float* t3;
  const float* w4; const float* b4;
} dn_fuse_mlp_params;
int dn_fuse_mlp_supported(int c);
/* tools / tests only: the launch form of dn_disco_fuse_mlp -- 4 (the ego term, the list slots and the channels of the
 * weighted sum of a 32-pixel tile split over four waves: launches of fewer than 512 tiles), 2 (round 5: one wave per
 * tile, workgroups of 2-4 tiles that stage the layer-1 weights in LDS once: 512 tiles and more) or 1 (one wave per
 * tile streaming its weight fragments from L2: rounds 2-4's form for large launches);
 * 0 = chosen per launch (the default).  All forms give bit-identical results.
 * Process-wide, not thread-safe. */
int dn_fuse_mlp_set_waves(int waves);
size_t dn_fuse_mlp_packed_bytes(int c);
int dn_fuse_mlp_pack(const float* w1, const float* w2, const float* w3, int c, float wmul1,
                     float wmul2, float wmul3, void* packed, void* stream);
int dn_disco_fuse_mlp(const float* feat, const float* warped, const int32_t* num_agent,
                      const dn_fuse_mlp_params* p, int batch, int agents, int hw, int c,
                      int only_v2i, int ego_first, int ego_count, void* fused_sp,
                      float* fused_nhwc, float* weights_out, void* stream);
/* FRAGMENT-MAJOR form of the warped neighbour maps (the default of the Python host when h * w % 32 == 0 and
 * c % 64 == 0).  dn_warp_neighbors_fm writes each (sample, ego, neighbour) block of hw * c floats as
 *   [tile t of 32 pixels][k-step ks of 16 channels][half r][lane = 32 h + j] x 4 floats
 *   = channels 16 ks + 8 h + 4 r + 0..3 of pixel 32 t + j
 * -- the order dn_disco_fuse_mlp_fm's wavefronts read it (lane (j, h) of the wave that owns tile t holds exactly these
 * pieces as its MFMA operand), so that every load instruction of a wave is one contiguous 1 KB run instead of 32 half
 * cache lines.  Same values, same arithmetic and same results as dn_warp_neighbors + dn_disco_fuse_mlp; the block is an
 * intermediate between the two calls, nothing else reads it. */
int dn_warp_fm_supported(int h, int w, int c);
int dn_warp_neighbors_fm(const float* feat, const float* trans, const int32_t* num_agent,
                         int batch, int agents, int h, int w, int c, int only_v2i,
                         int ego_first, int ego_count, float* warped_fm, void* stream);
int dn_disco_fuse_mlp_fm(const float* feat, const float* warped_fm, const int32_t* num_agent,
                         const dn_fuse_mlp_params* p, int batch, int agents, int hw, int c,
                         int only_v2i, int ego_first, int ego_count, void* fused_sp,
                         float* fused_nhwc, float* weights_out, void* stream);

/* ------------------------------------------------------------------------
 * `--com agent` (dn_version 149) -- upstream AgentWiseWeightedFusion over FusionBase.forward (recalled
 * from upstream, not pinned against its source): ONE scalar weight per agent of the ego's list, softmax over the list,
 * weighted sum.  The weight net is PixelWeightedFusionSoftmax's four 1x1 layers plus conv1_5 = Conv2d(1, 1, (h, w)), which
 * turns the score map into one scalar.  Upstream builds torch.tensor(list of scalars): the weights are detached, so the net
 * is never trained; this library keeps that (include/disconet_train.h :: dn_agent_combine_lists).
 * Two launches behind dn_warp_neighbors / dn_warp_neighbors_fm (disconet_amd/csrc/agent_fuse.hip): no atomics, no host
 * synchronisation, graph-capturable; the same bits from run to run and in every launch form of dn_fuse_mlp_set_waves.
 *   feat, warped, num_agent, p, batch, agents, hw, c, only_v2i, ego_first, ego_count: as dn_disco_fuse_mlp;
 *   warped_fm != 0: `warped` is dn_warp_neighbors_fm's form (hw % 32 == 0)
 *   w5 [hw] = conv1_5.weight [1][1][h][w] (its kernel is the exchanged map's own size: pixel p = y * w + x), b5 [1]
 *   workspace: dn_agent_fuse_workspace_bytes(batch, agents, ego_count, hw) bytes, 16-byte aligned, owned by the caller;
 *              written and read inside the call, nothing is kept in it
 *   fused [ego_count*B][hw][c] float32 NHWC, image (i - ego_first) * B + b
 *   agent_weights (may be NULL) [B][ego_count][A]: w_k in list order, 0 in unused slots and for a padded ego
 * For scene b with n = clamp(num_agent[b], 0, A) and ego i < n the list is dn_fuse_reduce's: entry 0 the ego's own map,
 * then warp(j -> i) for the live j != i ascending (only_v2i drops the pairs with i != 0 and j != 0); L entries.
 *   scores   s_k[p] = relu(W4 . h3 + b4): exactly dn_disco_fuse_mlp's layers 1-4 on (ego, map_k) -- the same packed weights,
 *            the same folded eval-mode BatchNorm, the self pair (ego, ego) as entry 0
 *   scalar   a_k = relu(b5 + sum_p w5[p] * s_k[p]) in fp32, every product rounded before it is added, in this order: the
 *            pixels in tiles of 32 consecutive p (a pixel past hw contributes +0); within a tile a binary tree over the
 *            pixel's index l in the tile -- l with l + 16, then with l + 8, + 4, + 2, + 1; the tiles' sums one after the
 *            other, ascending, starting from tile 0's sum; then + b5, then the ReLU
 *   softmax  m = max_k a_k;  e_k = expf(a_k - m);  w_k = e_k / sum e, the sum in list order, fp32, IEEE division
 *   fused    sum_k w_k * map_k: each product rounded to fp32 (no fused multiply-add) and added in list order, starting
 *            from the first product.  A list of one entry has w_0 = 1: the ego's own bits.
 * A padded ego (i >= n) passes through, the same bits; a dead neighbour's map is never read; agents == 1 copies (no score
 * launch).  DN_ERR_ARG, before any launch: a null pointer, a bad ego range, a c that dn_fuse_mlp_supported refuses, more
 * than 8 agents, a workspace that is too small, unaligned buffers.
 * fusion_modes.host_agent_fuse states this in plain torch on the CPU.
 * ------------------------------------------------------------------------ */
size_t dn_agent_fuse_workspace_bytes(int batch, int agents, int ego_count, int hw);
int dn_agent_fuse(const float* feat, const float* warped, int warped_fm, const int32_t* num_agent,
                  const dn_fuse_mlp_params* p, const float* w5, const float* b5, int batch, int agents, int hw, int c,
                  int only_v2i, int ego_first, int ego_count, void* workspace, size_t workspace_bytes, float* fused,
                  float* agent_weights, void* stream);


/* ------------------------------------------------------------------------
 * Detection decode (first step after the hot path).
 * Replaces the dense part of upstream:coperception/utils/postprocess.py that
 * CoDetModule.predict_all runs on the CPU: foreground probability = softmax of
 * the 2 class logits, box = anchor-relative decode of the 6-value code
 * (x, y, w, h, sin, cos).  dn_detect below runs top-k + NMS on the GPU and dn_ap_match the per-frame part
 * of mAP; the final precision / recall curve is computed on the host from one copy of the records.
 *   cls [n_images][anchors_per_image][2], loc [n_images][anchors_per_image][6],
 *   anchors [anchors_per_image][6] -> scores [n][apl], boxes [n][apl][6]
 * ------------------------------------------------------------------------ */
int dn_decode_boxes(const float* cls, const float* loc, const float* anchors, int n_images,
                    long anchors_per_image, float* scores, float* boxes, void* stream);

/* ------------------------------------------------------------------------
 * Detection tail (disconet_amd/csrc/detect.hip): per image, the tail of
 * postprocess.host_detections -- top-k anchors by foreground score, rotated greedy NMS -- batched, graph-capturable,
 * with no host synchronisation; the launch sequence depends on the shapes only.
 *   cls, loc, anchors as dn_decode_boxes.  Per image:
 *   - candidates: every anchor (use_score_thr = 0) or those with score > score_thr; a NaN score never is one;
 *   - order: score descending, anchor index ascending (torch.sort(stable=True)); the first min(top_k, #candidates);
 *   - greedy NMS in that order: j is suppressed by an earlier kept i when union > 0 and inter / union > iou_thr
 *     (union = w_i h_i + w_j h_j - inter; fp64 geometry, operation for operation postprocess._intersection_area);
 *   - out: count[n] kept rows; rows < count of boxes [n][top_k][6], scores [n][top_k], index [n][top_k] (anchor
 *     index within the image) in keep order, bit for bit what dn_decode_boxes writes for those anchors; rows >= count
 *     are 0 with index -1, on every call.
 *   1 <= top_k <= 1024, iou_thr finite and >= 0; workspace: dn_detect_workspace_bytes(n, apl, top_k) bytes
 *   (0 for arguments dn_detect refuses); the results are the same bits on every run.
 * ------------------------------------------------------------------------ */
size_t dn_detect_workspace_bytes(int n_images, long anchors_per_image, int top_k);
int dn_detect(const float* cls, const float* loc, const float* anchors, int n_images, long anchors_per_image,
              int top_k, int use_score_thr, float score_thr, double iou_thr, float* boxes, float* scores,
              int32_t* index, int32_t* count, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------
 * Late fusion, `--com late` (disconet_amd/csrc/detect.hip): collaboration at the box level.  Every agent detects from
 * its own view (`--com lowerbound`), sends its detections, and each ego merges them in its own frame and suppresses
 * duplicates.  (What upstream's detection_util :: late_fusion does is recalled, not pinned against its source; the
 * contract below is this library's own, and postprocess.host_late_fuse states it in numpy.)  Graph-capturable behind
 * dn_detect: three kernel launches, no host synchronisation, no allocation, integer arithmetic decides every order; the
 * launch sequence depends on the shapes only and the results are the same bits on every run.
 *   boxes [A*B][k_in][6], scores [A*B][k_in], count [A*B]: dn_detect's outputs or any rows (they need not be sorted),
 *   images agent-major; trans [B][A][A][4][4]: trans[b][i][j] carries agent j's frame into agent i's; num_agent [B]
 *   (clamped to 0..A); only_v2i, ego_first, ego_count as dn_fuse_reduce.
 * Per served ego (i, b), output image (i - ego_first) * B + b:
 *   - the list: [i], then the live j != i ascending (only_v2i drops j != 0 for i != 0); a padded ego (i >= n) has the
 *     list [i] alone; a dead neighbour is never read;
 *   - candidates: the rows r < clamp(count[j*B+b], 0, k_in) of every listed agent whose score is finite and >= 0 (-0
 *     counts and compares equal to +0).  An own row is taken bit for bit.  A neighbour's row is carried with
 *     M = trans[b][i][j], all in fp64 from the fp32 values, every product and every sum rounded on its own:
 *       x' = (M00 x + M01 y) + M03    y' = (M10 x + M11 y) + M13    sin' = M10 cos + M11 sin    cos' = M00 cos + M01 sin
 *     each rounded once to fp32; w, h and the score are copied; the heading is not renormalised (the NMS does that).
 *     With use_extents a neighbour's row is a candidate only when x_lo < x' < x_hi and y_lo < y' < y_hi for the fp32
 *     x', y' (xy_extents_host = {x_lo, x_hi, y_lo, y_hi}, a HOST array read before the launch); own rows are never
 *     filtered;
 *   - order: score descending, then list position ascending, then row ascending; the first min(top_k, #candidates);
 *   - greedy NMS in that order, exactly dn_detect's (inter / union > iou_thr, union > 0, fp64 geometry);
 *   - out: count[n]; rows < count of boxes [E*B][top_k][6], scores [E*B][top_k], source [E*B][top_k] in keep order,
 *     source = j * k_in + r with the agent's own index j; rows >= count are 0 with source -1, on every call.
 *   1 <= top_k <= 1024, 1 <= k_in <= 1024, agents <= 16, agents * k_in <= 8192, iou_thr finite and >= 0, the ego range
 *   inside 0..A, non-empty extents; everything else is DN_ERR_ARG with a message.  workspace:
 *   dn_late_fuse_workspace_bytes(...) bytes (0 for arguments dn_late_fuse refuses).
 * ------------------------------------------------------------------------ */
size_t dn_late_fuse_workspace_bytes(int batch, int agents, int k_in, int top_k, int ego_first, int ego_count);
int dn_late_fuse(const float* boxes, const float* scores, const int32_t* count, const float* trans,
                 const int32_t* num_agent, int batch, int agents, int k_in, int only_v2i, int ego_first, int ego_count,
                 int top_k, double iou_thr, int use_extents, const double* xy_extents_host, float* out_boxes,
                 float* out_scores, int32_t* out_source, int32_t* out_count, void* workspace, size_t workspace_bytes,
                 void* stream);

/* ------------------------------------------------------------------------
 * Detection mAP, per-frame part (disconet_amd/csrc/ap_match.hip): ground-truth matching and true / false positives
 * at up to 8 IoU thresholds for every image of a call, and the append of one record per detection to caller-owned
 * arrays.  Graph-capturable behind dn_detect: kernel launches only, no host synchronisation, no allocation; the launch
 * sequence depends on the shapes only.  Host reference: postprocess.host_match_ground_truth.
 *   boxes [n][k][6], scores [n][k], count [n]: dn_detect's outputs or any rows (they need not be sorted);
 *   gt_boxes [n][g][6], gt_count [n]: padded ground truth.  1 <= k <= 1024, 1 <= g <= 1024, 1 <= n_thr <= 8,
 *   every iou_thrs[t] (a HOST array, read before the launch) in (0, 1].  Counts are clamped to [0, k] / [0, g].
 *   Per image, a row i is valid when i < count and its score is finite:
 *   - rank [n][k]: position in the stable descending score order among the valid rows
 *     (#{q : s_q > s_i or (s_q == s_i and q < i)}); -1 for the other rows;
 *   - best_iou [n][k] (fp64), best_gt [n][k]: the largest IoU over the ground truth that passes the strict
 *     circumscribed-circle test and the lowest column that attains it (IoU as dn_detect's NMS: inter / union, 0 when
 *     union <= 0, fp64 geometry); 0 and -1 when no IoU is above 0 and for rows that are not valid;
 *   - tp [n_thr][n][k] (bytes): 1 when best_iou >= iou_thrs[t] and no row of the image with the same best_gt,
 *     best_iou >= iou_thrs[t] and a lower rank exists; 0 otherwise and for rows that are not valid.
 *   workspace: dn_ap_match_workspace_bytes(n, k, g, n_thr) bytes (0 for arguments dn_ap_match refuses).
 *   Accumulation (records != NULL; NULL skips it and ignores capacity / state / n_agents / batch):
 *   - state: 2 + n_agents 64-bit integers on the device -- [0] cursor = records appended so far (those dropped
 *     included), [1] status: bit 0 = records were dropped because the cursor passed `capacity` (sticky), bit 1 = a row
 *     below count had a non-finite score (sticky; such a row produces no record), [2 + a] ground-truth boxes of agent a
 *     (image / batch: images are agent-major); dn_ap_reset zeroes all of it with one thread;
 *   - records [capacity][2] 32-bit words: {score bits, agent << 8 | tp bit t at bit t}, written at
 *     cursor + (valid rows of the images before this one) + rank: image-major, rank order within an image;
 *   - (n + batch - 1) / batch <= n_agents <= 65536, capacity > 0.
 *   Only integer atomics: two runs write the same bytes.
 * ------------------------------------------------------------------------ */
size_t dn_ap_match_workspace_bytes(int n_images, int k, int g, int n_thr);
int dn_ap_match(const float* boxes, const float* scores, const int32_t* count, const float* gt_boxes,
                const int32_t* gt_count, int n_images, int k, int g, const double* iou_thrs, int n_thr,
                double* best_iou, int32_t* best_gt, int32_t* rank, uint8_t* tp, void* workspace,
                size_t workspace_bytes, void* records, long long capacity, long long* state, int n_agents, int batch,
                void* stream);
int dn_ap_reset(long long* state, int n_agents, void* stream);

/* ------------------------------------------------------------------------
 * Stratified detection AP (disconet_amd/csrc/ap_match.hip, dn_version 153): every ground-truth box carries a stratum and
 * the matching, the records and the counters are kept per stratum.  All three entries are graph-capturable: kernel
 * launches only, no host synchronisation, no allocation; the launch sequence depends on the shapes only.  Host
 * references: postprocess.host_gt_strata, host_match_strata, stratified_ap_from_records.
 *
 * dn_gt_strata: stratum [n][g] int32 of gt_boxes [n][g][6], gt_count [n] (clamped to [0, g]); rows at or beyond the
 *   count get -1.  edges: a HOST array of n_edges doubles (read before the launch), 1 <= n_edges <= 7, finite, positive,
 *   strictly ascending; the stratum of a row is the number of edges it has reached, 0 .. n_edges.
 *   - mode 0, range from the ego: d2 = (double)x * (double)x + (double)y * (double)y, both products and the sum each
 *     rounded on their own; stratum = #{e : d2 >= e2[e]} with e2[e] = edges[e] * edges[e] squared on the host in fp64 and
 *     passed by value (no square root, no division: numpy states the same words).  A row whose x or y is not finite
 *     gets -1.  gt_own_hits may be NULL.
 *   - mode 1, own visibility: gt_own_hits [n][g] int32 (dn_lidar_scan's) is needed, the edges are integers >= 1;
 *     stratum = #{e : own_hits >= edges[e]}.  With the single edge 5 (the lidar scenes' min_points) stratum 0 is
 *     "hidden from the ego" and stratum 1 "seen by the ego itself".
 *
 * dn_ap_match_strata: dn_ap_match's arguments and gt_stratum [n][g] int32, n_strata S in [1, 8] and the optional output
 *   gt_claim [n_thr][n][g] int32 (NULL skips it): the rank of the detection that claimed the box at that threshold, -1
 *   when none did and for rows at or beyond gt_count.  rank, best_iou, best_gt and tp are dn_ap_match's, bit for bit (the
 *   same ap_rank / ap_iou / ap_claim launches; the tp bits come from one device function).  A stratum word of a row
 *   below gt_count outside [-1, S) counts as -1 everywhere.  -1 is a don't-care box: it can be matched and claimed, it is
 *   counted apart, and the metric leaves out the detections that reach it.
 *   workspace: dn_ap_match_strata_workspace_bytes(n, k, g, n_thr, S) bytes (0 for arguments the call refuses).
 *   Accumulation (records != NULL, 16-byte aligned):
 *   - records [capacity][4] 32-bit words, one 16-byte store each, at dn_ap_match's position (cursor + valid rows of
 *     the images before + rank): {score bits, agent << 8 | tp bits, (stratum + 1) << 8 | reach bits, best_gt};
 *     stratum is that of the row's best_gt, -1 when it has none; reach bit t is set when best_gt >= 0 and
 *     best_iou >= iou_thrs[t], whether the row won the claim or is a duplicate;
 *   - state: 2 + n_agents * (S + 1) 64-bit integers -- [0] the cursor, [1] the status: bits 0 and 1 as in dn_ap_match,
 *     bit 2 (sticky) = a row below gt_count carried a stratum outside [-1, S); [2 + a * (S + 1) + s] the ground-truth
 *     boxes of agent a in stratum s, s == S the don't-care boxes.  Counted per image in a workgroup with LDS integer
 *     counters, folded in image order by the advance launch.  dn_ap_strata_reset zeroes all of it.
 *   Only integer atomics: two runs write the same bytes.
 *
 * The metric (evaluated on the host in fp64 from the records, postprocess.stratified_ap_from_records), for a threshold t
 * and a stratum s: a record is LEFT OUT when its reach bit t is set and its stratum is not s (it found a real box of
 * another stratum, or a don't-care box); every other record stays, a true positive when its tp bit t is set (its
 * stratum is then s), a false positive otherwise (duplicates on a box of s, detections that reach nothing).  n_gt is the
 * stratum's counter, recall = TP / n_gt (NaN when n_gt == 0; AP is then 0).  The row "all" leaves out only the records
 * that reach a don't-care box and has the sum of the strata's counters as n_gt.
 * ------------------------------------------------------------------------ */
int dn_gt_strata(const float* gt_boxes, const int32_t* gt_count, const int32_t* gt_own_hits, int n_images, int g, int mode,
                 const double* edges, int n_edges, int32_t* stratum, void* stream);
size_t dn_ap_match_strata_workspace_bytes(int n_images, int k, int g, int n_thr, int n_strata);
int dn_ap_match_strata(const float* boxes, const float* scores, const int32_t* count, const float* gt_boxes,
                       const int32_t* gt_count, const int32_t* gt_stratum, int n_images, int k, int g,
                       const double* iou_thrs, int n_thr, int n_strata, double* best_iou, int32_t* best_gt, int32_t* rank,
                       uint8_t* tp, int32_t* gt_claim, void* workspace, size_t workspace_bytes, void* records,
                       long long capacity, long long* state, int n_agents, int batch, void* stream);
int dn_ap_strata_reset(long long* state, int n_agents, int n_strata, void* stream);

/* ------------------------------------------------------------------------
 * Training targets from ground-truth boxes (disconet_amd/csrc/assign.hip): the anchor assignment that the reference runs
 * on the CPU when it creates the dataset (upstream:tools/det/create_data_det.py; the SECOND / FaF rule, thresholds as
 * parameters), here per training step on the GPU.  Graph-capturable beside the training step: kernel launches only, no
 * host synchronisation, no allocation; the launch sequence depends on the shapes only.  Host reference:
 * targets.host_assign_targets.
 *   anchors [apl][6] = (x, y, w, h, sin, cos) as dn_decode_boxes; gt_boxes [n][g][6], gt_count [n]: padded ground truth,
 *   the arrays dn_ap_match takes.  1 <= n <= 65535, 1 <= apl < 2^31 - 64, 1 <= g <= 1024, 0 < neg_thr <= pos_thr <= 1.
 *   Counts are clamped to [0, g]; rows behind the count are never read.
 *   Per (image, anchor):
 *   - best_iou (fp64): the largest IoU over the rows j < count that pass the strict circumscribed-circle test, best: the
 *     lowest j that attains it (IoU as dn_detect's NMS and dn_ap_match: inter / union, 0 when union <= 0, fp64 geometry,
 *     the anchor's polygon clipped by the box's); 0 and -1 when no IoU is above 0;
 *   - threshold match: positive with target row `best` when best_iou >= pos_thr; negative when best_iou < neg_thr;
 *     don't care otherwise;
 *   - force match (force_match != 0): every row j makes the anchor with the largest IoU against j over all anchors of the
 *     image (the lowest anchor index among equals) positive with target row j, provided that IoU is above 0; this
 *     overrides the anchor's threshold match; of several rows that force one anchor the lowest j wins;
 *   - labels [n][apl][2]: (0, 1) positive, (1, 0) negative, (0, 0) don't care; reg_mask [n][apl]: 1 positive, else 0;
 *     matched_gt [n][apl] (may be NULL): the target row, -1 when not positive; best_iou [n][apl] (may be NULL);
 *   - reg_targets [n][apl][6]: for a positive anchor (xa, ya, wa, ha, sa, ca) with target box (x, y, w, h, sn, cs) and
 *     (s, c) = (sn, cs) / max(hypot(sn, cs), 1e-12) the code dn_decode_boxes inverts,
 *       ((x - xa) / wa, (y - ya) / ha, log(w / wa), log(h / ha), s ca - c sa, c ca + s sa),
 *     computed in fp64 from the fp32 inputs and rounded once to fp32; all zero when not positive.
 *   Every output element is written on every call.  workspace: dn_assign_targets_workspace_bytes(n, apl, g) bytes (0 for
 *   arguments dn_assign_targets refuses).  Only integer atomics: two runs write the same bytes.
 * ------------------------------------------------------------------------ */
size_t dn_assign_targets_workspace_bytes(int n_images, long anchors_per_image, int g);
int dn_assign_targets(const float* anchors, const float* gt_boxes, const int32_t* gt_count, int n_images,
                      long anchors_per_image, int g, double pos_thr, double neg_thr, int force_match, float* labels,
                      float* reg_targets, float* reg_mask, int32_t* matched_gt, double* best_iou, void* workspace,
                      size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------
 * Multi-object tracking behind the detection tail (disconet_amd/csrc/track.hip): one SORT step per image and call --
 * Sort.update of Bewley et al.'s tracker with filterpy's constant-velocity Kalman filter.  What the reference's own
 * tracker computes is recalled, not pinned: this contract is the project's own and
 * tracking.HostSort (numpy / float64) is its normative statement, which the kernel equals bit for bit.
 * Graph-capturable behind dn_detect: one kernel launch, no host synchronisation, no allocation; the launch depends on
 * the shapes only.  Every image of the agent-major batch is its own sequence with its own tracker.
 *   boxes [n][k][6], scores [n][k], count [n]: dn_detect's outputs, 1 <= k <= 1024; counts are clamped to [0, k].
 *   1 <= max_tracks (M) <= 128, max_age >= 0, min_hits >= 0, iou_threshold finite and >= 0, scale finite and > 0.
 *   All arithmetic is fp64 in the order written here, + - * / and sqrt only, never
 *   contracted; a sum over an index runs left to right and starts from its first term.
 *   Measurement.  The four corners of a row (x, y, w, h, sin, cos) as dn_detect's NMS takes them, in fp64 from the fp32
 *   row, with (sin, cos) / max(sqrt(sin sin + cos cos), 1e-12) -- sqrt where postprocess._corners calls hypot, because a
 *   library hypot does not round alike on the host and the device --, each multiplied by `scale`; x1, y1, x2, y2 = their
 *   min / max; w = x2 - x1, h = y2 - y1; z = (x1 + w / 2, y1 + h / 2, w h, w / h).  A row is valid when it is below its
 *   image's count, its score is finite, x1 .. y2 are finite and w > 0, h > 0.  An invalid row below count sets status
 *   bit 1 and is ignored; only the first 128 valid rows in row order are used, a 129th sets status bit 2.
 *   Track: x[7] = (u, v, s, r, u', v', s'), P[7][7], id, age, hits, hit_streak, time_since_update.
 *   R = diag(1, 1, 10, 10), Q = diag(1, 1, 1, 1, .01, .01, .0001), initial P = diag(10, 10, 10, 10, 1e4, 1e4, 1e4),
 *   initial x = (z, 0, 0, 0); rectangle of a state: w = sqrt(s r), h = s / w, (u - w/2, v - h/2, u + w/2, v + h/2).
 *   Per image and call, in this order:
 *   1. frame_count += 1.
 *   2. Predict every track: if x[6] + x[2] <= 0 then x[6] = 0; x[i] += x[i + 4] (i < 3); P: rows 0..2 += rows 4..6,
 *      then columns 0..2 += columns 4..6, then the diagonal += Q (F P F^T + Q in F's sparse form); age += 1; if
 *      time_since_update > 0 then hit_streak = 0; time_since_update += 1.  A track whose rectangle has a non-finite member
 *      is deleted here (the others keep their order).
 *   3. IoU of every surviving track's rectangle a with every valid detection's b: w = min(a2, b2) - max(a0, b0),
 *      h = min(a3, b3) - max(a1, b1); 0 unless w > 0 and h > 0; inter = w h;
 *      union = (a2 - a0)(a3 - a1) + (b2 - b0)(b3 - b1) - inter; inter / union when union > 0, else 0.
 *   4. Associate.  If every row and every column of (iou > iou_threshold) holds at most one true entry, those entries
 *      are the matches.  Otherwise the assignment that maximises the total IoU, by shortest augmenting paths on
 *      cost = -iou: rows are the smaller side (the tracks when T <= D), taken in ascending order; potentials start at 0;
 *      reduced cost = (cost - u[row]) - v[column]; the next column is the unused one with the smallest reduced cost, the
 *      lowest index among equals; a row's search ends after columns + 1 steps at the latest (and leaves the row free),
 *      so the whole takes at most rows x (columns + 1) steps whatever the numbers are.  Either way a pair with
 *      iou < iou_threshold is unmatched.
 *   5. Update each matched track with its detection's z: time_since_update = 0, hits += 1, hit_streak += 1;
 *      y = z - x[:4]; S = P[:4][:4] + R, of which the lower triangle is factored S = L L^T (row by row, column by column,
 *      s = S[i][j] - sum_k<j L[i][k] L[j][k], subtracted one by one; L[i][i] = sqrt(s), L[i][j] = s / L[j][j]);
 *      K = P[:][:4] S^-1 row by row: L w = P[r][:4] forwards, L^T k = w backwards (terms subtracted in ascending k, then
 *      the division); x += K y; A = I - K H; P = (A P) A^T + (K R) K^T (Joseph form), every product a dense sum over
 *      the inner index, (K R)[r][j] = K[r][j] R[j].
 *   6. Deletions are decided: a track with time_since_update > max_age leaves, the others keep their order.  THEN every
 *      unmatched valid detection, in row order, starts a track in the next free slot with id = next_id++ (ids start at
 *      1 per image), hits = hit_streak = age = time_since_update = 0; a birth that finds all M slots taken sets status
 *      bit 0, is dropped and takes no id.  So the slots a frame's deletions free are open to the same frame's births.
 *   7. Report every track of the list with time_since_update < 1 and (hit_streak >= min_hits or frame_count <=
 *      min_hits), in list order (ascending id): out_rect [n][M][4] (fp64, the state's rectangle, scaled units),
 *      out_id [n][M], out_det [n][M] (the detection row it took or was born from this frame), out_score [n][M] (that
 *      row's score), out_count [n].  Rows at or past out_count are 0 with id and det -1, on every call.
 *      det_track [n][k]: the id each detection row was matched to or born as, -1 otherwise.
 *   State (caller-owned, on the device, dn_track_state_bytes(n, M) = n (64 + 480 M) bytes, 0 for refused arguments): per
 *   image 16 int32 {frame_count, next_id, n_tracks, status, 12 x 0}, then M records of 480 bytes {fp64 x[7], P[7][7] row
 *   major; int32 id, age, hits, hit_streak, time_since_update, 3 x 0}; records at or past n_tracks are all zero.  Status
 *   bits are sticky until dn_track_reset, which zeroes everything and sets next_id = 1.  Two runs write the same bytes.
 * ------------------------------------------------------------------------ */
size_t dn_track_state_bytes(int n_images, int max_tracks);
int dn_track_reset(void* state, int n_images, int max_tracks, void* stream);
int dn_track_step(const float* boxes, const float* scores, const int32_t* count, int n_images, int k, int max_tracks,
                  int max_age, int min_hits, double iou_threshold, double scale, void* state, double* out_rect,
                  int32_t* out_id, int32_t* out_det, float* out_score, int32_t* out_count, int32_t* det_track,
                  void* stream);

/* ------------------------------------------------------------------------
 * CLEAR MOT evaluation of the tracks (disconet_amd/csrc/mot_eval.hip): the stage behind dn_track_step -- per image and
 * call one evaluation step of the CLEAR metrics (Bernardin & Stiefelhagen) as the MOT benchmark's evaluation kit computes
 * them.  What the reference's own evaluation computes is recalled, not pinned: this contract is the
 * project's own and tracking.HostClearMot (numpy / float64) is its normative statement, which the kernel equals bit for
 * bit.  Graph-capturable behind dn_track_step: one kernel launch, no host synchronisation, no allocation; the launch
 * depends on the shapes only.  Every image of the agent-major batch is its own sequence.
 *   rect [n][m][4] fp64, id [n][m], count [n]: dn_track_step's report (out_rect, out_id, out_count), 1 <= m <= 128; counts
 *   are clamped to [0, m]; ids are the tracker's (>= 1: the words last and pst below use 0 for "none").
 *   gt_boxes [n][g][6] fp32 rows (x, y, w, h, sin, cos), gt_ids [n][g], gt_count [n], 1 <= g <= 1024; counts are clamped
 *   to [0, g].  scale finite and > 0, iou_threshold in (0, 1], 1 <= max_gt_ids <= 1024.
 *   All arithmetic is fp64 in the order written here, + - * / and sqrt only, never contracted.
 *   Per image and call, in this order:
 *   1. frames += 1.
 *   2. Ground truth, rows below the count in row order.  A row's rectangle is dn_track_step's measurement: the corners
 *      with (sin, cos) / max(sqrt(sin sin + cos cos), 1e-12), each multiplied by `scale`, x1, y1, x2, y2 = their min /
 *      max.  A row whose corners are not all finite or with not (x2 - x1 > 0 and y2 - y1 > 0) is ignored and sets status
 *      bit 2 (value 2).  Else a row whose id is outside 0 .. max_gt_ids - 1 is ignored and sets status bit 4.  Of the
 *      rows left the first 128 are kept; a 129th sets status bit 1.  Of the kept rows, one whose id a lower kept row
 *      carries is dropped and sets status bit 8.  The V rows that remain are the frame's valid ground truth.
 *   3. iou[a][t] of valid ground truth a's rectangle with reported track t's (t < count), dn_track_step's step 3 with the
 *      ground truth as its first rectangle; 0 for a track whose rectangle has a non-finite member.
 *   4. score[a][t] = 0 where iou < iou_threshold (so an IoU equal to the threshold counts); elsewhere iou + 1000.0 when
 *      id[t] equals pst of a's identity, else iou.
 *   5. The assignment that maximises the total score: dn_track_step's shortest-augmenting-path step on cost = -score
 *      (rows the smaller side -- the ground truths when V <= count --, ascending; potentials from 0; the unused column of
 *      smallest reduced cost, the lowest index among equals; a row's search ends after columns + 1 steps).  A pair is
 *      kept only when its score is > 0.
 *   6. Every identity of the image: pst = 0.  Every valid ground truth, in ascending row order: frames_present += 1;
 *      if it holds a kept pair with track t: TP += 1; motp_sum = motp_sum + iou (step 3's value, one pair after the
 *      other in this order); an id switch (IDSW += 1, flag bit 1) when last != 0 and last != id[t]; a segment start
 *      (segments += 1, flag bit 2) when pst was 0 before this call; last = pst = id[t]; frames_matched += 1.
 *   7. FN += V - pairs kept; FP += count - pairs kept.
 *   out_match [n][g]: the track id a ground-truth row took, else -1; out_iou [n][g] fp64: that pair's IoU, else 0;
 *   out_flags [n][g]: bit 0 matched, bit 1 id switch, bit 2 segment start, else 0.  Every word is written on every call.
 *   State (caller-owned, on the device, dn_mot_state_bytes(n, max_gt_ids) = n (64 + 32 max_gt_ids) bytes, 0 for refused
 *   arguments; 8-byte aligned): per image {int64 frames, TP, FP, FN, IDSW; fp64 motp_sum; int32 status; 12 bytes 0}, then
 *   max_gt_ids records of 32 bytes {int32 last, pst, frames_present, frames_matched, segments, 3 x 0}.  Status bits are
 *   sticky until dn_mot_reset, which zeroes everything.  Two runs write the same bytes.
 *   From the state, on the host (tracking.ClearMot.compute): Frag = sum over identities of max(segments - 1, 0); of the
 *   identities with frames_present > 0, frames_matched / frames_present > 0.8 is mostly tracked, < 0.2 mostly lost, else
 *   partly tracked; MOTA = (TP - FP - IDSW) / max(1, TP + FN); MOTP = motp_sum / max(1, TP).
 *   A launch whose score matrix (8 min(g, 128) (m | 1) bytes of LDS) would not fit beside the work arrays is refused.
 * ------------------------------------------------------------------------ */
size_t dn_mot_state_bytes(int n_images, int max_gt_ids);
int dn_mot_reset(void* state, int n_images, int max_gt_ids, void* stream);
int dn_mot_step(const double* rect, const int32_t* id, const int32_t* count, int n_images, int m, const float* gt_boxes,
                const int32_t* gt_ids, const int32_t* gt_count, int g, double scale, double iou_threshold, int max_gt_ids,
                void* state, int32_t* out_match, double* out_iou, int32_t* out_flags, void* stream);

/* ------------------------------------------------------------------------
 * Identity metrics of the tracks (disconet_amd/csrc/idf_eval.hip): IDF1, IDP, IDR (Ristani et al., "Performance measures
 * and a data set for multi-target, multi-camera tracking") and the Count family beside them, as the MOT benchmark's
 * evaluation kit prints them next to CLEAR.  What the reference's own evaluation computes is recalled, not pinned
 * (SURVEY.md section 0): this contract is the project's own and tracking.HostIdentity (numpy) is its normative statement,
 * which the kernels equal bit for bit.  dn_idf_step is graph-capturable behind dn_track_step / dn_mot_step and
 * dn_idf_finish behind it: one kernel launch each, no host synchronisation, no allocation; a launch depends on the
 * shapes only.  Every image of the agent-major batch is its own sequence.
 *   Inputs of dn_idf_step: exactly dn_mot_step's (rect [n][m][4] fp64, id [n][m], count [n], 1 <= m <= 128; gt_boxes
 *   [n][g][6] fp32, gt_ids [n][g], gt_count [n], 1 <= g <= 1024; counts clamped; scale finite and > 0; iou_threshold in
 *   (0, 1]; 1 <= max_gt_ids <= 1024) and 1 <= max_track_ids <= 2048.  Ground-truth ids are 0 .. max_gt_ids - 1, track ids
 *   1 .. max_track_ids (the tracker counts from 1); track id t owns column t - 1.
 *   Per image and call:
 *   1. frames += 1.
 *   2. Ground truth: the V kept rows of dn_mot_step's step 2, by the same rule in the same order (status bits 2, 4, 1, 8
 *      with the same meanings).  Every kept row: gt_count[id] += 1, gt_dets += 1.
 *   3. Reported rows (below the count): a row whose id is outside 1 .. max_track_ids sets status bit 16 and is ignored --
 *      it is counted nowhere.  Every other row: track_count[id - 1] += 1, dets += 1, also when its rectangle has a
 *      non-finite member (a reported box that matches nothing).  The same id on two rows of a frame is counted twice.
 *   4. Every pair (kept ground-truth row a, counted reported row t with a finite rectangle): iou as dn_mot_step's step 3,
 *      fp64, never contracted; when not (iou < iou_threshold): pairs[id_a][id_t - 1] += 1.
 *   out_overlaps [n][g] int32: per ground-truth row the number of such pairs, 0 for a row that was not kept.  Every word
 *   is written on every call.
 *   State (caller-owned, on the device, 4-byte aligned; dn_idf_state_bytes(n, G_ids, T_ids) = n (64 + 4 (G_ids + T_ids +
 *   G_ids T_ids)) bytes, 0 for refused arguments), per image in this order: a 64-byte header {int64 frames, gt_dets, dets
 *   at bytes 0..23; int32 status at bytes 24..27; the rest 0}, int32 gt_count[max_gt_ids], int32
 *   track_count[max_track_ids], int32 pairs[max_gt_ids][max_track_ids] row-major.  All adds are integer adds (the matrix
 *   and track_count by atomics): their result does not depend on the order, two runs write the same bytes.  Status bits
 *   are sticky until dn_idf_reset, which zeroes everything.
 *   dn_idf_finish reads the state and does not write it: it may run after any frame and the sequence may go on.  Rows =
 *   the identities with gt_count > 0, columns = the track ids with track_count > 0, both ascending; the weight of a cell
 *   is its pairs word.  The assignment that maximises the total weight is dn_track_step's shortest-augmenting-path step on
 *   cost = -weight as fp64 (rows the smaller side -- the identities when there are no more of them than track ids --,
 *   ascending; potentials from 0; the unused column of smallest reduced cost, the lowest index among equals; a row's
 *   search ends after columns + 1 steps).  All values are integers below 2^31: every sum is exact.  A pair is kept only
 *   when its weight is > 0; IDTP = the sum of the kept weights.
 *   out_counts [n][8] int64: frames, GT_Dets, Dets, IDTP, GT_IDs (rows), IDs (columns), status, 0.
 *   out_match [n][max_gt_ids] int32: the track id an identity was given, else 0.
 *   From the counts, on the host (tracking.idf_figures), per image, agent and overall, sums in image order: IDFN = GT_Dets
 *   - IDTP, IDFP = Dets - IDTP, IDR = IDTP / max(1, IDTP + IDFN), IDP = IDTP / max(1, IDTP + IDFP), IDF1 = 2 IDTP /
 *   max(1, 2 IDTP + IDFP + IDFN).  The kit's (GT_IDs + IDs)^2 cost matrix with its false-negative / false-positive halves
 *   has the minimum GT_Dets + Dets - 2 IDTP: the plain rectangular matrix gives the same figures.
 *   The finish kernel's work arrays (58.1 KB of LDS, sized for 2049 columns) do not depend on the arguments; a launch
 *   that would not fit 160 KB is refused.
 * ------------------------------------------------------------------------ */
size_t dn_idf_state_bytes(int n_images, int max_gt_ids, int max_track_ids);
int dn_idf_reset(void* state, int n_images, int max_gt_ids, int max_track_ids, void* stream);
int dn_idf_step(const double* rect, const int32_t* id, const int32_t* count, int n_images, int m, const float* gt_boxes,
                const int32_t* gt_ids, const int32_t* gt_count, int g, double scale, double iou_threshold, int max_gt_ids,
                int max_track_ids, void* state, int32_t* out_overlaps, void* stream);
int dn_idf_finish(const void* state, int n_images, int max_gt_ids, int max_track_ids, int64_t* out_counts,
                  int32_t* out_match, void* stream);

/* ------------------------------------------------------------------------
 * HOTA of the tracks (disconet_amd/csrc/hota_eval.hip): the higher-order tracking accuracy (Luiten et al., "HOTA: A Higher
 * Order Metric for Evaluating Multi-Object Tracking") with its detection, association and localisation parts, the third
 * family the MOT benchmark's evaluation kit prints beside CLEAR and identity.  What the kit computes is recalled, not
 * pinned: this contract is the project's own and tracking.HostHota (numpy / float64) is its
 * normative statement, which the kernels equal bit for bit.  The frame matching is weighted by a global alignment score
 * that is known only after the last frame, so the sequence is seen twice: dn_hota_step (graph-capturable behind
 * dn_track_step, one launch) adds the frame to the potential-match matrix and logs its rectangles in the state;
 * dn_hota_finish (graph-capturable, three launches: the zeroing of `work`, the match over a (max_frames, n_images) grid,
 * the fold) matches every logged frame.  No host synchronisation, no allocation; a launch depends on the shapes only.
 *   Inputs of dn_hota_step: dn_idf_step's without a threshold (HOTA has no single IoU threshold), and 1 <= max_frames <=
 *   4096.  Ground-truth ids are 0 .. max_gt_ids - 1, track ids 1 .. max_track_ids; track id t owns column t - 1.
 *   All arithmetic is fp64 in the order written here, + - * / and sqrt only, never contracted.
 *   Alphas: alpha_k = 0.05 * (k + 1) as an fp64 product, k = 0 .. 18.  A pair with IoU s counts at alpha k when
 *   not (s < alpha_k - 2^-52) (the kit's epsilon: without it an IoU of 3/20 misses 0.05 * 3 = 0.15000000000000002).
 *   dn_hota_step, per image and call:
 *   1. frames += 1.  If logged == max_frames: status bit 32 is set and nothing else of this image changes (its
 *      out_potential row is 0); the figures are then those of the first max_frames frames.
 *   2. Ground truth: the V kept rows of dn_mot_step's step 2, by the same rule in the same order (status bits 2, 4, 1, 8).
 *   3. Reported rows below the count, ascending: an id outside 1 .. max_track_ids sets status bit 16 and the row is
 *      ignored; an id that a lower counted row of this frame carries sets status bit 64 and the row is ignored (HOTA matches
 *      one-to-one per id: unlike dn_idf_step a second row is not counted).  The rest are the C <= 128 columns; a column
 *      whose rectangle has a non-finite member stays a column with IoU 0 to everything (a false positive).
 *   4. gt_count[id] += 1 and gt_dets += 1 per kept row; track_count[id - 1] += 1 and dets += 1 per column.
 *   5. s[a][t] is dn_mot_step's step 3.  rs[a] = the sum of s[a][.] over t ascending, cs[t] = the sum of s[.][t] over a
 *      ascending, both from 0.0.  For every pair with s > 0, in (a, t) row-major order:
 *      pot[id_a][id_t - 1] += s / ((rs[a] + cs[t]) - s).  Ids are unique within a frame after steps 2 and 3, so a cell
 *      gets at most one add per call: no atomics, a deterministic result.
 *   6. Log slot `logged` is written, then logged += 1.  A slot is 9232 bytes: int32 V, C and 8 bytes of 0; int32 gid[128],
 *      int32 tid[128]; fp64 gt_rect[128][4], fp64 track_rect[128][4] (the measured rectangles, their bits copied).  Unused
 *      entries stay 0.
 *   out_potential [n][g] fp64: per ground-truth row the sum over t ascending (from 0.0) of the terms it added, 0 for a row
 *   that was not kept.  Every word is written on every call.
 *   State (caller-owned, on the device, 8-byte aligned), per image in this order: a 64-byte header {int64 frames, logged,
 *   gt_dets, dets at bytes 0..31; int32 status at bytes 32..35; the rest 0}, fp64 pot[max_gt_ids][max_track_ids] row-major,
 *   max_frames log slots, int32 gt_count[max_gt_ids], int32 track_count[max_track_ids], padded to a multiple of 8 bytes.
 *   dn_hota_state_bytes is n times that, 0 for refused arguments.  Status bits are sticky until dn_hota_reset, which
 *   zeroes everything.  Two runs write the same bytes.
 *   dn_hota_finish reads the state and never writes it: it may run after any frame and the sequence may go on.  `work` is
 *   scratch of dn_hota_work_bytes (per image 160 + 160 max_frames + 80 max_gt_ids max_track_ids bytes: the per-alpha
 *   TP words, the per-frame loc partials and a 20-bin histogram per cell; 0 for refused arguments), 8-byte aligned; its
 *   contents are unspecified and the call zeroes it itself.  Per image:
 *   1. A[i][j] = pot / ((gt_count[i] + track_count[j]) - pot) where pot > 0, else 0.
 *   2. Every logged frame, independently of the others: s is taken again from the logged rectangles (the same function,
 *      the same bits); score[a][t] = A[gid_a][tid_t - 1] * s[a][t]; dn_track_step's shortest-augmenting-path step on
 *      cost = -score with the row side, the tie rules and the step limit of dn_mot_step's step 5; a pair is kept only when
 *      its score is > 0.  For a kept pair let K be the number of alphas at which it counts (a prefix, the alphas ascend):
 *      hist[gid][tid - 1][K] += 1 (an integer atomic), and for k < K: TP_k += 1, loc_k += s.  Per frame and alpha:
 *      FN_k += V - TP_k(frame), FP_k += C - TP_k(frame).
 *   3. The order of loc_k is two-level so that frames can run in parallel: a frame's partial sum over its kept pairs in
 *      ascending ground-truth row order from 0.0, then the frame partials in ascending slot order from 0.0.
 *   4. Per alpha k the matched count of a cell is c = the sum of its hist bins > k; assa_k = sum of c * (c / ((gt_count +
 *      track_count) - c)), assre_k = sum of c * (c / gt_count), asspr_k = sum of c * (c / track_count): each per identity
 *      over ascending track id from 0.0, then over the identities ascending from 0.0 (a cell with c = 0 adds +0.0).
 *   out_counts [n][8] int64: frames, logged, GT_Dets, Dets, GT_IDs (gt_count > 0), IDs (track_count > 0), status, 0.
 *   out_alpha_counts [n][19][4] int64: TP, FN, FP, 0.  out_alpha_sums [n][19][4] fp64: loc, assa, assre, asspr.
 *   out_match [n][max_frames][128] int32 (may be null): per logged frame and kept ground-truth row, in kept order, the
 *   track id taken, else 0; slots that are not logged hold 0.
 *   From these, on the host (tracking.hota_figures), per image, agent and overall, counts and sums added in image order
 *   (adding the numerators is the kit's TP-weighted combination), per alpha: DetA = TP / max(1, TP + FN + FP), DetRe = TP
 *   / max(1, TP + FN), DetPr = TP / max(1, TP + FP); AssA = assa / max(1, TP), AssRe, AssPr alike; LocA = loc / TP, 1.0
 *   when TP = 0; HOTA = sqrt(DetA * AssA).  Each figure is its mean over the 19 alphas (the fold x = x + v from 0.0,
 *   divided by 19); beside them HOTA(0), LocA(0) and HOTALocA(0) = HOTA(0) * LocA(0) at k = 0.
 *   The match kernel keeps a frame's score matrix in LDS (8 * 128 * 129 bytes beside 17 KB of work arrays, whatever the
 *   arguments are: V and C are read from the log); a launch that would not fit 160 KB is refused.
 * ------------------------------------------------------------------------ */
size_t dn_hota_state_bytes(int n_images, int max_gt_ids, int max_track_ids, int max_frames);
size_t dn_hota_work_bytes(int n_images, int max_gt_ids, int max_track_ids, int max_frames);
int dn_hota_reset(void* state, int n_images, int max_gt_ids, int max_track_ids, int max_frames, void* stream);
int dn_hota_step(const double* rect, const int32_t* id, const int32_t* count, int n_images, int m, const float* gt_boxes,
                 const int32_t* gt_ids, const int32_t* gt_count, int g, double scale, int max_gt_ids, int max_track_ids,
                 int max_frames, void* state, double* out_potential, void* stream);
int dn_hota_finish(const void* state, int n_images, int max_gt_ids, int max_track_ids, int max_frames, void* work,
                   int64_t* out_counts, int64_t* out_alpha_counts, double* out_alpha_sums, int32_t* out_match,
                   void* stream);

/* ------------------------------------------------------------------------
 * BEV rendering (disconet_amd/csrc/render.hip, dn_version 151): every image of a batch rasterised into an RGB canvas on
 * the device -- the scene's occupancy or class map, an optional heat overlay (the DiscoGraph weights), up to 4 sets of
 * rotated boxes.  The result is integer pixels; render.host_render_bev (numpy, float64 and integers) is the normative
 * statement, which the kernel equals in every byte.  Graph-capturable behind dn_detect / dn_track_step: one kernel
 * launch, no atomics, no workspace, no host synchronisation; two runs write the same bytes.
 *   Canvas.  out [n][S h][S w][3] uint8, S = scale in {1, 2, 4}.  Canvas row r belongs to BEV x index r / S, column q to
 *   y index q / S (the layout of bev_seq, no flip); a pixel's centre in canvas units is (r + 0.5, q + 0.5).
 *   DN_ERR_ARG: voxel[0] != voxel[1], voxel not finite and > 0, w % 4 != 0, S outside {1, 2, 4}, n outside 1..65535,
 *   a canvas of 2^31 bytes or more per image, `out` not 4-byte aligned, a null pointer where one is needed, more than 4
 *   sets, a set with k < 1, thickness < 1 or fill_alpha outside 0..255, heat_alpha outside 0..255, heat_hi not > heat_lo
 *   (both finite), h % heat_h != 0 or w % heat_w != 0, an unknown background kind or colour mode.
 *   Background (bg_kind).  DN_RENDER_BG_NONE: every pixel is `ground`.  DN_RENDER_BG_OCCUPANCY: background is
 *   [n][h][w] uint32, the words dn_scatter_dense_bits writes; m = min(popcount(word), 8) and each channel is
 *   (ground (8 - m) + point m + 4) / 8 in integers.  DN_RENDER_BG_CLASSES: background is [n][h][w] int32 labels, palette
 *   [n_classes][3] uint8; a label outside [0, n_classes) gives `ground`.
 *   Heat overlay (heat may be null).  heat [n][heat_h][heat_w] fp32, upsampled nearest: pixel (r, q) reads
 *   heat[(r / S) / (h / heat_h)][(q / S) / (w / heat_w)] = v.  t = ((double)v - heat_lo) / (heat_hi - heat_lo); a NaN
 *   leaves the pixel alone, otherwise t is clamped to [0, 1], l = floor(t 255), a = (heat_alpha l + 127) / 255 and each
 *   channel becomes (below (255 - a) + heat_colour a + 127) / 255 (BLEND, in integers).
 *   Box sets, painted in set order and within a set in ascending row order.  boxes [n][k][6] fp32 = (x, y, w, h, sin,
 *   cos) in metres, the frame and convention of postprocess._corners (local +x is the heading); count [n] (null: k rows;
 *   clamped to [0, k]), scores [n][k], ids [n][k] as the colour mode needs them.
 *   Per row, fp64 from the fp32 members, every product, sum, quotient and root rounded on its own (no contraction):
 *   nrm = sqrt(s s + c c); the row is skipped when a member is not finite, nrm is not > 0, w or h is not > 0;
 *   c' = c / nrm, s' = s / nrm; X = ((x - x_lo) / voxel) S, Y = ((y - y_lo) / voxel) S; A = ((w / 2) / voxel) S,
 *   B = ((h / 2) / voxel) S.  x_lo, y_lo are the lower edges of the extents (make_anchors' origin).
 *   Per pixel, fp64, the same rule: dx = (r + 0.5) - X, dy = (q + 0.5) - Y; u = dx c' + dy s', v = dy c' - dx s';
 *   e = max(|u| - A, |v| - B).  Outline when -thickness < e <= 0: the pixel takes the row's colour.  Heading tick (when
 *   the set has one) when 0 <= u <= A and |v| <= thickness / 2: the same.  Otherwise, when e <= 0 and fill_alpha > 0,
 *   the pixel is BLENDed with the row's colour at a = fill_alpha.
 *   Colour.  DN_RENDER_COLOUR_FIXED: `colour`.  DN_RENDER_COLOUR_SCORE: z = (double)score clamped to [0, 1], a NaN
 *   giving 0; l = floor(z 255); each channel (colour (255 - l) + colour_hi l + 127) / 255.  DN_RENDER_COLOUR_ID: entry
 *   id mod 32 of DN_RENDER_ID_PALETTE; a row with a negative id (Sort's padding) is skipped.
 *   The kernel bins the rows per 32 x 32 tile by a conservative circle test first; the contract is the per-pixel rule
 *   alone.
 * ------------------------------------------------------------------------ */
#define DN_RENDER_MAX_SETS 4
#define DN_RENDER_BG_NONE 0
#define DN_RENDER_BG_OCCUPANCY 1
#define DN_RENDER_BG_CLASSES 2
#define DN_RENDER_COLOUR_FIXED 0
#define DN_RENDER_COLOUR_SCORE 1
#define DN_RENDER_COLOUR_ID 2
/* 32 x (r, g, b) */
#define DN_RENDER_ID_PALETTE { \
  229,34,34, 91,229,131, 107,24,165, 165,153,66, 34,196,229, 229,91,166, 59,165,24, 70,66,165, \
  229,99,34, 91,229,178, 154,24,165, 144,165,66, 34,131,229, 229,91,120, 24,165,36, 103,66,165, \
  229,164,34, 91,229,224, 165,24,130, 111,165,66, 34,66,229, 229,109,91, 24,165,83, 137,66,165, \
  228,229,34, 91,188,229, 165,24,83, 78,165,66, 67,34,229, 229,155,91, 24,165,131, 165,66,161 }

typedef struct dn_render_set {
  const float* boxes;
  const int32_t* count;
  const float* scores;
  const int32_t* ids;
  int32_t k, thickness, fill_alpha, heading, colour_by;
  uint8_t colour[4], colour_hi[4];   /* r, g, b, 0 */
  int32_t reserved;
} dn_render_set;

typedef struct dn_render_desc {
  int32_t n, h, w, scale;
  double x_lo, y_lo, voxel[2];
  const void* background;
  const uint8_t* palette;
  const float* heat;
  int32_t bg_kind, n_classes, heat_h, heat_w, heat_alpha, n_sets;
  double heat_lo, heat_hi;
  uint8_t ground[4], point[4], heat_colour[4];   /* r, g, b, 0 */
  int32_t reserved;
  dn_render_set sets[DN_RENDER_MAX_SETS];
} dn_render_desc;

int dn_render_bev(const dn_render_desc* desc, uint8_t* out, void* stream);

/* ------------------------------------------------------------------------
 * Occlusion-aware lidar scenes (disconet_amd/csrc/lidar.hip, dn_version 152): a spinning lidar's rays cast from every
 * agent's pose against the scene's solids, the nearest hit kept, and the ground truth that somebody in the scene can see.
 * THIS IS THE PROJECT'S OWN SENSOR MODEL, not recalled from upstream: the reference ships CARLA recordings, not a
 * simulator.  lidar.host_scan (numpy, float64) is the normative statement, which the kernels equal in every byte.
 * Graph-capturable: one stream, no host read, nothing allocated; the library's zero-fill launch (solid_hits) and two
 * kernels of its own.  Images are agent-major: image a * S + s is agent a of scene s.
 *   solids            [S][K][8] float64, world frame: x, y, w, l, sin, cos, z_lo, z_hi; the footprint as in gt_boxes (w
 *                     along the heading).  Rows at or beyond solid_count are never read: a NaN there reaches nothing.
 *   solid_count       [S] int32, clamped to [0, K].
 *   object_count      [S] int32, clamped to [0, solid_count]: the first object_count solids are ground-truth candidates,
 *                     the rest are occluders.
 *   sensor_from_world [S][A][4][4] float64 row-major = inverse(agent pose), computed by the host.  The poses are planar
 *                     (synthetic.agent_pose): only T00, T01, T03, T10, T11, T13 are read and the sensor sits at z = 0.
 *   num_agent         [S] int32, the live agents.  A padded agent's image (a >= num_agent[s]) is all misses with zero
 *                     counts and no ground truth.
 *   dirs              [R][3] float64, unit ray directions in the sensor frame (lidar.beam_table): the device evaluates no
 *                     sin or cos.
 *   range_jitter      nullable: [A*S][R] float32 (finite), added to the hit distance.
 * All geometry is fp64, + - * / and comparisons only, every operation rounded on its own (no contraction).
 * THE SCAN, one ray d = (dx, dy, dz) of image (a, s), T = sensor_from_world[s][a].  A solid (x, y, w, l, sn, cs, z_lo,
 * z_hi) is carried into the agent's frame with synthetic.boxes_in_agent_frame's expressions:
 *     cx = (T00 x + T01 y) + T03,  cy = (T10 x + T11 y) + T13,  s = T10 cs + T11 sn,  c = T00 cs + T01 sn.
 * For each solid k ascending the ray (origin 0) is taken into the solid's frame and put through the slab test:
 *     ox = (-cx) c + (-cy) s,  oy = (-cy) c - (-cx) s,  oz = 0;   ex = dx c + dy s,  ey = dy c - dx s,  ez = dz;
 *     slabs [-(w/2), w/2] on x', [-(l/2), l/2] on y', [z_lo, z_hi] on z; per axis t0 = (lo - o) / e, t1 = (hi - o) / e,
 *     tmin = max over axes of min(t0, t1), tmax = min over axes of max(t0, t1) (from -inf / +inf); an axis whose e is
 *     exactly 0 makes no division: it requires lo <= o <= hi instead, else the solid is missed.
 * The solid is hit iff 0 < tmin <= tmax and tmin <= max_range (a sensor inside a solid gets no return from it).  The
 * nearest tmin wins, on a tie the lowest k.  The ground competes as a solid of index -1 that loses ties: for dz < 0,
 * t = ground_z / dz, a candidate iff 0 < t <= max_range.  It competes whatever keep_ground says; with keep_ground = 0 a ray
 * whose nearest return is the ground is reported as a miss.
 *   points     [A*S][R][4] float32 out: float32((t + (double)jitter) d_i) per component (the sensor-frame d), column 3 =
 *              1.0 for a solid and 0.0 for the ground; a miss is four quiet NaNs (0x7fc00000), which
 *              dn_voxelize_occupy and dn_voxelize_views drop by their strict extent test.
 *   hit        [A*S][R] int32 out: k, -1 for the ground, -2 for a miss.
 *   solid_hits [A*S][K] int32 out: the rays of the image whose hit is k (integer atomics: no order dependence).
 * THE VISIBLE GROUND TRUTH, per image, objects k < object_count ascending: the box (cx, cy, w, l, s, c) in the agent's
 * frame by the expressions above is kept iff |cx| < half_extent and |cy| < half_extent (strict, on the fp64 values) and
 * the sum over the scene's LIVE agents of solid_hits[.][k] is >= min_points -- somebody sees it.
 *   gt_boxes    [A*S][G][6] float32 out, compacted in k order, rows at or beyond the count zero; boxes beyond G dropped
 *   gt_count    [A*S] int32 out
 *   gt_own_hits [A*S][G] int32 out: this agent's own returns on each kept box (rows beyond the count zero)
 * DN_ERR_ARG: K outside [0, DN_LIDAR_MAX_SOLIDS] (the LDS table: 256 solids x 64 B), R, S, A or G < 1, A*S > 65535, a null
 * required pointer (solids may be null when K == 0), max_range or half_extent not finite and > 0, ground_z not finite.
 * ------------------------------------------------------------------------ */
#define DN_LIDAR_MAX_SOLIDS 256
int dn_lidar_scan(const double* solids, const int32_t* solid_count, const int32_t* object_count,
                  const double* sensor_from_world, const int32_t* num_agent, const double* dirs, const float* range_jitter,
                  int n_scenes, int n_agents, int k, int n_rays, double max_range, double ground_z, int keep_ground,
                  int min_points, double half_extent, int gt_rows, float* points, int32_t* hit, int32_t* solid_hits,
                  float* gt_boxes, int32_t* gt_count, int32_t* gt_own_hits, void* stream);

/* ------------------------------------------------------------------------
 * Lidar sequences (disconet_amd/csrc/lidar_seq.hip and lidar.hip, dn_version 154): the scan's world at frame f, and the
 * identities of the scan's ground truth.
 *
 * dn_lidar_scan_ids is dn_lidar_scan with one more output through the same two kernels (dn_lidar_scan passes null):
 *   gt_ids [A*S][G] int32 out: the solid index k of each kept row of gt_boxes; rows at or beyond gt_count are -1.
 * Every other output has dn_lidar_scan's bytes.  DN_ERR_ARG: dn_lidar_scan's cases, and a null gt_ids.
 *
 * dn_lidar_world_step moves the world: one launch, grid S (one workgroup per scene), graph-capturable, no host read,
 * nothing allocated.  Motion is closed-form, not integrated: the state at frame f depends on f only, so the world is
 * random-access and lidar.host_world_step (numpy, float64) states it exactly -- the kernel equals it in every byte.
 *   solids0     [S][K][8] float64, the frame-0 rows in dn_lidar_scan's layout
 *   solid_vel   [S][K][2] float64, metres per frame
 *   solid_count [S] int32, clamped to [0, K] as the scan does
 *   agent0      [S][A][4] float64: x, y, sin, cos of each sensor's pose at frame 0
 *   agent_vel   [S][A][2] float64, metres per frame
 *   frame       [S] int32, the cursor, in and out
 * Everything is fp64, + - * only, every operation rounded on its own (no contraction).  t = (double)frame[s].
 * SOLIDS.  Row k < solid_count[s]: x = x0 + t * vx, y = y0 + t * vy (one product and one sum each); columns 2 to 7 are
 * copied as bytes.  A row at or beyond solid_count is the frame-0 row's bytes, all 8 columns, with no arithmetic: a NaN
 * there keeps its payload.
 * SENSORS.  Agent a: x, y as for a solid, (sn, cs) as given; T = sensor_from_world[s][a] = inverse of the planar pose:
 *     T00 = cs,   T01 = sn,  T03 = -((cs * x) + (sn * y)),
 *     T10 = -sn,  T11 = cs,  T13 = (sn * x) - (cs * y),
 *     T22 = T33 = 1, every other entry +0.0.
 * TRANS.  trans[s][i][j] = T_i^-1 T_j in synthetic.make_trans_matrices' layout and meaning.  For i != j, with Ti =
 * sensor_from_world[s][i] and (xj, yj, sj, cj) agent j's pose at the frame:
 *     r00 = Ti00 cj + Ti01 sj,  r01 = Ti01 cj - Ti00 sj,  r03 = (Ti00 xj + Ti01 yj) + Ti03,
 *     r10 = Ti10 cj + Ti11 sj,  r11 = Ti11 cj - Ti10 sj,  r13 = (Ti10 xj + Ti11 yj) + Ti13,
 *     r22 = r33 = 1, the rest 0; each result is rounded once to float32.  i == j is the exact identity.
 * All A agents are computed: the call takes no num_agent (the scan ignores padded agents).
 *   solids            [S][K][8] float64 out
 *   sensor_from_world [S][A][4][4] float64 out
 *   trans             [S][A][A][4][4] float32 out
 * THE CURSOR.  Every lane of workgroup s reads frame[s] before a barrier and lane 0 writes frame[s] + 1 after it; a
 * workgroup touches no other scene's cursor.  A replay of the captured step therefore advances the world with nothing
 * uploaded.  The caller may write the cursor to seek; negative frames are legal and exact.
 * DN_ERR_ARG: K outside [0, DN_LIDAR_MAX_SOLIDS], S or A < 1, a null required pointer (solids0, solid_vel and solids may
 * be null when K == 0).
 * ------------------------------------------------------------------------ */
int dn_lidar_scan_ids(const double* solids, const int32_t* solid_count, const int32_t* object_count,
                      const double* sensor_from_world, const int32_t* num_agent, const double* dirs,
                      const float* range_jitter, int n_scenes, int n_agents, int k, int n_rays, double max_range,
                      double ground_z, int keep_ground, int min_points, double half_extent, int gt_rows, float* points,
                      int32_t* hit, int32_t* solid_hits, float* gt_boxes, int32_t* gt_count, int32_t* gt_own_hits,
                      int32_t* gt_ids, void* stream);
int dn_lidar_world_step(const double* solids0, const double* solid_vel, const int32_t* solid_count, const double* agent0,
                        const double* agent_vel, int32_t* frame, int n_scenes, int n_agents, int k, double* solids,
                        double* sensor_from_world, float* trans, void* stream);

/* ------------------------------------------------------------------------
 * Feature exchange wire format (disconet_amd/csrc/exchange.hip, dn_version 155): what one agent sends the others -- its
 * map of the exchanged pyramid level -- as f16, MXFP8 or MXFP4 instead of fp32.  disconet_amd/exchange.py states the same
 * contract in numpy (host_encode / host_decode); the kernels equal it in every byte.
 *
 * FORMATS.  DN_EXCHANGE_F32 is the identity: no bytes change and there is nothing to launch (dn_exchange_encode /
 * _decode refuse it); it has a message size so that the formats can be compared.
 *
 * MESSAGE of one image [h][w][c] fp32 NHWC, c % 32 == 0: one contiguous range of dn_exchange_message_bytes() bytes, the
 * payload first, then the scale bytes, then zero bytes up to a multiple of 16 (the zeros are part of the contract: the
 * encode launch writes them).  Payload in pixel-major, channel order:
 *   f16    2 bytes per value, little endian; no scales.
 *   mxfp8  1 byte per value.
 *   mxfp4  two values per byte, the lower channel index in the low nibble.
 * Scales: one byte per BLOCK = 32 consecutive channels of one pixel, in [pixel][block] order.  At 32 x 32 x 256 a message
 * is 1 048 576 (f32), 524 288 (f16), 270 336 (mxfp8), 139 264 (mxfp4) bytes.
 *
 * f16: IEEE binary16, round to nearest even, plain conversion (numpy.astype(float16)): overflow gives +-Inf, a NaN stays
 * a NaN.  Decode is the exact widening.
 *
 * mxfp8 / mxfp4: OCP Microscaling v1.0.  Element format E4M3 (e4m3fn: bias 7, largest magnitude 448 = code 0x7E,
 * subnormals mant * 2^-9; emax = 8) or E2M1 (magnitudes 0, .5, 1, 1.5, 2, 3, 4, 6; emax = 2); the block's shared scale is
 * E8M0.  For a block v_0 .. v_31:
 *   - any v_i a NaN or +-Inf: scale byte 0xFF, every element code 0; every value of the block decodes to a NaN;
 *   - else m = max |v_i|, E = floor(log2 m) read from m's fp32 bits (a subnormal m: the position of its leading mantissa
 *     bit), e = max(E - emax, -127), and e = -127 for m == 0.  The scale byte is e + 127;
 *   - element i is v_i * 2^-e, computed exactly, rounded to nearest even as if the element format had no upper exponent
 *     limit, the magnitude then clamped to the format's largest (448 or 6).  The sign bit of v_i is always kept: also
 *     when the magnitude rounds to zero, and for -0.
 * Decode is value(code) * 2^e, and that product is exact in fp32: value(code) is an integer below 16 (below 4) times a
 * power of two, so the product has at most 4 significant bits, and its exponent lies inside fp32's -- the smallest
 * non-zero product is 2^-9 * 2^-127 = 2^-136 >= 2^-149, the largest are 448 * 2^119 < 2^128 and 6 * 2^125 < 2^128 (e <=
 * 127 - emax).  The E4M3 NaN codes 0x7F / 0xFF, which encode never writes, decode to a NaN.
 * Consequences: decode(encode(.)) is idempotent in every bit (a decoded block's maximum keeps E unless it was rounded up
 * to the clamp, and every decoded value is representable under the new scale); per block |x - x'| <= m / 8 for mxfp8 (the
 * worst case is the clamp from 512 to 448 scaled; rounding alone gives m / 16) and <= m / 4 for mxfp4.  The two bounds
 * need a scale above its floor: for m < 2^(emax - 127) -- fp32's own subnormals and the binades just above them, which
 * E8M0 cannot follow -- e stays -127 and the error is at most half the smallest quantum left, 2^-137 (mxfp8) or 2^-129
 * (mxfp4): such a block decodes to zeros with the signs kept.
 *
 *   feat  [n_images][h][w][c] float32 NHWC
 *   wire  [n_images][dn_exchange_message_bytes(format, h, w, c)] bytes: the messages back to back
 * One launch each, graph-capturable, no atomics, no workspace, no host read; every byte of `wire` (of `feat`) is
 * written.  dn_exchange_message_bytes returns DN_ERR_ARG, and the two calls return it before anything is launched, for:
 * c not a positive multiple of 32, a map of 2^31 values or more, an unknown format; the two calls also for
 * DN_EXCHANGE_F32, a null pointer, n_images < 1, and a feat or wire that is not 16-byte aligned.
 * ------------------------------------------------------------------------ */
#define DN_EXCHANGE_F32 0
#define DN_EXCHANGE_F16 1
#define DN_EXCHANGE_MXFP8 2
#define DN_EXCHANGE_MXFP4 3
long dn_exchange_message_bytes(int format, int h, int w, int c);
int dn_exchange_encode(const float* feat, int n_images, int h, int w, int c, int format, uint8_t* wire, void* stream);
int dn_exchange_decode(const uint8_t* wire, int n_images, int h, int w, int c, int format, float* feat, void* stream);

/* ------------------------------------------------------------------------
 * Selective exchange (disconet_amd/csrc/exchange_cells.hip, dn_version 156): an agent sends only the K strongest cells
 * of its map, in any of the four formats above.  disconet_amd/exchange.py states the same contract in numpy (host_select,
 * host_encode_cells, host_decode_cells); the kernels equal it in every byte, with no tolerance anywhere.
 *
 * INPUT.  feat [n_images][h][w][c] fp32 NHWC, c % 32 == 0, P = h * w cells with 1 <= P <= 16384 (one image's scores fit
 * in 64 KiB of LDS), capacity cells = K with 1 <= K <= P.
 *
 * SCORE of cell p: max over its c channels of (bits(v) & 0x7fffffff), as a uint32.  fp32 magnitudes order as their bit
 * patterns, so no float compare and no summation order is involved; Inf and NaN sort at the top, so a poisoned cell is
 * always sent.
 *
 * SELECTION.  Z = number of cells with score > 0.  Order the cells by score descending, then by cell index ascending: the
 * selected cells are the first count = min(K, Z) of that order.  A cell whose values are all +-0 is never sent.  The
 * selected cells are LISTED in ascending cell index: the message is canonical and a receiver can binary-search it.  The
 * selection is the same for all four formats.
 *
 * MESSAGE of one image, one contiguous range of dn_exchange_cells_message_bytes() bytes, every byte written by the
 * encode call:
 *   16 bytes            uint32 count, then three zero words
 *   pad16(2 K) bytes    K uint16 little-endian cell indices p = y * w + x; entries at and beyond count are 0xFFFF; then
 *                       zero bytes up to a multiple of 16
 *   body                exactly the dense message of `format` for the image [1][K][c]: row r is cell index[r] for
 *                       r < count and +0.0 in every channel for r >= count; dn_exchange_message_bytes(format, 1, K, c)
 *                       bytes.  For DN_EXCHANGE_F32 the body is the raw 4 K c bytes.
 * At 32 x 32 x 256, K = 128: 131 344 (f32), 65 808 (f16), 34 064 (mxfp8), 17 680 (mxfp4) bytes.  The capacity is fixed
 * so that the step stays graph-capturable; what a variable-length link would carry for `count` cells is
 *   sent_bytes = 16 + 2 count + count c bits / 8  (+ count c / 32 scale bytes for the MX formats).
 *
 * DECODE.  Every byte of feat is written: cell index[r], for r < min(count, K), gets the dense decode of row r; every
 * other cell is +0.0 in every channel.  An index >= P is skipped.  A wire the encoder cannot have produced (duplicates,
 * not ascending) does not fault; which row wins is then unspecified.  MX blocks are 32 channels of one pixel, so a sent
 * cell decodes to exactly what the dense round trip gives that cell.
 *
 * COUNTS.  sent_cells [n_images] int64, nullable: encode adds each image's count to its word -- one lane per image owns
 * it, a plain read-modify-write: no floating point, no global atomics.
 *
 *   workspace  dn_exchange_cells_workspace_bytes(n_images, h, w) bytes, 16-byte aligned: the scores
 *   wire       [n_images][dn_exchange_cells_message_bytes(format, h, w, c, cells)] bytes, the messages back to back
 * Encode is three launches (score, select, pack), decode one; both are graph-capturable, read nothing back to the host
 * and give the same bytes on every run.  dn_exchange_cells_message_bytes returns DN_ERR_ARG, and the two calls return it
 * before anything is launched, for: c not a positive multiple of 32, P outside [1, 16384], cells outside [1, P], an
 * unknown format; dn_exchange_cells_workspace_bytes for n_images < 1 or P outside [1, 16384]; the two calls also for a
 * null feat / wire / workspace, n_images < 1, a workspace that is too small, and a feat, wire or workspace that is not
 * 16-byte aligned (sent_cells: 8-byte).
 * ------------------------------------------------------------------------ */
#define DN_EXCHANGE_CELLS_MAX 16384
long dn_exchange_cells_message_bytes(int format, int h, int w, int c, int cells);
long dn_exchange_cells_workspace_bytes(int n_images, int h, int w);
int dn_exchange_encode_cells(const float* feat, int n_images, int h, int w, int c, int format, int cells, void* workspace,
                             size_t workspace_bytes, uint8_t* wire, int64_t* sent_cells, void* stream);
int dn_exchange_decode_cells(const uint8_t* wire, int n_images, int h, int w, int c, int format, int cells, float* feat,
                             void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DISCONET_HIP_H */
