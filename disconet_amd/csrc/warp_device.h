// Device helpers of the pose warp (upstream:coperception/models/det/base/* :: feature_transformation, SURVEY.md
// Appx A.4) of warp.hip: grid_sample's bilinear tap set and a branch-free bilinear read
// of an NHWC fp32 image through a buffer resource.
#pragma once
#include <hip/hip_runtime.h>

#ifndef DN_F32X4_DEFINED
#define DN_F32X4_DEFINED
typedef float f32x4 __attribute__((ext_vector_type(4)));
#endif

namespace {

struct Bilinear {
  int x0, y0;          // north-west integer tap
  float w_nw, w_ne, w_sw, w_se;
};

// grid_sample(bilinear, align_corners=False) tap set for normalised (gx, gy)
__device__ inline Bilinear bilinear_taps(float gx, float gy, int w, int h) {
  const float ix = ((gx + 1.f) * w - 1.f) * 0.5f;
  const float iy = ((gy + 1.f) * h - 1.f) * 0.5f;
  const float fx = floorf(ix), fy = floorf(iy);
  Bilinear b;
  b.x0 = (int)fx;
  b.y0 = (int)fy;
  const float ex = fx + 1.f, ey = fy + 1.f;  // south-east corner
  b.w_nw = (ex - ix) * (ey - iy);
  b.w_ne = (ix - fx) * (ey - iy);
  b.w_sw = (ex - ix) * (iy - fy);
  b.w_se = (ix - fx) * (iy - fy);
  return b;
}

__device__ inline f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }

// One source image as a buffer resource: every tap load is `buffer_load_dwordx4` with a 32-bit
// byte offset, like the conv engine's operand loads (no 64-bit address arithmetic per tap).
struct SrcImage {
  __amdgpu_buffer_rsrc_t rsrc;
};
__device__ inline SrcImage make_src_image(const float* base, size_t bytes) {
  return SrcImage{__builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(base), 0, (int)bytes, 0x00020000)};
}
__device__ inline f32x4 ldb4(const SrcImage& s, unsigned byte_off) {
  return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(s.rsrc, byte_off, 0, 0));
}

// bilinear sample of src (one image, [h][w][c]) at taps b, channels c4*4..+3.
// Branch-free: every tap is loaded from a clamped in-frame address and its weight
// is zeroed when the tap is outside, so the 4 loads (16 per output pixel) issue
// back to back instead of draining vmcnt at every divergent join.  A zero weight
// times a finite in-frame value is exactly the zero padding.
__device__ inline f32x4 sample_src(const SrcImage& src, const Bilinear& b, int w, int h, int c,
                                   int c4) {
  const bool x0ok = b.x0 >= 0 && b.x0 < w, x1ok = b.x0 + 1 >= 0 && b.x0 + 1 < w;
  const bool y0ok = b.y0 >= 0 && b.y0 < h, y1ok = b.y0 + 1 >= 0 && b.y0 + 1 < h;
  const int x0 = min(max(b.x0, 0), w - 1), x1 = min(max(b.x0 + 1, 0), w - 1);
  const int y0 = min(max(b.y0, 0), h - 1), y1 = min(max(b.y0 + 1, 0), h - 1);
  const unsigned lane_off = 16u * c4;
  const f32x4 v_nw = ldb4(src, (unsigned)((y0 * w + x0) * c) * 4u + lane_off);
  const f32x4 v_ne = ldb4(src, (unsigned)((y0 * w + x1) * c) * 4u + lane_off);
  const f32x4 v_sw = ldb4(src, (unsigned)((y1 * w + x0) * c) * 4u + lane_off);
  const f32x4 v_se = ldb4(src, (unsigned)((y1 * w + x1) * c) * 4u + lane_off);
  // order matches torch's CPU kernel: nw, ne, sw, se
  f32x4 acc = v_nw * ((y0ok && x0ok) ? b.w_nw : 0.f);
  acc += v_ne * ((y0ok && x1ok) ? b.w_ne : 0.f);
  acc += v_sw * ((y1ok && x0ok) ? b.w_sw : 0.f);
  acc += v_se * ((y1ok && x1ok) ? b.w_se : 0.f);
  return acc;
}

// The pose of one warp (4x4 row-major, neighbour -> ego) as the terms of the two passes, and their tap sets: pass 1 rotates
// (rotated pixel q reads the source map), pass 2 translates (output pixel p reads the rotated map).  Shared by every
// kernel of warp.hip and fuse_reduce.hip.
struct PoseTerms {
  float r00, r01, r10, r11, x_trans, y_trans;
};
__device__ inline PoseTerms pose_terms(const float* m) {
  return PoseTerms{m[0], m[1], m[4], m[5], (4.f * m[3]) / 128.f, -(4.f * m[7]) / 128.f};
}
__device__ inline Bilinear pass2_taps(const PoseTerms& t, int px, int py, int w, int h) {
  const float bx = (2.f * px + 1.f) / w - 1.f;
  const float by = (2.f * py + 1.f) / h - 1.f;
  return bilinear_taps(bx + t.x_trans, by + t.y_trans, w, h);
}
__device__ inline Bilinear pass1_taps(const PoseTerms& t, int qx, int qy, int w, int h) {
  const float qbx = (2.f * qx + 1.f) / w - 1.f;
  const float qby = (2.f * qy + 1.f) / h - 1.f;
  return bilinear_taps(t.r00 * qbx + t.r01 * qby, t.r10 * qbx + t.r11 * qby, w, h);
}

// ---- per-pixel form: both passes for ONE output pixel (px, py) and one float4 of channels (c4).  The two resampling passes
// cannot be merged algebraically (the rotated map is zero-padded before it is translated; SURVEY.md Appx A.4), but the
// intermediate map need not exist: out2(p) reads <= 4 integer pixels q of the rotated map, and each in-frame out1(q) is
// re-derived from <= 4 source taps with exactly the per-element arithmetic of the two-pass form (a q outside the frame is the
// zero padding: its weight is zeroed).  The tap sets depend on the pixel only: in a channel loop the compiler hoists them.
__device__ inline f32x4 warp_pixel(const SrcImage& src, const PoseTerms& t, int px, int py, int w, int h, int c, int c4) {
  const Bilinear t2 = pass2_taps(t, px, py, w, h);
  const float qw[4] = {t2.w_nw, t2.w_ne, t2.w_sw, t2.w_se};
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int qx = t2.x0 + (k & 1), qy = t2.y0 + (k >> 1);
    const bool qok = qx >= 0 && qx < w && qy >= 0 && qy < h;
    acc += sample_src(src, pass1_taps(t, qx, qy, w, h), w, h, c, c4) * (qok ? qw[k] : 0.f);
  }
  return acc;
}

// ---- tile-shared form of the same two passes.  Every output pixel p of an 8x8 tile reads the four rotated-map pixels
// q = (x0(p) + {0,1}, y0(p) + {0,1}); the translation is one offset per (ego, neighbour) pair, so the tile's q pixels form a
// (T+1)^2 block (T+2 allowed for a rounding split of floor()).  The rotated map R(q) of that block is computed ONCE per
// workgroup into LDS (4 taps of the source map each, with sample_src's arithmetic) and the tile's 64 outputs are blended from
// LDS with the per-pixel weights of the per-pixel form -- the same values in the same order, with ~3x fewer L2 tap reads (the
// per-pixel form re-derives every R(q) four times and is bound by L2 -> L1 bandwidth, ~1.3 GB per step).  A workgroup of 256
// threads covers one 64-channel slice of the tile, sixteen lanes (l = tid & 15, a float4 each) per pixel: 100 x 256 B =
// 25.6 KB of LDS for R.
//
// The tap sets depend on the pixel only, and sixteen lanes share a pixel: computed ONCE per pixel into LDS (clamped byte
// offsets / LDS rows and validity-masked weights, the expressions of sample_src and of warp_pixel), then every lane does loads
// and FMAs only.  Round 3's form re-derived them in every lane: 1290 VALU instructions per wave, half of the launch's wave
// cycles stalled on VALU issue (profiles/r04_fuse_pmc.txt).  Same values, same order of operations.
//
// The steps of one (tile, source image, pose), a workgroup barrier between each two (and one before the tables of a
// further source image are filled: the last blend reads them):
//   warp_tile_fill_taps | warp_tile_rotate | warp_tile_blend per output pixel
constexpr int WARP_T = 8, WARP_Q = WARP_T + 2, WARP_CS = 64;
typedef unsigned u32x4w __attribute__((ext_vector_type(4)));
typedef int i32x4w __attribute__((ext_vector_type(4)));

struct WarpTile {
  f32x4 rot[WARP_Q * WARP_Q][WARP_CS / 4];
  __attribute__((aligned(16))) unsigned tap1_off[WARP_Q * WARP_Q][4];
  __attribute__((aligned(16))) float tap1_w[WARP_Q * WARP_Q][4];
  __attribute__((aligned(16))) int tap2_row[WARP_T * WARP_T][4];
  __attribute__((aligned(16))) float tap2_w[WARP_T * WARP_T][4];
};

__device__ inline void warp_tile_fill_taps(WarpTile& s, const PoseTerms& t, int tile_x0, int tile_y0, int w, int h, int c,
                                           int tid) {
  // north-west q of the tile: the smallest x0(p) - (p - tile origin) over the tile's columns / rows; column / row k on lane
  // k mod 8, minimum over each group of eight lanes (every group holds all eight)
  int qx_base, qy_base;
  {
    const int k = tid & 7;
    const Bilinear t2 = pass2_taps(t, tile_x0 + k, tile_y0 + k, w, h);
    qx_base = t2.x0 - k;
    qy_base = t2.y0 - k;
#pragma unroll
    for (int d = 1; d < 8; d <<= 1) {
      qx_base = min(qx_base, __shfl_xor(qx_base, d, 64));
      qy_base = min(qy_base, __shfl_xor(qy_base, d, 64));
    }
  }
  if (tid < WARP_Q * WARP_Q) {      // pass-1 tap set of rotated pixel q = tid: sample_src's clamped offsets and masked weights
    const int q = tid;
    const Bilinear t1 = pass1_taps(t, qx_base + q % WARP_Q, qy_base + q / WARP_Q, w, h);
    const bool x0ok = t1.x0 >= 0 && t1.x0 < w, x1ok = t1.x0 + 1 >= 0 && t1.x0 + 1 < w;
    const bool y0ok = t1.y0 >= 0 && t1.y0 < h, y1ok = t1.y0 + 1 >= 0 && t1.y0 + 1 < h;
    const int x0 = min(max(t1.x0, 0), w - 1), x1 = min(max(t1.x0 + 1, 0), w - 1);
    const int y0 = min(max(t1.y0, 0), h - 1), y1 = min(max(t1.y0 + 1, 0), h - 1);
    *reinterpret_cast<u32x4w*>(s.tap1_off[q]) = u32x4w{(unsigned)((y0 * w + x0) * c) * 4u, (unsigned)((y0 * w + x1) * c) * 4u,
                                                        (unsigned)((y1 * w + x0) * c) * 4u, (unsigned)((y1 * w + x1) * c) * 4u};
    *reinterpret_cast<f32x4*>(s.tap1_w[q]) = f32x4{(y0ok && x0ok) ? t1.w_nw : 0.f, (y0ok && x1ok) ? t1.w_ne : 0.f,
                                                   (y1ok && x0ok) ? t1.w_sw : 0.f, (y1ok && x1ok) ? t1.w_se : 0.f};
  } else if (tid >= 128 && tid < 128 + WARP_T * WARP_T) {     // pass-2 tap set of output pixel pl (a wave of its own)
    const int pl = tid - 128;
    const Bilinear t2 = pass2_taps(t, tile_x0 + pl % WARP_T, tile_y0 + pl / WARP_T, w, h);
    const float qw[4] = {t2.w_nw, t2.w_ne, t2.w_sw, t2.w_se};
    int row[4];
    float wk[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int qx = t2.x0 + (k & 1), qy = t2.y0 + (k >> 1);
      const bool qok = qx >= 0 && qx < w && qy >= 0 && qy < h;
      const int lx = min(max(qx - qx_base, 0), WARP_Q - 1), ly = min(max(qy - qy_base, 0), WARP_Q - 1);
      row[k] = ly * WARP_Q + lx;
      wk[k] = qok ? qw[k] : 0.f;
    }
    *reinterpret_cast<i32x4w*>(s.tap2_row[pl]) = i32x4w{row[0], row[1], row[2], row[3]};
    *reinterpret_cast<f32x4*>(s.tap2_w[pl]) = f32x4{wk[0], wk[1], wk[2], wk[3]};
  }
}

// pass 1 (rotation) of the tile's q block, channels 64 slice + 4 l .. + 3 on this thread: nw, ne, sw, se as torch's CPU
// kernel (sample_src)
__device__ inline void warp_tile_rotate(WarpTile& s, const SrcImage& src, int slice, int tid) {
  const int l = tid & 15;
  const unsigned lane_off = 16u * (slice * (WARP_CS / 4) + l);
  for (int idx = tid; idx < WARP_Q * WARP_Q * 16; idx += 256) {
    const int q = idx >> 4;
    const u32x4w off = *reinterpret_cast<const u32x4w*>(s.tap1_off[q]);
    const f32x4 wt = *reinterpret_cast<const f32x4*>(s.tap1_w[q]);
    const f32x4 v_nw = ldb4(src, off[0] + lane_off), v_ne = ldb4(src, off[1] + lane_off);
    const f32x4 v_sw = ldb4(src, off[2] + lane_off), v_se = ldb4(src, off[3] + lane_off);
    f32x4 acc = v_nw * wt[0];
    acc += v_ne * wt[1];
    acc += v_sw * wt[2];
    acc += v_se * wt[3];
    s.rot[q][l] = acc;
  }
}

// pass 2 (translation): the four q of output pixel pl of the tile, blended in tap order, this thread's four channels
__device__ inline f32x4 warp_tile_blend(const WarpTile& s, int pl, int l) {
  const i32x4w row = *reinterpret_cast<const i32x4w*>(s.tap2_row[pl]);
  const f32x4 wt = *reinterpret_cast<const f32x4*>(s.tap2_w[pl]);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < 4; ++k) acc += s.rot[row[k]][l] * wt[k];
  return acc;
}

}  // namespace
