// K4: pose-based two-pass bilinear warp of neighbour feature maps into the ego
// frame (rotate -> zero-pad -> translate).  HBM/L2-bound gather.
//
// Layout: NHWC, so the C channels of one pixel are contiguous; one wavefront
// handles one output pixel at a time with each lane carrying a float4 of
// channels (C = 256 -> exactly one 1 KiB coalesced row per tap).  All tap
// coordinates of a pixel are wave-uniform, so the bounds tests are scalar
// branches, not divergent lanes.
//
// The two resampling passes are fused in one launch: the intermediate (rotated)
// map is never written to HBM.  The arithmetic of both forms -- per pixel
// (warp_pixel: the 4x re-derivation is L2-resident work) and per 8x8 tile
// (WarpTile) -- is warp_device.h's; who is warped for whom is ego_list.h's.
//
// Replaces upstream:coperception/models/det/base/* :: feature_transformation
// (SURVEY.md §8 a5).
#include <hip/hip_runtime.h>
#include <cstdlib>

#include "disconet_train.h"
#include "dn_internal.h"

#include "ego_list.h"
#include "warp_device.h"

namespace {

constexpr int PIX_PER_BLOCK = 32;

__global__ void __launch_bounds__(256)
warp_neighbors_kernel(const float* __restrict__ feat, const float* __restrict__ trans,
                      const int32_t* __restrict__ num_agent, int batch, int agents, int h, int w,
                      int c, int only_v2i, int ego_first, int ego_count,
                      float* __restrict__ warped) {
  const int jj = blockIdx.y;              // neighbour slot 0..A-2
  const int bi = blockIdx.z;              // b * ego_count + (i - ego_first)
  const int b = bi / ego_count, i = ego_first + bi % ego_count;
  const int j = jj + (jj >= i ? 1 : 0);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c4n = c >> 2;
  const int hw = h * w;
  float* dst = warped + ((size_t)bi * (agents - 1) + jj) * hw * c;

  const bool live = listed(i, j, live_count(num_agent, b, agents), only_v2i);
  const SrcImage src = make_src_image(feat + ((size_t)j * batch + b) * hw * c, (size_t)hw * c * 4);   // image j*B+b
  const PoseTerms t = pose_terms(trans + (((size_t)b * agents + i) * agents + j) * 16);

  // Channel loop with a wave-uniform trip count; whole rows of 64 lanes (c % 256 == 0) carry no per-lane
  // condition.  (Round 1 believed a lane-dependent exit here was behind the corruption seen beside the conv
  // engine on a second stream; profiles/r02_hazard_repro.txt shows this form fails the same way -- the loop
  // form is a convenience, not a fix.)
  const int n_it = (c4n + 63) >> 6;
  const bool full = (c4n & 63) == 0;
  for (int pp = wave; pp < PIX_PER_BLOCK; pp += 4) {
    const int p = blockIdx.x * PIX_PER_BLOCK + pp;
    if (p >= hw) break;
    const int py = p / w, px = p % w;
    float* out = dst + (size_t)p * c;
    if (!live) {
      for (int it = 0; it < n_it; ++it) {
        const int c4 = lane + 64 * it;
        if (full) *reinterpret_cast<f32x4*>(out + 4 * c4) = f32x4{0.f, 0.f, 0.f, 0.f};
        else if (c4 < c4n) *reinterpret_cast<f32x4*>(out + 4 * c4) = f32x4{0.f, 0.f, 0.f, 0.f};
      }
      continue;
    }
    // (the body of warp_pixel with the tap sets of the pixel kept for both loop forms below: through warp_pixel itself this
    // kernel's tap arithmetic was contracted differently and its output bits moved)
    const Bilinear t2 = pass2_taps(t, px, py, w, h);
    Bilinear t1[4];
    bool qok[4];
    float qw[4] = {t2.w_nw, t2.w_ne, t2.w_sw, t2.w_se};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int qx = t2.x0 + (k & 1), qy = t2.y0 + (k >> 1);
      qok[k] = qx >= 0 && qx < w && qy >= 0 && qy < h;
      t1[k] = pass1_taps(t, qx, qy, w, h);
    }
    auto channels = [&](int c4) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int k = 0; k < 4; ++k) acc += sample_src(src, t1[k], w, h, c, c4) * (qok[k] ? qw[k] : 0.f);
      *reinterpret_cast<f32x4*>(out + 4 * c4) = acc;
    };
    if (full) {
      for (int it = 0; it < n_it; ++it) channels(lane + 64 * it);
    } else {
      for (int it = 0; it < n_it; ++it)
        if (lane + 64 * it < c4n) channels(lane + 64 * it);
    }
  }
}

// ---- training form: an explicit list of warps, and the backward scatter ------------------
__global__ void __launch_bounds__(256)
warp_list_kernel(const float* __restrict__ src_maps, const float* __restrict__ poses,
                 const int32_t* __restrict__ src_image, int h, int w, int c,
                 float* __restrict__ warped) {
  const int wi = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c4n = c >> 2, hw = h * w;
  const SrcImage src = make_src_image(src_maps + (size_t)src_image[wi] * hw * c, (size_t)hw * c * 4);
  const PoseTerms t = pose_terms(poses + 16 * (size_t)wi);
  for (int pp = wave; pp < PIX_PER_BLOCK; pp += 4) {
    const int p = blockIdx.x * PIX_PER_BLOCK + pp;
    if (p >= hw) break;
    float* out = warped + ((size_t)wi * hw + p) * c;
    for (int c4 = lane; c4 < c4n; c4 += 64)
      *reinterpret_cast<f32x4*>(out + 4 * c4) = warp_pixel(src, t, p % w, p / w, w, h, c, c4);
  }
}

// Transposes of the two gathers, in reverse order.  PASS = 2: gradient of the translated map
// -> gradient of the rotated map (scratch, per warp).  PASS = 1: rotated-map gradient ->
// the source agent's map.  Several outputs share a tap: hardware float atomics (L2).
template <int PASS>
__global__ void __launch_bounds__(256)
warp_scatter_kernel(const float* __restrict__ grad_in, const float* __restrict__ poses,
                    const int32_t* __restrict__ src_image, int h, int w, int c,
                    float* __restrict__ grad_out) {
  const int wi = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c4n = c >> 2, hw = h * w;
  const PoseTerms t = pose_terms(poses + 16 * (size_t)wi);
  float* dst = grad_out + (size_t)(PASS == 2 ? wi : src_image[wi]) * hw * c;
  for (int pp = wave; pp < PIX_PER_BLOCK; pp += 4) {
    const int p = blockIdx.x * PIX_PER_BLOCK + pp;
    if (p >= hw) break;
    const Bilinear b = PASS == 2 ? pass2_taps(t, p % w, p / w, w, h) : pass1_taps(t, p % w, p / w, w, h);
    const float wt[4] = {b.w_nw, b.w_ne, b.w_sw, b.w_se};
    const float* gin = grad_in + ((size_t)wi * hw + p) * c;
    for (int c4 = lane; c4 < c4n; c4 += 64) {
      const f32x4 g = ld4(gin + 4 * c4);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int x = b.x0 + (k & 1), y = b.y0 + (k >> 1);
        if (x < 0 || x >= w || y < 0 || y >= h) continue;   // wave-uniform
        float* o = dst + ((size_t)y * w + x) * c + 4 * c4;
#pragma unroll
        for (int e = 0; e < 4; ++e) unsafeAtomicAdd(o + e, g[e] * wt[k]);
      }
    }
  }
}

// Gather forms of the same two transposes for RIGID poses (rotation + translation) on square
// maps: deterministic, no atomics, no zero-filled scratch.  Every output pixel looks at the few
// input pixels whose bilinear footprint can reach it and re-derives their taps with exactly the
// forward's arithmetic, so the result is the scatter's sum in a fixed order.
//   pass 2 (translation): out1_grad[q] = sum over p with q in taps2(p): the taps of p sit at
//     p + floor(shift) (+1), so p lies within [-2, +1] of q - floor(shift) per axis (float fuzz incl.);
//   pass 1 (rotation):    src_grad[r] += sum over warps w of source image m, over q with r in
//     taps1(q): for an orthonormal R the footprint of q reaches r only if q is within sqrt(2) of
//     R^-1 r, i.e. within +-2 of its rounding.
__global__ void __launch_bounds__(256)
warp_gather2_kernel(const float* __restrict__ d_warped, const float* __restrict__ poses, int h, int w,
                    int c, float* __restrict__ d_out1) {
  const int wi = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c4n = c >> 2, hw = h * w;
  const PoseTerms t = pose_terms(poses + 16 * (size_t)wi);
  const int fsx = (int)floorf(t.x_trans * w * 0.5f), fsy = (int)floorf(t.y_trans * h * 0.5f);
  const float* gin = d_warped + (size_t)wi * hw * c;
  for (int pp = wave; pp < PIX_PER_BLOCK; pp += 4) {
    const int q = blockIdx.x * PIX_PER_BLOCK + pp;
    if (q >= hw) break;
    const int qx = q % w, qy = q / w;
    f32x4 acc[4];                                  // c <= 1024
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int dy = -2; dy <= 1; ++dy) {
      const int py = qy - fsy + dy;
      if (py < 0 || py >= h) continue;
      for (int dx = -2; dx <= 1; ++dx) {
        const int px = qx - fsx + dx;
        if (px < 0 || px >= w) continue;
        const Bilinear b = pass2_taps(t, px, py, w, h);
        const int ox = qx - b.x0, oy = qy - b.y0;
        if (ox < 0 || ox > 1 || oy < 0 || oy > 1) continue;   // wave-uniform
        const float wt = oy ? (ox ? b.w_se : b.w_sw) : (ox ? b.w_ne : b.w_nw);
        const float* g = gin + (size_t)(py * w + px) * c;
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (lane + 64 * i < c4n) acc[i] += ld4(g + 4 * (lane + 64 * i)) * wt;
      }
    }
    float* out = d_out1 + ((size_t)wi * hw + q) * c;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (lane + 64 * i < c4n) *reinterpret_cast<f32x4*>(out + 4 * (lane + 64 * i)) = acc[i];
  }
}

__global__ void __launch_bounds__(256)
warp_gather1_kernel(const float* __restrict__ d_out1, const float* __restrict__ poses,
                    const int32_t* __restrict__ src_image, int n_warps, int h, int w, int c,
                    float* __restrict__ d_src) {
  const int m = blockIdx.y;                       // source image
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c4n = c >> 2, hw = h * w;
  for (int pp = wave; pp < PIX_PER_BLOCK; pp += 4) {
    const int r = blockIdx.x * PIX_PER_BLOCK + pp;
    if (r >= hw) break;
    const int rx = r % w, ry = r / w;
    const float rbx = (2.f * rx + 1.f) / w - 1.f, rby = (2.f * ry + 1.f) / h - 1.f;
    float* out = d_src + ((size_t)m * hw + r) * c;
    f32x4 acc[4];                                  // c <= 1024
#pragma unroll
    for (int i = 0; i < 4; ++i)
      acc[i] = (lane + 64 * i < c4n) ? ld4(out + 4 * (lane + 64 * i)) : f32x4{0.f, 0.f, 0.f, 0.f};
    for (int wi = 0; wi < n_warps; ++wi) {
      if (src_image[wi] != m) continue;            // wave-uniform
      const PoseTerms t = pose_terms(poses + 16 * (size_t)wi);
      const float det = t.r00 * t.r11 - t.r01 * t.r10;
      const float qbx = (t.r11 * rbx - t.r01 * rby) / det, qby = (-t.r10 * rbx + t.r00 * rby) / det;
      const int cx = (int)rintf(((qbx + 1.f) * w - 1.f) * 0.5f), cy = (int)rintf(((qby + 1.f) * h - 1.f) * 0.5f);
      const float* gin = d_out1 + (size_t)wi * hw * c;
      for (int dy = -2; dy <= 2; ++dy) {
        const int qy = cy + dy;
        if (qy < 0 || qy >= h) continue;
        for (int dx = -2; dx <= 2; ++dx) {
          const int qx = cx + dx;
          if (qx < 0 || qx >= w) continue;
          const Bilinear b = pass1_taps(t, qx, qy, w, h);
          const int ox = rx - b.x0, oy = ry - b.y0;
          if (ox < 0 || ox > 1 || oy < 0 || oy > 1) continue;
          const float wt = oy ? (ox ? b.w_se : b.w_sw) : (ox ? b.w_ne : b.w_nw);
          const float* g = gin + (size_t)(qy * w + qx) * c;
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (lane + 64 * i < c4n) acc[i] += ld4(g + 4 * (lane + 64 * i)) * wt;
        }
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (lane + 64 * i < c4n) *reinterpret_cast<f32x4*>(out + 4 * (lane + 64 * i)) = acc[i];
  }
}

// ---- lane-parallel candidate search of the two gathers (round 6).  The kernels above evaluate their 16 / 25 candidate pixels one
// after the other with wave-uniform arithmetic -- 64 lanes computing the same tap set, ~100 evaluations per output pixel in pass 1:
// VALU-bound at 228 + 92 us per step for 32 x 32 x 256 maps.  Here lane k evaluates candidate k (the same expressions: pass1_taps /
// pass2_taps of the same integers), a ballot gives the hits, and the hits are added in ascending candidate order -- the order of the
// loops above -- four rows in flight at a time.  Deterministic like them; against them the sums agree to a few ulp, not bit for bit
// (the compiler contracts the tap arithmetic per kernel: weights differ in their last bit).  PIXW: output pixels per wave.
constexpr int GATHER_PIXW = 1;
struct GatherHits {
  unsigned long long mask;
  float wt;
  int off;
};
// adds the hit rows (row offset `off`, weight `wt` of the lanes in `mask`, ascending) of `gin` into acc
__device__ inline void gather_add_hits(GatherHits hs, const float* __restrict__ gin, int c, int c4n, int lane, f32x4 (&acc)[4]) {
  while (hs.mask) {
    int n = 0;
    float wk[4];
    int ok[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (hs.mask) {
        const int kk = __builtin_ctzll(hs.mask);
        hs.mask &= hs.mask - 1;
        wk[j] = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, hs.wt), kk));
        ok[j] = __builtin_amdgcn_readlane(hs.off, kk);
        n = j + 1;
      } else {
        wk[j] = 0.f;
        ok[j] = 0;
      }
    }
    f32x4 v[4][4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < n) {                                   // wave-uniform
        const float* g = gin + (size_t)ok[j] * c;
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (lane + 64 * i < c4n) v[j][i] = ld4(g + 4 * (lane + 64 * i));
      }
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < n) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (lane + 64 * i < c4n) acc[i] += v[j][i] * wk[j];
      }
  }
}

__global__ void __launch_bounds__(256)
warp_gather2_lanes_kernel(const float* __restrict__ d_warped, const float* __restrict__ poses, int h, int w,
                          int c, float* __restrict__ d_out1) {
  const int wi = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c4n = c >> 2, hw = h * w;
  const PoseTerms t = pose_terms(poses + 16 * (size_t)wi);
  const int fsx = (int)floorf(t.x_trans * w * 0.5f), fsy = (int)floorf(t.y_trans * h * 0.5f);
  const float* gin = d_warped + (size_t)wi * hw * c;
  const int k = lane & 15, dy = (k >> 2) - 2, dx = (k & 3) - 2;      // candidate k of the scalar kernel's (dy, dx) loops
  for (int pp = 0; pp < GATHER_PIXW; ++pp) {
    const int q = (blockIdx.x * 4 + wave) * GATHER_PIXW + pp;
    if (q >= hw) break;
    const int qx = q % w, qy = q / w;
    f32x4 acc[4];                                  // c <= 1024
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int py = qy - fsy + dy, px = qx - fsx + dx;
    bool hit = lane < 16 && py >= 0 && py < h && px >= 0 && px < w;
    const Bilinear b = pass2_taps(t, px, py, w, h);
    const int ox = qx - b.x0, oy = qy - b.y0;
    hit = hit && ox >= 0 && ox <= 1 && oy >= 0 && oy <= 1;
    GatherHits hs;
    hs.wt = oy ? (ox ? b.w_se : b.w_sw) : (ox ? b.w_ne : b.w_nw);
    hs.off = py * w + px;
    hs.mask = __ballot(hit);
    gather_add_hits(hs, gin, c, c4n, lane, acc);
    float* out = d_out1 + ((size_t)wi * hw + q) * c;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (lane + 64 * i < c4n) *reinterpret_cast<f32x4*>(out + 4 * (lane + 64 * i)) = acc[i];
  }
}

__global__ void __launch_bounds__(256)
warp_gather1_lanes_kernel(const float* __restrict__ d_out1, const float* __restrict__ poses,
                          const int32_t* __restrict__ src_image, int n_warps, int h, int w, int c,
                          float* __restrict__ d_src) {
  const int m = blockIdx.y;                       // source image
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c4n = c >> 2, hw = h * w;
  const int k = lane < 25 ? lane : 24, dy = k / 5 - 2, dx = k % 5 - 2;   // candidate k of the scalar kernel's (dy, dx) loops
  for (int pp = 0; pp < GATHER_PIXW; ++pp) {
    const int r = (blockIdx.x * 4 + wave) * GATHER_PIXW + pp;
    if (r >= hw) break;
    const int rx = r % w, ry = r / w;
    const float rbx = (2.f * rx + 1.f) / w - 1.f, rby = (2.f * ry + 1.f) / h - 1.f;
    float* out = d_src + ((size_t)m * hw + r) * c;
    f32x4 acc[4];                                  // c <= 1024
#pragma unroll
    for (int i = 0; i < 4; ++i)
      acc[i] = (lane + 64 * i < c4n) ? ld4(out + 4 * (lane + 64 * i)) : f32x4{0.f, 0.f, 0.f, 0.f};
    for (int w0 = 0; w0 < n_warps; w0 += 64) {
      unsigned long long wmask = __ballot(w0 + lane < n_warps && src_image[w0 + lane < n_warps ? w0 + lane : 0] == m);
      while (wmask) {                              // the warps of this source image, ascending
        const int wi = w0 + __builtin_ctzll(wmask);
        wmask &= wmask - 1;
        const PoseTerms t = pose_terms(poses + 16 * (size_t)wi);
        const float det = t.r00 * t.r11 - t.r01 * t.r10;
        const float qbx = (t.r11 * rbx - t.r01 * rby) / det, qby = (-t.r10 * rbx + t.r00 * rby) / det;
        const int cx = (int)rintf(((qbx + 1.f) * w - 1.f) * 0.5f), cy = (int)rintf(((qby + 1.f) * h - 1.f) * 0.5f);
        const int qy = cy + dy, qx = cx + dx;
        bool hit = lane < 25 && qy >= 0 && qy < h && qx >= 0 && qx < w;
        const Bilinear b = pass1_taps(t, qx, qy, w, h);
        const int ox = rx - b.x0, oy = ry - b.y0;
        hit = hit && ox >= 0 && ox <= 1 && oy >= 0 && oy <= 1;
        GatherHits hs;
        hs.wt = oy ? (ox ? b.w_se : b.w_sw) : (ox ? b.w_ne : b.w_nw);
        hs.off = qy * w + qx;
        hs.mask = __ballot(hit);
        gather_add_hits(hs, d_out1 + (size_t)wi * hw * c, c, c4n, lane, acc);
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (lane + 64 * i < c4n) *reinterpret_cast<f32x4*>(out + 4 * (lane + 64 * i)) = acc[i];
  }
}

// ---- tile-shared form of the same two passes (warp_device.h :: WarpTile): one workgroup = one 8 x 8 tile x one
// 64-channel slice of one (ego, neighbour) pair ------------------
__global__ void __launch_bounds__(256)
warp_neighbors_tiled_kernel(const float* __restrict__ feat, const float* __restrict__ trans,
                            const int32_t* __restrict__ num_agent, int batch, int agents, int h, int w,
                            int c, int only_v2i, int ego_first, int ego_count, int tiles_x, int fm,
                            float* __restrict__ warped) {
  __shared__ WarpTile tile_s;
  const int n_slices = c / WARP_CS;
  const int slice = blockIdx.x % n_slices, tile = blockIdx.x / n_slices;
  const int tile_x0 = (tile % tiles_x) * WARP_T, tile_y0 = (tile / tiles_x) * WARP_T;
  const int jj = blockIdx.y, bi = blockIdx.z;
  const int b = bi / ego_count, i = ego_first + bi % ego_count;
  const int j = jj + (jj >= i ? 1 : 0);
  const int tid = threadIdx.x, l = tid & 15;
  const int hw = h * w;
  float* dst = warped + ((size_t)bi * (agents - 1) + jj) * hw * c + (fm ? 0 : slice * WARP_CS + 4 * l);
  // fm: FRAGMENT-MAJOR pair block (include/disconet_hip.h :: dn_warp_neighbors_fm) -- the order in which the attention
  // launch reads it: [tile of 32 pixels][k-step of 16 channels][half r][lane = 32 h + j] x 4 floats, channel
  // 16 ks + 8 h + 4 r + e of pixel 32 t + j.  This thread's four channels 64 slice + 4 l .. + 3 are one such piece.
  const int fm_ks = slice * 4 + (l >> 2), fm_h = (l >> 1) & 1, fm_r = l & 1, fm_kss = c >> 4;
  auto out_of = [&](int p) {
    return fm ? dst + (((((size_t)(p >> 5) * fm_kss + fm_ks) * 2 + fm_r) * 64) + fm_h * 32 + (p & 31)) * 4
              : dst + (size_t)p * c;
  };
  const bool live = listed(i, j, live_count(num_agent, b, agents), only_v2i);
  if (!live) {
    for (int pl = tid >> 4; pl < WARP_T * WARP_T; pl += 16) {
      const int px = tile_x0 + pl % WARP_T, py = tile_y0 + pl / WARP_T;
      if (px < w && py < h) *reinterpret_cast<f32x4*>(out_of(py * w + px)) = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    return;
  }
  const SrcImage src = make_src_image(feat + ((size_t)j * batch + b) * hw * c, (size_t)hw * c * 4);
  const PoseTerms t = pose_terms(trans + (((size_t)b * agents + i) * agents + j) * 16);
  warp_tile_fill_taps(tile_s, t, tile_x0, tile_y0, w, h, c, tid);
  __syncthreads();
  warp_tile_rotate(tile_s, src, slice, tid);
  __syncthreads();
  for (int pl = tid >> 4; pl < WARP_T * WARP_T; pl += 16) {
    const int px = tile_x0 + pl % WARP_T, py = tile_y0 + pl / WARP_T;
    if (px < w && py < h) *reinterpret_cast<f32x4*>(out_of(py * w + px)) = warp_tile_blend(tile_s, pl, l);
  }
}

}  // namespace



extern "C" int dn_warp_list(const float* src, const float* poses, const int32_t* src_image,
                            int n_warps, int h, int w, int c, float* warped, void* stream) {
  DN_REQUIRE(src && poses && src_image && warped, "warp list: null pointer");
  DN_REQUIRE(n_warps > 0 && h > 0 && w > 0 && c > 0 && c % 4 == 0, "warp list: bad shape");
  dim3 grid((h * w + PIX_PER_BLOCK - 1) / PIX_PER_BLOCK, n_warps);
  hipLaunchKernelGGL(warp_list_kernel, grid, dim3(256), 0, (hipStream_t)stream, src, poses, src_image, h,
                     w, c, warped);
  return dn::check_launch("warp_list_kernel");
}

extern "C" int dn_warp_backward(const float* d_warped, const float* poses, const int32_t* src_image,
                                int n_warps, int n_src_images, int h, int w, int c, int rigid,
                                float* scratch, float* d_src, void* stream) {
  DN_REQUIRE(d_warped && poses && src_image && scratch && d_src, "warp backward: null pointer");
  DN_REQUIRE(n_warps > 0 && n_src_images > 0 && h > 0 && w > 0 && c > 0 && c % 4 == 0 && c <= 1024,
             "warp backward: bad shape");
  hipStream_t s = (hipStream_t)stream;
  dim3 grid((h * w + PIX_PER_BLOCK - 1) / PIX_PER_BLOCK, n_warps);
  if (rigid && h == w) {
    static const bool legacy = [] { const char* e = getenv("DN_WARP_GATHER_LEGACY"); return e && e[0] == '1'; }();
    if (legacy) {     // round 5's one-candidate-at-a-time kernels (tests, A/B runs)
      hipLaunchKernelGGL(warp_gather2_kernel, grid, dim3(256), 0, s, d_warped, poses, h, w, c, scratch);
      hipLaunchKernelGGL(warp_gather1_kernel, dim3(grid.x, n_src_images), dim3(256), 0, s, scratch, poses,
                         src_image, n_warps, h, w, c, d_src);
    } else {
      const int gx = (h * w + 4 * GATHER_PIXW - 1) / (4 * GATHER_PIXW);
      hipLaunchKernelGGL(warp_gather2_lanes_kernel, dim3(gx, n_warps), dim3(256), 0, s, d_warped, poses, h, w, c, scratch);
      hipLaunchKernelGGL(warp_gather1_lanes_kernel, dim3(gx, n_src_images), dim3(256), 0, s, scratch, poses,
                         src_image, n_warps, h, w, c, d_src);
    }
    return dn::check_launch("warp_gather kernels");
  }
  if (dn::zero_fill(scratch, sizeof(float) * (size_t)n_warps * h * w * c, s) != hipSuccess)
    return dn::fail(DN_ERR_LAUNCH, "warp backward: memset failed");
  hipLaunchKernelGGL(warp_scatter_kernel<2>, grid, dim3(256), 0, s, d_warped, poses, src_image, h, w, c,
                     scratch);
  hipLaunchKernelGGL(warp_scatter_kernel<1>, grid, dim3(256), 0, s, scratch, poses, src_image, h, w, c,
                     d_src);
  return dn::check_launch("warp_scatter_kernel");
}

namespace {
int warp_neighbors_impl(const float* feat, const float* trans, const int32_t* num_agent, int batch, int agents, int h, int w,
                        int c, int only_v2i, int ego_first, int ego_count, float* warped, int fm, void* stream);
}

extern "C" int dn_warp_neighbors(const float* feat, const float* trans, const int32_t* num_agent,
                                 int batch, int agents, int h, int w, int c, int only_v2i,
                                 int ego_first, int ego_count, float* warped, void* stream) {
  return warp_neighbors_impl(feat, trans, num_agent, batch, agents, h, w, c, only_v2i, ego_first, ego_count, warped, 0, stream);
}

extern "C" int dn_warp_fm_supported(int h, int w, int c) { return c % WARP_CS == 0 && (h * w) % 32 == 0; }

extern "C" int dn_warp_neighbors_fm(const float* feat, const float* trans, const int32_t* num_agent,
                                    int batch, int agents, int h, int w, int c, int only_v2i,
                                    int ego_first, int ego_count, float* warped, void* stream) {
  DN_REQUIRE(dn_warp_fm_supported(h, w, c), "warp (fragment-major): needs c %% 64 == 0 and h * w %% 32 == 0 (got %d x %d x %d)", h, w, c);
  return warp_neighbors_impl(feat, trans, num_agent, batch, agents, h, w, c, only_v2i, ego_first, ego_count, warped, 1, stream);
}

namespace {
int warp_neighbors_impl(const float* feat, const float* trans, const int32_t* num_agent, int batch, int agents, int h, int w,
                        int c, int only_v2i, int ego_first, int ego_count, float* warped, int fm, void* stream) {
  DN_REQUIRE(batch > 0 && agents > 0 && h > 0 && w > 0, "warp: empty problem");
  DN_REQUIRE(feat && trans && num_agent && (warped || agents < 2), "warp: null pointer");
  DN_REQUIRE(c > 0 && c % 4 == 0, "warp: channel count %d must be a multiple of 4", c);
  DN_REQUIRE(ego_first >= 0 && ego_count > 0 && ego_first + ego_count <= agents,
             "warp: ego range [%d, %d) outside 0..%d", ego_first, ego_first + ego_count, agents);
  if (agents < 2) return DN_OK;   // no neighbours to warp
  const int hw = h * w;
  if (c % WARP_CS == 0) {
    const int tiles_x = (w + WARP_T - 1) / WARP_T, tiles_y = (h + WARP_T - 1) / WARP_T;
    dim3 tgrid(tiles_x * tiles_y * (c / WARP_CS), agents - 1, batch * ego_count);
    hipLaunchKernelGGL(warp_neighbors_tiled_kernel, tgrid, dim3(256), 0, (hipStream_t)stream, feat, trans,
                       num_agent, batch, agents, h, w, c, only_v2i, ego_first, ego_count, tiles_x, fm, warped);
    return dn::check_launch("warp_neighbors_tiled_kernel");
  }
  dim3 grid((hw + PIX_PER_BLOCK - 1) / PIX_PER_BLOCK, agents - 1, batch * ego_count);
  hipLaunchKernelGGL(warp_neighbors_kernel, grid, dim3(256), 0, (hipStream_t)stream, feat, trans,
                     num_agent, batch, agents, h, w, c, only_v2i, ego_first, ego_count, warped);
  return dn::check_launch("warp_neighbors_kernel");
}
}  // namespace
