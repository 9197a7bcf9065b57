// Parameter-free collaboration baselines (upstream SumFusion / MeanFusion / MaxFusion, `--com sum | mean | max`;
// SURVEY.md 2.1 row 8): the pose warp of every live neighbour and the reduction over the ego's list in ONE launch.
// The warped maps are never written: a workgroup keeps its piece of the ego's map in registers as the accumulator,
// warps one neighbour after the other into LDS (the tile-shared form of warp.hip :: warp_neighbors_tiled_kernel, with
// the neighbour loop inside the workgroup) and folds each into the accumulator in list order.  One store per output.
// No workspace, no atomics, no host synchronisation: graph-capturable and bit-identical from run to run.
//
// The contract (list order, the three reductions, padded and dead agents) is in include/disconet_hip.h ::
// dn_fuse_reduce.  The warp arithmetic is warp_device.h's; against dn_warp_neighbors the warped values agree to the
// compiler's per-kernel contraction (a few ulp), not bit for bit -- as warp.hip says of its own gather kernels.
//
// Training keeps the warps (the backward of `max` needs them): dn_fuse_reduce_lists / _backward run the same
// reductions over the lists of train.fusion_lists on maps that dn_warp_list has written.
#include <hip/hip_runtime.h>

#include "disconet_train.h"
#include "dn_internal.h"

#include "ego_list.h"
#include "warp_device.h"

namespace {

// one step of the reduction over a list: `acc` holds the result over the entries so far, `v` is the next entry
//   sum, mean: fp32 add (mean divides once, at the end)
//   max: torch.max(dim=0) -- the first NaN of the list, else its first maximum (a tie keeps the earlier entry)
__device__ inline bool takes(float acc, float v) {
  return acc == acc && !(v <= acc);      // acc is no NaN, and v is larger or a NaN
}
template <int MODE>
__device__ inline void fold(f32x4& acc, const f32x4& v) {
  if (MODE == DN_FUSE_MAX) {
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] = takes(acc[e], v[e]) ? v[e] : acc[e];
  } else {
    acc += v;
  }
}
template <int MODE>
__device__ inline f32x4 finish(const f32x4& acc, int len) {
  if (MODE != DN_FUSE_MEAN) return acc;
  const float n = (float)len;
  return f32x4{acc[0] / n, acc[1] / n, acc[2] / n, acc[3] / n};      // IEEE division (x / 1 = x: a list of one)
}

// ---- c % 64 == 0: a workgroup owns one 8 x 8 tile x one 64-channel slice of one ego image.  The tile body is written out
// here, the steps of warp_device.h :: WarpTile in their order: called through them, this kernel's tap arithmetic is
// contracted differently (which product of a sum is fused, where 0.5 * x folds into a difference) and its output moves in
// the last bits against what it has always computed.  A change to WarpTile's steps is made here too.
template <int MODE>
__global__ void __launch_bounds__(256)
fuse_reduce_tiled_kernel(const float* __restrict__ feat, const float* __restrict__ trans,
                         const int32_t* __restrict__ num_agent, int batch, int agents, int h, int w, int c,
                         int only_v2i, int ego_first, int tiles_x, float* __restrict__ fused) {
  __shared__ f32x4 rot[WARP_Q * WARP_Q][WARP_CS / 4];
  __shared__ __attribute__((aligned(16))) unsigned tap1_off[WARP_Q * WARP_Q][4];
  __shared__ __attribute__((aligned(16))) float tap1_w[WARP_Q * WARP_Q][4];
  __shared__ __attribute__((aligned(16))) int tap2_row[WARP_T * WARP_T][4];
  __shared__ __attribute__((aligned(16))) float tap2_w[WARP_T * WARP_T][4];
  const int n_slices = c / WARP_CS;
  const int slice = blockIdx.x % n_slices, tile = blockIdx.x / n_slices;
  const int tile_x0 = (tile % tiles_x) * WARP_T, tile_y0 = (tile / tiles_x) * WARP_T;
  const int out_image = blockIdx.y;                       // (i - ego_first) * batch + b
  const int b = out_image % batch, i = ego_first + out_image / batch;
  const int n_live = live_count(num_agent, b, agents);
  const int tid = threadIdx.x, l = tid & 15;
  const int hw = h * w;
  const unsigned lane_off = 16u * (slice * (WARP_CS / 4) + l);

  // the ego's own values: the accumulator (pixels pl = tid / 16 + 16 k of the tile, four channels each)
  const float* ego = feat + ((size_t)i * batch + b) * hw * c + slice * WARP_CS + 4 * l;
  f32x4 acc[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int pl = (tid >> 4) + 16 * k;
    const int px = tile_x0 + pl % WARP_T, py = tile_y0 + pl / WARP_T;
    acc[k] = (px < w && py < h) ? ld4(ego + (size_t)(py * w + px) * c) : f32x4{0.f, 0.f, 0.f, 0.f};
  }
  int len = 1;
  for (int j = 0; j < n_live; ++j) {                      // (workgroup-uniform: the barriers below are met by every thread)
    if (!listed(i, j, n_live, only_v2i)) continue;
    ++len;
    const SrcImage src = make_src_image(feat + ((size_t)j * batch + b) * hw * c, (size_t)hw * c * 4);
    const PoseTerms t = pose_terms(trans + (((size_t)b * agents + i) * agents + j) * 16);
    // north-west q of the tile, as warp_neighbors_tiled_kernel
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
    __syncthreads();                                      // the previous neighbour's blend has read rot and the tables
    if (tid < WARP_Q * WARP_Q) {              // pass-1 tap set of rotated pixel q = tid: sample_src's clamped offsets and masked weights
      const int q = tid;
      const Bilinear t1 = pass1_taps(t, qx_base + q % WARP_Q, qy_base + q / WARP_Q, w, h);
      const bool x0ok = t1.x0 >= 0 && t1.x0 < w, x1ok = t1.x0 + 1 >= 0 && t1.x0 + 1 < w;
      const bool y0ok = t1.y0 >= 0 && t1.y0 < h, y1ok = t1.y0 + 1 >= 0 && t1.y0 + 1 < h;
      const int x0 = min(max(t1.x0, 0), w - 1), x1 = min(max(t1.x0 + 1, 0), w - 1);
      const int y0 = min(max(t1.y0, 0), h - 1), y1 = min(max(t1.y0 + 1, 0), h - 1);
      *reinterpret_cast<u32x4w*>(tap1_off[q]) = u32x4w{(unsigned)((y0 * w + x0) * c) * 4u, (unsigned)((y0 * w + x1) * c) * 4u,
                                                        (unsigned)((y1 * w + x0) * c) * 4u, (unsigned)((y1 * w + x1) * c) * 4u};
      *reinterpret_cast<f32x4*>(tap1_w[q]) = f32x4{(y0ok && x0ok) ? t1.w_nw : 0.f, (y0ok && x1ok) ? t1.w_ne : 0.f,
                                                   (y1ok && x0ok) ? t1.w_sw : 0.f, (y1ok && x1ok) ? t1.w_se : 0.f};
    } else if (tid >= 128 && tid < 128 + WARP_T * WARP_T) {       // pass-2 tap set of output pixel pl (a wave of its own)
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
      *reinterpret_cast<i32x4w*>(tap2_row[pl]) = i32x4w{row[0], row[1], row[2], row[3]};
      *reinterpret_cast<f32x4*>(tap2_w[pl]) = f32x4{wk[0], wk[1], wk[2], wk[3]};
    }
    __syncthreads();
    // pass 1 (rotation) of the tile's q block: nw, ne, sw, se
    for (int idx = tid; idx < WARP_Q * WARP_Q * 16; idx += 256) {
      const int q = idx >> 4;
      const u32x4w off = *reinterpret_cast<const u32x4w*>(tap1_off[q]);
      const f32x4 wt = *reinterpret_cast<const f32x4*>(tap1_w[q]);
      const f32x4 v_nw = ldb4(src, off[0] + lane_off), v_ne = ldb4(src, off[1] + lane_off);
      const f32x4 v_sw = ldb4(src, off[2] + lane_off), v_se = ldb4(src, off[3] + lane_off);
      f32x4 r = v_nw * wt[0];
      r += v_ne * wt[1];
      r += v_sw * wt[2];
      r += v_se * wt[3];
      rot[q][l] = r;
    }
    __syncthreads();
    // pass 2 (translation): blend the four q of every output pixel in tap order, then fold into the accumulator
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int pl = (tid >> 4) + 16 * k;
      const i32x4w row = *reinterpret_cast<const i32x4w*>(tap2_row[pl]);
      const f32x4 wt = *reinterpret_cast<const f32x4*>(tap2_w[pl]);
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) v += rot[row[kk]][l] * wt[kk];
      fold<MODE>(acc[k], v);
    }
  }
  float* out = fused + (size_t)out_image * hw * c + slice * WARP_CS + 4 * l;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int pl = (tid >> 4) + 16 * k;
    const int px = tile_x0 + pl % WARP_T, py = tile_y0 + pl / WARP_T;
    if (px < w && py < h) *reinterpret_cast<f32x4*>(out + (size_t)(py * w + px) * c) = finish<MODE>(acc[k], len);
  }
}

// ---- any other c (a multiple of 4): one output pixel per wave, a float4 of channels per lane, after
// warp_neighbors_kernel -- rows of 64 lanes, the last one partial ---------------------------------------------------
constexpr int PIX_PER_BLOCK = 32;

template <int MODE>
__global__ void __launch_bounds__(256)
fuse_reduce_pixel_kernel(const float* __restrict__ feat, const float* __restrict__ trans,
                         const int32_t* __restrict__ num_agent, int batch, int agents, int h, int w, int c,
                         int only_v2i, int ego_first, float* __restrict__ fused) {
  const int out_image = blockIdx.y;
  const int b = out_image % batch, i = ego_first + out_image / batch;
  const int n_live = live_count(num_agent, b, agents);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c4n = c >> 2, hw = h * w;
  const int n_it = (c4n + 63) >> 6;
  const float* ego = feat + ((size_t)i * batch + b) * hw * c;
  float* out = fused + (size_t)out_image * hw * c;
  for (int pp = wave; pp < PIX_PER_BLOCK; pp += 4) {
    const int p = blockIdx.x * PIX_PER_BLOCK + pp;
    if (p >= hw) break;
    const int py = p / w, px = p % w;
    for (int it = 0; it < n_it; ++it) {
      const int c4 = lane + 64 * it;
      const bool on = c4 < c4n;                           // the partial lane row
      const int c4s = on ? c4 : 0;                        // (an idle lane loads channel 0 and stores nothing)
      f32x4 acc = ld4(ego + (size_t)p * c + 4 * c4s);
      int len = 1;
      for (int j = 0; j < n_live; ++j) {
        if (!listed(i, j, n_live, only_v2i)) continue;
        ++len;
        const SrcImage src = make_src_image(feat + ((size_t)j * batch + b) * hw * c, (size_t)hw * c * 4);
        const PoseTerms t = pose_terms(trans + (((size_t)b * agents + i) * agents + j) * 16);
        fold<MODE>(acc, warp_pixel(src, t, px, py, w, h, c, c4s));
      }
      if (on) *reinterpret_cast<f32x4*>(out + (size_t)p * c + 4 * c4) = finish<MODE>(acc, len);
    }
  }
}

// ---- training: the same reductions over explicit lists of materialised maps --------------------------------------
template <int MODE>
__global__ void __launch_bounds__(256)
fuse_reduce_lists_kernel(const float* __restrict__ maps, const int32_t* __restrict__ first,
                         const int32_t* __restrict__ map_image, const int32_t* __restrict__ ego_out, long quads,
                         float* __restrict__ fused) {
  const int e = blockIdx.y;
  const int s = first[e], t = first[e + 1];
  if (t <= s) return;
  for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < quads; q += (long)gridDim.x * 256) {
    f32x4 acc = ld4(maps + ((size_t)map_image[s] * quads + q) * 4);
    for (int k = s + 1; k < t; ++k) fold<MODE>(acc, ld4(maps + ((size_t)map_image[k] * quads + q) * 4));
    *reinterpret_cast<f32x4*>(fused + ((size_t)ego_out[e] * quads + q) * 4) = finish<MODE>(acc, t - s);
  }
}

template <int MODE>
__global__ void __launch_bounds__(256)
fuse_reduce_lists_backward_kernel(const float* __restrict__ dfused, int ld, const float* __restrict__ maps,
                                  const int32_t* __restrict__ first, const int32_t* __restrict__ map_image,
                                  const int32_t* __restrict__ ego_out, int hw, int c4n, float* __restrict__ dmaps) {
  const int e = blockIdx.y;
  const int s = first[e], t = first[e + 1];
  if (t <= s) return;
  const long quads = (long)hw * c4n;
  for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < quads; q += (long)gridDim.x * 256) {
    const long p = q / c4n;
    const int c4 = (int)(q - p * c4n);
    const f32x4 g = ld4(dfused + ((size_t)ego_out[e] * hw + p) * ld + 4 * c4);
    if (MODE == DN_FUSE_MAX) {
      // the winner of every element, re-derived from the maps under the forward's rule
      f32x4 acc = ld4(maps + ((size_t)map_image[s] * quads + q) * 4);
      i32x4w win = {s, s, s, s};
      for (int k = s + 1; k < t; ++k) {
        const f32x4 v = ld4(maps + ((size_t)map_image[k] * quads + q) * 4);
#pragma unroll
        for (int x = 0; x < 4; ++x)
          if (takes(acc[x], v[x])) {
            acc[x] = v[x];
            win[x] = k;
          }
      }
      for (int k = s; k < t; ++k)
        *reinterpret_cast<f32x4*>(dmaps + ((size_t)map_image[k] * quads + q) * 4) =
            f32x4{win[0] == k ? g[0] : 0.f, win[1] == k ? g[1] : 0.f, win[2] == k ? g[2] : 0.f, win[3] == k ? g[3] : 0.f};
    } else {
      const f32x4 d = finish<MODE>(g, t - s);             // sum: dfused; mean: dfused / (float)len
      for (int k = s; k < t; ++k) *reinterpret_cast<f32x4*>(dmaps + ((size_t)map_image[k] * quads + q) * 4) = d;
    }
  }
}

int lists_grid_x(long quads) {
  const long blocks = (quads + 255) / 256;
  return (int)(blocks < 1 ? 1 : (blocks > 4096 ? 4096 : blocks));
}

}  // namespace

#define DN_FUSE_BY_MODE(mode, LAUNCH)                    \
  do {                                                   \
    if ((mode) == DN_FUSE_SUM) { LAUNCH(DN_FUSE_SUM); }  \
    else if ((mode) == DN_FUSE_MEAN) { LAUNCH(DN_FUSE_MEAN); } \
    else { LAUNCH(DN_FUSE_MAX); }                        \
  } while (0)

extern "C" int dn_fuse_reduce(const float* feat, const float* trans, const int32_t* num_agent, int batch, int agents,
                              int h, int w, int c, int only_v2i, int ego_first, int ego_count, int mode, float* fused,
                              void* stream) {
  DN_REQUIRE(batch > 0 && agents > 0 && h > 0 && w > 0, "fuse reduce: empty problem");
  DN_REQUIRE(feat && trans && num_agent && fused, "fuse reduce: null pointer");
  DN_REQUIRE(c > 0 && c % 4 == 0, "fuse reduce: channel count %d must be a multiple of 4", c);
  DN_REQUIRE(ego_first >= 0 && ego_count > 0 && ego_first + ego_count <= agents,
             "fuse reduce: ego range [%d, %d) outside 0..%d", ego_first, ego_first + ego_count, agents);
  DN_REQUIRE(mode == DN_FUSE_SUM || mode == DN_FUSE_MEAN || mode == DN_FUSE_MAX,
             "fuse reduce: unknown mode %d (DN_FUSE_SUM 0, DN_FUSE_MEAN 1, DN_FUSE_MAX 2)", mode);
  // 32-bit byte offsets into one image (the buffer loads), grid limits
  DN_REQUIRE((size_t)h * w * c * 4 < ((size_t)1 << 31), "fuse reduce: a %d x %d x %d map is past 2 GiB", h, w, c);
  DN_REQUIRE((long)batch * ego_count <= 65535, "fuse reduce: %ld output images, at most 65535", (long)batch * ego_count);
  hipStream_t s = (hipStream_t)stream;
  if (c % WARP_CS == 0) {
    const int tiles_x = (w + WARP_T - 1) / WARP_T, tiles_y = (h + WARP_T - 1) / WARP_T;
    dim3 grid(tiles_x * tiles_y * (c / WARP_CS), batch * ego_count);
#define DN_LAUNCH(M)                                                                                             \
    hipLaunchKernelGGL(fuse_reduce_tiled_kernel<M>, grid, dim3(256), 0, s, feat, trans, num_agent, batch, agents, \
                       h, w, c, only_v2i, ego_first, tiles_x, fused)
    DN_FUSE_BY_MODE(mode, DN_LAUNCH);
#undef DN_LAUNCH
    return dn::check_launch("fuse_reduce_tiled_kernel");
  }
  dim3 grid((h * w + PIX_PER_BLOCK - 1) / PIX_PER_BLOCK, batch * ego_count);
#define DN_LAUNCH(M)                                                                                             \
  hipLaunchKernelGGL(fuse_reduce_pixel_kernel<M>, grid, dim3(256), 0, s, feat, trans, num_agent, batch, agents,  \
                     h, w, c, only_v2i, ego_first, fused)
  DN_FUSE_BY_MODE(mode, DN_LAUNCH);
#undef DN_LAUNCH
  return dn::check_launch("fuse_reduce_pixel_kernel");
}

extern "C" int dn_fuse_reduce_lists(const float* maps, const int32_t* first, const int32_t* map_image,
                                    const int32_t* ego_out, int n_egos, int hw, int c, int mode, float* fused,
                                    void* stream) {
  DN_REQUIRE(maps && first && map_image && ego_out && fused, "fuse reduce lists: null pointer");
  DN_REQUIRE(n_egos > 0 && n_egos <= 65535 && hw > 0 && c > 0 && c % 4 == 0, "fuse reduce lists: bad shape");
  DN_REQUIRE(mode == DN_FUSE_SUM || mode == DN_FUSE_MEAN || mode == DN_FUSE_MAX, "fuse reduce lists: unknown mode %d", mode);
  const long quads = (long)hw * (c >> 2);
  dim3 grid(lists_grid_x(quads), n_egos);
#define DN_LAUNCH(M)                                                                                                   \
  hipLaunchKernelGGL(fuse_reduce_lists_kernel<M>, grid, dim3(256), 0, (hipStream_t)stream, maps, first, map_image,     \
                     ego_out, quads, fused)
  DN_FUSE_BY_MODE(mode, DN_LAUNCH);
#undef DN_LAUNCH
  return dn::check_launch("fuse_reduce_lists_kernel");
}

extern "C" int dn_fuse_reduce_lists_backward(const float* dfused, int ld, const float* maps, const float* fused,
                                             const int32_t* first, const int32_t* map_image, const int32_t* ego_out,
                                             int n_egos, int hw, int c, int mode, float* dmaps, void* stream) {
  (void)fused;      // the winner of `max` is re-derived from the maps (include/disconet_train.h)
  DN_REQUIRE(dfused && maps && first && map_image && ego_out && dmaps, "fuse reduce lists backward: null pointer");
  DN_REQUIRE(n_egos > 0 && n_egos <= 65535 && hw > 0 && c > 0 && c % 4 == 0, "fuse reduce lists backward: bad shape");
  DN_REQUIRE(ld >= c && ld % 4 == 0 && ((size_t)dfused & 15) == 0,
             "fuse reduce lists backward: dfused rows must be 16-byte aligned (ld = %d, c = %d)", ld, c);
  DN_REQUIRE(mode == DN_FUSE_SUM || mode == DN_FUSE_MEAN || mode == DN_FUSE_MAX,
             "fuse reduce lists backward: unknown mode %d", mode);
  dim3 grid(lists_grid_x((long)hw * (c >> 2)), n_egos);
#define DN_LAUNCH(M)                                                                                                   \
  hipLaunchKernelGGL(fuse_reduce_lists_backward_kernel<M>, grid, dim3(256), 0, (hipStream_t)stream, dfused, ld, maps,  \
                     first, map_image, ego_out, hw, c >> 2, dmaps)
  DN_FUSE_BY_MODE(mode, DN_LAUNCH);
#undef DN_LAUNCH
  return dn::check_launch("fuse_reduce_lists_backward_kernel");
}
