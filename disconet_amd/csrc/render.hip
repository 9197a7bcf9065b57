// BEV rendering: every image of a batch rasterised into an RGB canvas (dn_render_bev).  The contract is in
// include/disconet_hip.h; the host statement that defines the bytes is render.host_render_bev.  All geometry is fp64 in a
// fixed order, + - * / and sqrt only, and every function that computes it carries `#pragma clang fp contract(off)`; the
// colours are integer arithmetic.
//
// One launch (render_bev_kernel), one workgroup of 256 lanes per 32 x 32 canvas tile, four consecutive pixels of a canvas
// row per lane; the 12 bytes of those four pixels leave as three dword stores (w % 4 == 0, so a group of four is wholly
// inside the canvas or wholly outside and every group starts on a dword).
//   background  the occupancy word / label of each pixel -> its colour, then the heat overlay, in registers
//   bin         per set and per pass of 256 rows: a lane takes a row, computes its constants in fp64, tests the row's
//               bounding circle grown by the thickness against the tile; the survivors are compacted IN ROW ORDER into an
//               LDS list (64-bit ballot, popcount prefix per wave, wave counts through LDS).  A pass holds at most 256
//               entries, so a tile that more rows cover than one pass holds still paints all of them, in order.
//   paint       every lane walks the list for its four pixels: the per-pixel rule of the contract
// The circle test is conservative (a slack of one pixel and a relative 1e-6 over the rounding of the per-pixel terms): it
// never changes a byte.  Every barrier is reached by every lane: the pass count depends on the image's count, which is the
// same for the whole workgroup (one image per workgroup); the ids and the tile's position only decide a lane's own keep
// flag and stores.
#include <cmath>

#include "dn_internal.h"

namespace {

constexpr int kTile = 32;        // canvas pixels per tile side
constexpr int kThreads = 256;    // 32 rows x 8 groups of four pixels
constexpr int kWaves = kThreads / 64;
__constant__ unsigned char d_id_palette[96] = DN_RENDER_ID_PALETTE;

struct Rgb {
  int r, g, b;
};

__device__ __forceinline__ Rgb rgb_of(const uint8_t* c) { return Rgb{(int)c[0], (int)c[1], (int)c[2]}; }

__device__ __forceinline__ unsigned pack_rgb(Rgb c) { return (unsigned)c.r | ((unsigned)c.g << 8) | ((unsigned)c.b << 16); }

__device__ __forceinline__ Rgb unpack_rgb(unsigned p) { return Rgb{(int)(p & 255u), (int)((p >> 8) & 255u), (int)((p >> 16) & 255u)}; }

// BLEND of the contract: (below (255 - a) + over a + 127) / 255 per channel
__device__ __forceinline__ Rgb blend(Rgb below, Rgb over, int a) {
  return Rgb{(below.r * (255 - a) + over.r * a + 127) / 255, (below.g * (255 - a) + over.g * a + 127) / 255,
             (below.b * (255 - a) + over.b * a + 127) / 255};
}

// the row's constants: centre, unit heading, half sizes in canvas units; false when the contract skips the row
__device__ __forceinline__ bool row_constants(const float* row, double x_lo, double y_lo, double voxel, double scale, double& X,
                                              double& Y, double& cs, double& sn, double& A, double& B) {
#pragma clang fp contract(off)
  const double x = (double)row[0], y = (double)row[1], w = (double)row[2], h = (double)row[3];
  const double s = (double)row[4], c = (double)row[5];
  if (!(std::isfinite(x) && std::isfinite(y) && std::isfinite(w) && std::isfinite(h) && std::isfinite(s) && std::isfinite(c)))
    return false;
  const double nrm = sqrt(s * s + c * c);
  if (!(nrm > 0.0) || !(w > 0.0) || !(h > 0.0)) return false;
  cs = c / nrm;
  sn = s / nrm;
  X = ((x - x_lo) / voxel) * scale;
  Y = ((y - y_lo) / voxel) * scale;
  A = ((w / 2.0) / voxel) * scale;
  B = ((h / 2.0) / voxel) * scale;
  return true;
}

// may a pixel of the tile [r0, r0 + 32) x [q0, q0 + 32) be touched by the row?  Conservative: a touched pixel's centre lies
// within sqrt(A A + B B) + thickness of (X, Y) up to the rounding of u and v, which the slack covers.
__device__ __forceinline__ bool circle_meets_tile(double X, double Y, double A, double B, double t, int r0, int q0) {
  const double R = (sqrt(A * A + B * B) + t + 1.0) * 1.000001;
  const double lo_r = (double)r0, hi_r = (double)(r0 + kTile), lo_q = (double)q0, hi_q = (double)(q0 + kTile);
  const double ddx = X < lo_r ? lo_r - X : (X > hi_r ? X - hi_r : 0.0);
  const double ddy = Y < lo_q ? lo_q - Y : (Y > hi_q ? Y - hi_q : 0.0);
  return ddx * ddx + ddy * ddy <= R * R;
}

__device__ __forceinline__ Rgb row_colour(const dn_render_set& s, size_t at) {
#pragma clang fp contract(off)
  if (s.colour_by == DN_RENDER_COLOUR_SCORE) {
    const double z = (double)s.scores[at];
    const double zc = z > 0.0 ? (z < 1.0 ? z : 1.0) : 0.0;      // a NaN gives 0
    const int l = (int)floor(zc * 255.0);
    const Rgb lo = rgb_of(s.colour), hi = rgb_of(s.colour_hi);
    return Rgb{(lo.r * (255 - l) + hi.r * l + 127) / 255, (lo.g * (255 - l) + hi.g * l + 127) / 255,
               (lo.b * (255 - l) + hi.b * l + 127) / 255};
  }
  if (s.colour_by == DN_RENDER_COLOUR_ID) {
    const int e = (int)((unsigned)s.ids[at] & 31u);            // the id is >= 0 here
    return Rgb{(int)d_id_palette[3 * e], (int)d_id_palette[3 * e + 1], (int)d_id_palette[3 * e + 2]};
  }
  return rgb_of(s.colour);
}

__global__ void __launch_bounds__(kThreads) render_bev_kernel(dn_render_desc d, uint8_t* __restrict__ out) {
#pragma clang fp contract(off)
  __shared__ double l_x[kThreads], l_y[kThreads], l_c[kThreads], l_s[kThreads], l_a[kThreads], l_b[kThreads];
  __shared__ unsigned l_col[kThreads];
  __shared__ int wave_count[kWaves];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int S = d.scale, ch = d.h * S, cw = d.w * S;
  const int img = blockIdx.z, r0 = blockIdx.y * kTile, q0 = blockIdx.x * kTile;
  const int r = r0 + (tid >> 3), q = q0 + 4 * (tid & 7);
  const bool inside = r < ch && q < cw;                         // the four pixels together: cw % 4 == 0
  const double voxel = d.voxel[0], scale = (double)S;

  // ---- background and heat overlay ----
  Rgb px[4];
  const Rgb ground = rgb_of(d.ground);
#pragma unroll
  for (int j = 0; j < 4; ++j) px[j] = ground;
  // S is 1, 2 or 4: the cell of a pixel is a shift.  The four pixels of a lane mostly share one heat cell, so its fp64
  // division is made once per distinct cell, and the cell's index costs a division only where the four differ.
  const int ls = S == 4 ? 2 : (S == 2 ? 1 : 0);
  if (inside) {
    const int bx = r >> ls;
    const size_t base = ((size_t)img * d.h + bx) * d.w;
    if (d.bg_kind == DN_RENDER_BG_OCCUPANCY) {
      const unsigned* words = static_cast<const unsigned*>(d.background);
      const Rgb point = rgb_of(d.point);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int pc = __popc(words[base + ((q + j) >> ls)]);
        const int m = pc < 8 ? pc : 8;
        px[j] = Rgb{(ground.r * (8 - m) + point.r * m + 4) / 8, (ground.g * (8 - m) + point.g * m + 4) / 8,
                    (ground.b * (8 - m) + point.b * m + 4) / 8};
      }
    } else if (d.bg_kind == DN_RENDER_BG_CLASSES) {
      const int* labels = static_cast<const int*>(d.background);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int label = labels[base + ((q + j) >> ls)];
        if (label >= 0 && label < d.n_classes) px[j] = rgb_of(d.palette + 3 * (size_t)label);
      }
    }
    if (d.heat) {
      const int fy = d.h / d.heat_h, fx = d.w / d.heat_w;
      const float* hrow = d.heat + ((size_t)img * d.heat_h + bx / fy) * d.heat_w;
      const Rgb hc = rgb_of(d.heat_colour);
      const double span = d.heat_hi - d.heat_lo;
      const int first_cell = (q >> ls) / fx, last_cell = ((q + 3) >> ls) / fx;
      int cell = -1, alpha = -1;                                // alpha < 0: a NaN, the pixel is left alone
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = first_cell == last_cell ? first_cell : ((q + j) >> ls) / fx;
        if (c != cell) {
          cell = c;
          const double t = ((double)hrow[c] - d.heat_lo) / span;
          const double tc = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
          alpha = t != t ? -1 : (d.heat_alpha * (int)floor(tc * 255.0) + 127) / 255;
        }
        if (alpha >= 0) px[j] = blend(px[j], hc, alpha);
      }
    }
  }

  // ---- the box sets ----
  const double pr = (double)r + 0.5;
  for (int si = 0; si < d.n_sets; ++si) {
    const dn_render_set& set = d.sets[si];
    const int k = set.k;
    int cnt = k;
    if (set.count) {
      cnt = set.count[img];
      cnt = cnt < 0 ? 0 : (cnt > k ? k : cnt);
    }
    cnt = __builtin_amdgcn_readfirstlane(cnt);                  // one image per workgroup: the same in every lane
    const double thick = (double)set.thickness, half_thick = thick / 2.0;
    const bool by_id = set.colour_by == DN_RENDER_COLOUR_ID;
    for (int first = 0; first < cnt; first += kThreads) {       // the pass count is the workgroup's: the image's count
      const int row = first + tid;
      bool keep = false;
      double X = 0, Y = 0, cs = 0, sn = 0, A = 0, B = 0;
      unsigned col = 0;
      if (row < cnt) {
        const size_t at = (size_t)img * k + row;
        keep = row_constants(set.boxes + 6 * at, d.x_lo, d.y_lo, voxel, scale, X, Y, cs, sn, A, B);
        if (keep && by_id && set.ids[at] < 0) keep = false;
        if (keep) keep = circle_meets_tile(X, Y, A, B, thick, r0, q0);
        if (keep) col = pack_rgb(row_colour(set, at));
      }
      const unsigned long long ballot = __ballot(keep);
      const int before = __popcll(ballot & ((1ull << lane) - 1ull));
      if (lane == 0) wave_count[wave] = __popcll(ballot);
      __syncthreads();
      int offset = 0, total = 0;
#pragma unroll
      for (int w = 0; w < kWaves; ++w) {
        const int c = wave_count[w];
        if (w < wave) offset += c;
        total += c;
      }
      if (keep) {
        const int e = offset + before;
        l_x[e] = X; l_y[e] = Y; l_c[e] = cs; l_s[e] = sn; l_a[e] = A; l_b[e] = B;
        l_col[e] = col;
      }
      __syncthreads();
      if (inside) {
        for (int e = 0; e < total; ++e) {
          const double eX = l_x[e], eY = l_y[e], ec = l_c[e], es = l_s[e], eA = l_a[e], eB = l_b[e];
          const Rgb colour = unpack_rgb(l_col[e]);
          const double dx = pr - eX;
          const double dxc = dx * ec, dxs = dx * es;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const double dy = ((double)(q + j) + 0.5) - eY;
            const double u = dxc + dy * es;
            const double v = dy * ec - dxs;
            const double au = fabs(u) - eA, av = fabs(v) - eB;
            const double edge = au > av ? au : av;
            const bool outline = -thick < edge && edge <= 0.0;
            const bool tick = set.heading != 0 && 0.0 <= u && u <= eA && fabs(v) <= half_thick;
            if (outline || tick) px[j] = colour;
            else if (edge <= 0.0 && set.fill_alpha > 0) px[j] = blend(px[j], colour, set.fill_alpha);
          }
        }
      }
      __syncthreads();                                          // the list and the wave counts are rewritten next pass
    }
  }

  if (inside) {
    unsigned char b[12];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      b[3 * j] = (unsigned char)px[j].r; b[3 * j + 1] = (unsigned char)px[j].g; b[3 * j + 2] = (unsigned char)px[j].b;
    }
    unsigned* dst = reinterpret_cast<unsigned*>(out + (((size_t)img * ch + r) * cw + q) * 3);
#pragma unroll
    for (int wd = 0; wd < 3; ++wd)
      dst[wd] = (unsigned)b[4 * wd] | ((unsigned)b[4 * wd + 1] << 8) | ((unsigned)b[4 * wd + 2] << 16) |
                ((unsigned)b[4 * wd + 3] << 24);
  }
}

}  // namespace

extern "C" int dn_render_bev(const dn_render_desc* desc, uint8_t* out, void* stream) {
  DN_REQUIRE(desc, "render_bev: null descriptor");
  DN_REQUIRE(out, "render_bev: null canvas");
  const dn_render_desc& d = *desc;
  DN_REQUIRE((reinterpret_cast<size_t>(out) & 3) == 0, "render_bev: the canvas must be 4-byte aligned");
  DN_REQUIRE(d.n >= 1 && d.n <= 65535, "render_bev: %d images is out of range [1, 65535]", d.n);
  DN_REQUIRE(d.scale == 1 || d.scale == 2 || d.scale == 4, "render_bev: scale = %d, must be 1, 2 or 4", d.scale);
  DN_REQUIRE(d.h >= 1 && d.w >= 1 && d.w % 4 == 0, "render_bev: map %d x %d, the width must be a multiple of 4", d.h, d.w);
  DN_REQUIRE((double)d.h * d.scale * d.w * d.scale * 3.0 < 2147483648.0, "render_bev: a %d x %d map at scale %d is too large",
             d.h, d.w, d.scale);
  DN_REQUIRE(d.voxel[0] == d.voxel[1], "render_bev: voxel_size %g x %g, the pixels must be square", d.voxel[0], d.voxel[1]);
  DN_REQUIRE(std::isfinite(d.voxel[0]) && d.voxel[0] > 0, "render_bev: voxel_size = %g, must be finite and > 0", d.voxel[0]);
  DN_REQUIRE(std::isfinite(d.x_lo) && std::isfinite(d.y_lo), "render_bev: the extents' lower edge must be finite");
  DN_REQUIRE(d.bg_kind == DN_RENDER_BG_NONE || d.bg_kind == DN_RENDER_BG_OCCUPANCY || d.bg_kind == DN_RENDER_BG_CLASSES,
             "render_bev: unknown background kind %d", d.bg_kind);
  DN_REQUIRE(d.bg_kind == DN_RENDER_BG_NONE || d.background, "render_bev: null background");
  DN_REQUIRE(d.bg_kind != DN_RENDER_BG_CLASSES || (d.palette && d.n_classes >= 1),
             "render_bev: a class map needs a palette of >= 1 classes");
  if (d.heat) {
    DN_REQUIRE(d.heat_h >= 1 && d.heat_w >= 1 && d.h % d.heat_h == 0 && d.w % d.heat_w == 0,
               "render_bev: a %d x %d heat map does not divide the %d x %d map", d.heat_h, d.heat_w, d.h, d.w);
    DN_REQUIRE(std::isfinite(d.heat_lo) && std::isfinite(d.heat_hi) && d.heat_hi > d.heat_lo,
               "render_bev: heat range [%g, %g], must be finite with hi > lo", d.heat_lo, d.heat_hi);
    DN_REQUIRE(d.heat_alpha >= 0 && d.heat_alpha <= 255, "render_bev: heat_alpha = %d, must be in [0, 255]", d.heat_alpha);
  }
  DN_REQUIRE(d.n_sets >= 0 && d.n_sets <= DN_RENDER_MAX_SETS, "render_bev: %d box sets, at most %d", d.n_sets,
             DN_RENDER_MAX_SETS);
  for (int i = 0; i < d.n_sets; ++i) {
    const dn_render_set& s = d.sets[i];
    DN_REQUIRE(s.boxes, "render_bev: set %d: null boxes", i);
    DN_REQUIRE(s.k >= 1, "render_bev: set %d: k = %d rows, must be >= 1", i, s.k);
    DN_REQUIRE(s.thickness >= 1, "render_bev: set %d: thickness = %d, must be >= 1", i, s.thickness);
    DN_REQUIRE(s.fill_alpha >= 0 && s.fill_alpha <= 255, "render_bev: set %d: fill_alpha = %d, must be in [0, 255]", i,
               s.fill_alpha);
    DN_REQUIRE(s.colour_by == DN_RENDER_COLOUR_FIXED || s.colour_by == DN_RENDER_COLOUR_SCORE ||
               s.colour_by == DN_RENDER_COLOUR_ID, "render_bev: set %d: unknown colour mode %d", i, s.colour_by);
    DN_REQUIRE(s.colour_by != DN_RENDER_COLOUR_SCORE || s.scores, "render_bev: set %d: colour by score needs scores", i);
    DN_REQUIRE(s.colour_by != DN_RENDER_COLOUR_ID || s.ids, "render_bev: set %d: colour by id needs ids", i);
  }
  const int ch = d.h * d.scale, cw = d.w * d.scale;
  const dim3 grid((cw + kTile - 1) / kTile, (ch + kTile - 1) / kTile, d.n);
  DN_REQUIRE(grid.y <= 65535, "render_bev: a canvas of %d rows is too tall", ch);
  hipLaunchKernelGGL(render_bev_kernel, grid, dim3(kThreads), 0, (hipStream_t)stream, d, out);
  return dn::check_launch("render_bev");
}
