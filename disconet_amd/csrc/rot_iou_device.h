// Box geometry shared by the kernels that decide from rotated-box IoU in fp64: the NMS of dn_detect and dn_late_fuse
// (detect.hip), the ground-truth matching of dn_ap_match / dn_ap_match_strata (ap_match.hip) and the anchor assignment
// of dn_assign_targets (assign.hip).  Corners, the circumscribed-circle test, the polygon clip and the IoU are operation
// for operation postprocess._corners / _intersection_area / nms_rotated.  All of it is contract code: a detection that is
// a true positive for dn_ap_match at IoU v is the box dn_detect suppresses at any threshold below v, because both run the
// pair body below -- so a change to the circle test, a guard or the staging is made HERE, once.  Every function carries `#pragma clang fp contract(off)`: the library is built with hipcc's default contraction, and a
// fused multiply-add here would make the device's decisions differ from the host reference's.
#pragma once
#include <hip/hip_runtime.h>

namespace dn {

constexpr int kClipCap = 12;        // vertices of a clipped polygon kept per lane (a convex quad clipped 4 times has <= 8)
constexpr int kMaxBoxRows = 1024;   // box rows per image: dn_detect's top_k, dn_late_fuse's k_in, dn_ap_match's K
constexpr int kMaxGtRows = 1024;    // ground-truth rows per image
constexpr int kMaxImages = 65535;   // images per call (a grid dimension)

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

struct Box64 {
  double x[4], y[4];
  double cx, cy, radius, area;
};

__device__ inline void box64(const float* __restrict__ b, Box64& o) {
#pragma clang fp contract(off)
  const double bx = b[0], by = b[1], w = b[2], h = b[3], sn = b[4], cs = b[5];
  const double n = fmax(hypot(sn, cs), 1e-12);
  const double s = sn / n, c = cs / n;
  const double dx = w / 2.0, dy = h / 2.0;
  const double lx[4] = {-dx, dx, dx, -dx}, ly[4] = {-dy, -dy, dy, dy};
  for (int k = 0; k < 4; ++k) {
    o.x[k] = lx[k] * c - ly[k] * s + bx;
    o.y[k] = lx[k] * s + ly[k] * c + by;
  }
  o.cx = bx;
  o.cy = by;
  o.radius = 0.5 * hypot(w, h);
  o.area = w * h;
}

// Area of (quad a) clipped by the four edges of quad b (Sutherland-Hodgman).  The polygons live in LDS, one column per
// lane: px/py/qx/qy point at vertex 0 of this lane's column, vertex v is at [64 * v].
__device__ inline double intersection_area(const double* ax, const double* ay, const double* bx, const double* by,
                                           double* px, double* py, double* qx, double* qy) {
#pragma clang fp contract(off)
  int n = 4;
  for (int k = 0; k < 4; ++k) {
    px[64 * k] = ax[k];
    py[64 * k] = ay[k];
  }
  for (int e = 0; e < 4; ++e) {
    const double a0 = bx[e], a1 = by[e], b0 = bx[(e + 1) & 3], b1 = by[(e + 1) & 3];
    int m = 0;
    for (int k = 0; k < n; ++k) {
      const int k1 = k + 1 == n ? 0 : k + 1;
      const double p0 = px[64 * k], p1 = py[64 * k], q0 = px[64 * k1], q1 = py[64 * k1];
      const double sp = (b0 - a0) * (p1 - a1) - (b1 - a1) * (p0 - a0);
      const double sq = (b0 - a0) * (q1 - a1) - (b1 - a1) * (q0 - a0);
      if (sp >= 0) {
        if (m < kClipCap) {
          qx[64 * m] = p0;
          qy[64 * m] = p1;
        }
        ++m;
      }
      if (sp * sq < 0) {
        const double t = sp / (sp - sq);
        if (m < kClipCap) {
          qx[64 * m] = p0 + t * (q0 - p0);
          qy[64 * m] = p1 + t * (q1 - p1);
        }
        ++m;
      }
    }
    n = m < kClipCap ? m : kClipCap;
    double* t;
    t = px; px = qx; qx = t;
    t = py; py = qy; qy = t;
    if (n < 3) return 0.0;
  }
  double s1 = 0.0, s2 = 0.0;
  for (int k = 0; k < n; ++k) {
    const int k1 = k + 1 == n ? 0 : k + 1;
    s1 = s1 + px[64 * k] * py[64 * k1];
    s2 = s2 + py[64 * k] * px[64 * k1];
  }
  return 0.5 * fabs(s1 - s2);
}

// N boxes of one image in LDS, the columns a 64-lane wave tests its rows against.
template <int N>
struct BoxColumns {
  double x[4][N], y[4][N], cx[N], cy[N], radius[N], area[N];
};

// Lane t < rows stages row t of `boxes` (float6 rows) as column t; the caller's barrier follows.
template <int N>
__device__ __forceinline__ void stage_columns(BoxColumns<N>& c, const float* __restrict__ boxes, int rows, int t) {
  if (t < rows) {
    Box64 b;
    box64(boxes + 6 * (size_t)t, b);
    for (int q = 0; q < 4; ++q) {
      c.x[q][t] = b.x[q];
      c.y[q][t] = b.y[q];
    }
    c.cx[t] = b.cx;
    c.cy[t] = b.cy;
    c.radius[t] = b.radius;
    c.area[t] = b.area;
  }
}

// The two ping-pong polygons of intersection_area for each of a wave's 64 lanes.
struct ClipScratch {
  double x[2][kClipCap][64], y[2][kClipCap][64];
  __device__ __forceinline__ double clip(const double* ax, const double* ay, const double* bx, const double* by, int lane) {
    return intersection_area(ax, ay, bx, by, &x[0][0][lane], &y[0][0][lane], &x[1][0][lane], &y[1][0][lane]);
  }
};

// The strict circumscribed-circle test of the host reference.  The squared-distance comparison in front of it only
// spares the hypot of pairs that are far apart: its bound is a hundredth wider than the circles' sum, far beyond any
// rounding, so it never rejects a pair that the test itself would pass.  A NaN makes the comparison false and the pair
// goes on to the strict test; an infinite distance under a finite reach is rejected by both.
template <int N>
__device__ __forceinline__ bool circles_meet(const BoxColumns<N>& c, int jj, const Box64& a) {
#pragma clang fp contract(off)
  const double dx = c.cx[jj] - a.cx, dy = c.cy[jj] - a.cy, reach = c.radius[jj] + a.radius;
  if (dx * dx + dy * dy > 1.01 * reach * reach + 1e-12) return false;
  return hypot(dx, dy) < reach;
}

// IoU of box a and column jj; 0 when the union is not positive (or not a number).
template <int N>
__device__ __forceinline__ double pair_iou(const BoxColumns<N>& c, int jj, const Box64& a, ClipScratch& scratch,
                                           int lane) {
#pragma clang fp contract(off)
  double bx[4], by[4];
  for (int q = 0; q < 4; ++q) {
    bx[q] = c.x[q][jj];
    by[q] = c.y[q][jj];
  }
  const double inter = scratch.clip(a.x, a.y, bx, by, lane);
  const double uni = a.area + c.area[jj] - inter;
  return uni > 0 ? inter / uni : 0.0;
}

}  // namespace dn
