// Rotated-box IoU in fp64, operation for operation postprocess._corners / _intersection_area: the geometry shared by
// the NMS of detect.hip and the ground-truth matching of ap_match.hip.  Every function carries
// `#pragma clang fp contract(off)`: the library is built with hipcc's default contraction, and a fused multiply-add
// here would make the device's decisions differ from the host reference's.
#pragma once
#include <hip/hip_runtime.h>

namespace dn {

constexpr int kClipCap = 12;   // vertices of a clipped polygon kept per lane (a convex quad clipped 4 times has <= 8)

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

}  // namespace dn
