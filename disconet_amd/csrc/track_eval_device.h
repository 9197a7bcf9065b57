// The device phases shared by the tracker (track.hip) and the three evaluations of its tracks (mot_eval.hip,
// idf_eval.hip, hota_eval.hip): the rectangle of a row and the IoU of two, the ground-truth measure + dedupe phase, the
// kept-slot lookup of the outputs phases, the compaction of the ids present and the assignment
// (tracking.hungarian_max on one wave).  All of it is contract code: the kernels agree bit for bit with the host
// references of tracking.py, so a change to tie-breaking, the non-finite guard or a status bit is made HERE, once.
// Every kernel that uses it is ONE wave of 64 lanes per workgroup: every phase is a lane-strided loop, the phases hand
// over through LDS with single-wave barriers and every reduction is a wave shuffle or ballot.  Every function that
// touches fp64 is __forceinline__ and carries `#pragma clang fp contract(off)`: the library is built with hipcc's
// default contraction, and a fused multiply-add here would make the device's bits differ from the host reference's.
#pragma once
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>

namespace dn {
namespace trk {

constexpr int kThreads = 64;
constexpr int kMaxM = 128;          // track slots (track.hip) / reported track rows (the evaluations) per image
constexpr int kMaxV = 128;          // valid measured rows used per image: detections (track.hip), ground truths
constexpr int kMaxG = 1024;         // ground-truth rows per image
constexpr int kMaxGtIds = 1024;     // identities per image
constexpr int kMaxTrackIds = 2048;  // track ids per image
constexpr int kLdsPerCu = 160 * 1024;

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }
__device__ __forceinline__ int below(unsigned long long mask, int lane) {
  return __popcll(mask & ((1ull << lane) - 1ull));
}
// The OR of the lanes' status words (bits 1 .. 64), the same in every lane.
__device__ __forceinline__ unsigned wave_or(unsigned flags) {
  unsigned all = 0;
#pragma unroll
  for (unsigned bit = 1u; bit <= 64u; bit <<= 1)
    if (__any(flags & bit)) all |= bit;
  return all;
}

// The rectangle of a row (x, y, w, h, sin, cos): its four corners in the order and arithmetic of tracking._corners (the
// hypot written sqrt(s s + c c): ocml's hypot and the host's do not round alike, sqrt and the four operations do), each
// multiplied by scale, then min / max.  Returns whether every corner is finite.
__device__ __forceinline__ bool row_rect(const float* __restrict__ b, double scale, double* r) {
#pragma clang fp contract(off)
  const double bx = b[0], by = b[1], w = b[2], h = b[3], sn = b[4], cs = b[5];
  const double len = sqrt(sn * sn + cs * cs);
  const double n = len > 1e-12 ? len : (len != len ? len : 1e-12);
  const double s = sn / n, c = cs / n;
  const double dx = w / 2.0, dy = h / 2.0;
  const double lx[4] = {-dx, dx, dx, -dx}, ly[4] = {-dy, -dy, dy, dy};
  double x[4], y[4];
  bool fin = true;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    x[k] = (lx[k] * c - ly[k] * s + bx) * scale;
    y[k] = (lx[k] * s + ly[k] * c + by) * scale;
    fin = fin && isfinite(x[k]) && isfinite(y[k]);
  }
  r[0] = fmin(fmin(x[0], x[1]), fmin(x[2], x[3]));
  r[1] = fmin(fmin(y[0], y[1]), fmin(y[2], y[3]));
  r[2] = fmax(fmax(x[0], x[1]), fmax(x[2], x[3]));
  r[3] = fmax(fmax(y[0], y[1]), fmax(y[2], y[3]));
  return fin;
}

__device__ __forceinline__ double rect_iou(double a0, double a1, double a2, double a3, double b0, double b1, double b2,
                                           double b3) {
#pragma clang fp contract(off)
  const double w = fmin(a2, b2) - fmax(a0, b0);
  const double h = fmin(a3, b3) - fmax(a1, b1);
  if (!(w > 0 && h > 0)) return 0.0;
  const double inter = w * h;
  const double uni = (a2 - a0) * (a3 - a1) + (b2 - b0) * (b3 - b1) - inter;
  return uni > 0 ? inter / uni : 0.0;
}

// The ground truth of one image and frame -> the rows an evaluation uses (tracking._gt_measure), in the caller's LDS
// arrays grect[4][kMaxV], grow[kMaxV], gident[kMaxV]; returns their number V and ORs the status bits into `flags`:
//   measure   lanes over the rows below the count `c`, 64 at a time in row order: the rectangle of the scaled corners
//             must be finite with positive width and height (else bit 2), the id in 0 .. ids - 1 (else bit 4); ballot
//             prefix -> the first kMaxV such rows (a row past them sets bit 1)
//   dedupe    lanes over those rows: one whose id a lower one carries leaves (bit 8), the others close ranks (stable
//             compaction), so grow stays ascending
// `boxes` and `idents` point at the image's rows.  Carries its own barriers, the last one behind the last store: on
// return every lane sees the V rows, and what the caller stored in LDS before the call.  between() runs after the measure
// loop, ahead of the first barrier: the place of a phase of the caller's that needs no kept row and shares that barrier
// (idf_step_kernel's tracks, which stood there before the phases were shared; mot and hota pass nothing).
template <typename Between>
__device__ __forceinline__ int measure_ground_truth(const float* __restrict__ boxes, const int* __restrict__ idents, int c,
                                                    int ids, double scale, int lane, double (*grect)[kMaxV], int* grow,
                                                    int* gident, unsigned& flags, Between between) {
#pragma clang fp contract(off)
  int nv = 0;
  for (int base = 0; base < c; base += kThreads) {
    const int r = base + lane;
    bool ok = false;
    double q[4] = {0, 0, 0, 0};
    int ident = 0;
    if (r < c) {
      const bool fin = row_rect(boxes + 6 * (size_t)r, scale, q);
      if (!(fin && q[2] - q[0] > 0 && q[3] - q[1] > 0)) {
        flags |= 2u;
      } else {
        ident = idents[r];
        if (ident < 0 || ident >= ids) flags |= 4u;
        else ok = true;
      }
    }
    const unsigned long long mask = __ballot(ok);
    const int pos = nv + below(mask, lane);
    if (ok) {
      if (pos < kMaxV) {
        grect[0][pos] = q[0]; grect[1][pos] = q[1]; grect[2][pos] = q[2]; grect[3][pos] = q[3];
        grow[pos] = r;
        gident[pos] = ident;
      } else {
        flags |= 1u;
      }
    }
    nv += __popcll(mask);
  }
  const int V0 = nv < kMaxV ? nv : kMaxV;
  between();
  __syncthreads();

  bool keep[kMaxV / kThreads];
  double kq[kMaxV / kThreads][4];
  int krow[kMaxV / kThreads], kid[kMaxV / kThreads];
#pragma unroll
  for (int h = 0; h < kMaxV / kThreads; ++h) {
    const int j = h * kThreads + lane;
    keep[h] = j < V0;
    krow[h] = 0; kid[h] = 0;
    kq[h][0] = 0; kq[h][1] = 0; kq[h][2] = 0; kq[h][3] = 0;
    if (j < V0) {
      kid[h] = gident[j];
      krow[h] = grow[j];
      kq[h][0] = grect[0][j]; kq[h][1] = grect[1][j]; kq[h][2] = grect[2][j]; kq[h][3] = grect[3][j];
      for (int i = 0; i < j; ++i)
        if (gident[i] == kid[h]) {
          keep[h] = false;
          flags |= 8u;
          break;
        }
    }
  }
  __syncthreads();                                 // every kept row is in registers before a slot is rewritten
  int V = 0;
#pragma unroll
  for (int h = 0; h < kMaxV / kThreads; ++h) {
    const unsigned long long mask = __ballot(keep[h]);
    const int dst = V + below(mask, lane);
    if (keep[h]) {
      grect[0][dst] = kq[h][0]; grect[1][dst] = kq[h][1]; grect[2][dst] = kq[h][2]; grect[3][dst] = kq[h][3];
      grow[dst] = krow[h];
      gident[dst] = kid[h];
    }
    V += __popcll(mask);
  }
  __syncthreads();
  return V;
}

// The slot of ground-truth row r in the ascending list grow[0 .. V) of the rows kept, -1 for a row that was not kept.
__device__ __forceinline__ int kept_slot(const int* grow, int V, int r) {
  int lo = 0, hi = V;                              // first slot with grow >= r
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (grow[mid] < r) lo = mid + 1;
    else hi = mid;
  }
  return lo < V && grow[lo] == r ? lo : -1;
}

// The ids i < n with counts[i] > 0 -> out_ids, ascending (ballot prefix); returns their number.  No barrier: the caller
// places one before another lane reads out_ids.
__device__ __forceinline__ int compact_present(const int* __restrict__ counts, int n, int lane, unsigned short* out_ids) {
  int count = 0;
  for (int base = 0; base < n; base += kThreads) {
    const int i = base + lane;
    const bool on = i < n && counts[i] > 0;
    const unsigned long long mask = __ballot(on);
    if (on) out_ids[count + below(mask, lane)] = (unsigned short)i;
    count += __popcll(mask);
  }
  return count;
}

// tracking.hungarian_max to the letter on one wave: the shortest-augmenting-path assignment of n rows to mm >= n columns
// at the least total cost, lanes over columns.  cost_of(row, column) -> double, both 0-based, is called once per lane,
// column stride and step; a step is that read and one wave arg-min (the lowest column among equals).  hu[n + 1],
// hv / hminv / hp / hway / hused[mm + 1] are the caller's LDS; on return hp[j], j = 1 .. mm, is the row (1-based) that
// took column j, else 0 -- a value read back from LDS, so the caller clamps it as every index here is clamped.  A row's
// search is cut after mm + 1 steps whatever the numbers are, so the whole costs at most n (mm + 1) steps; a row that
// reaches nothing (non-finite costs only) stays free.  Such a row leaves its number in hp[0]: hp[0] is rewritten at the
// top of the next row and no read-out starts below j = 1, so it is not cleared.  Begins with the initialisation and a
// barrier and ends with a barrier behind the last path rewrite.
template <typename Index, typename Used, typename Cost>
__device__ __forceinline__ void assign_rows(int n, int mm, int lane, double* hu, double* hv, double* hminv, Index* hp,
                                            Index* hway, Used* hused, Cost cost_of) {
#pragma clang fp contract(off)
  const double inf = HUGE_VAL;
  for (int j = lane; j <= mm; j += kThreads) {
    hv[j] = 0.0; hp[j] = 0; hway[j] = 0;
  }
  for (int i = lane; i <= n; i += kThreads) hu[i] = 0.0;
  __syncthreads();
  for (int i = 1; i <= n; ++i) {
    for (int j = lane; j <= mm; j += kThreads) {
      hminv[j] = inf; hused[j] = 0;
    }
    if (lane == 0) hp[0] = (Index)i;
    __syncthreads();
    int j0 = 0;
    bool found = false;
    for (int step = 0; step <= mm; ++step) {
      if (lane == 0) hused[j0] = 1;
      __syncthreads();
      const int i0 = hp[j0] < 1 ? 1 : (hp[j0] > n ? n : hp[j0]);
      const double ui0 = hu[i0];
      double best = inf;
      int bj = INT_MAX;
      for (int j = 1 + lane; j <= mm; j += kThreads) {
        if (hused[j]) continue;
        const double cost = cost_of(i0 - 1, j - 1);
        const double cur = (cost - ui0) - hv[j];
        double mv = hminv[j];
        if (cur < mv) {
          mv = cur; hminv[j] = cur; hway[j] = (Index)j0;
        }
        if (mv < best) {
          best = mv; bj = j;
        }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const double ob = __shfl_xor(best, o);
        const int oj = __shfl_xor(bj, o);
        if (ob < best || (ob == best && oj < bj)) {
          best = ob; bj = oj;
        }
      }
      if (bj == INT_MAX) break;                    // nothing to reach (non-finite input only): the row stays free
      __syncthreads();
      for (int j = lane; j <= mm; j += kThreads) {
        if (hused[j]) {
          const int row = clampi(hp[j], n);
          hu[row] = hu[row] + best;
          hv[j] = hv[j] - best;
        } else {
          hminv[j] = hminv[j] - best;
        }
      }
      j0 = bj;
      __syncthreads();
      if (hp[j0] == 0) {
        found = true;
        break;
      }
    }
    __syncthreads();                               // every lane has read hp[j0] before the path is rewritten
    if (found && lane == 0) {
      for (int s = 0; s <= mm; ++s) {
        const int j1 = clampi(hway[j0], mm);
        hp[j0] = hp[j1];
        j0 = j1;
        if (j0 == 0) break;
      }
    }
    __syncthreads();
  }
}

}  // namespace trk
}  // namespace dn
