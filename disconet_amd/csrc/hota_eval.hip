// HOTA of the tracks (beside the CLEAR figures of mot_eval.hip and the identity figures of idf_eval.hip): the frame
// matching is weighted by a global alignment score that is known only after the last frame, so the sequence is seen
// twice.  Per frame the step adds to the potential-match matrix and LOGS the frame's rectangles in the device state; at
// the end the finish matches every logged frame, all frames of all images at once.  The contract is in
// include/disconet_hip.h; the host reference that defines the bits is tracking.HostHota.  All arithmetic is fp64 in a fixed
// order, + - * / and sqrt only, and every function that touches fp64 carries `#pragma clang fp contract(off)`.
//
// hota_step_kernel: one launch per frame, one workgroup of ONE wave per image, as mot_step_kernel and idf_step_kernel (the
// measure and dedupe phases and row_rect / rect_iou are copied here; mot_eval.hip and idf_eval.hip are not touched):
//   measure    lanes over ground-truth rows, 64 at a time in row order -> the first 128 valid rows in LDS
//   dedupe     a kept row whose id a lower kept row carries leaves (stable compaction)
//   tracks     lanes over reported rows: the id's range (status bit 16), an id a lower row carries (bit 64), ballot prefix
//              -> the columns in LDS, in row order
//   iou        lanes over (ground truth, column) pairs -> the matrix in LDS, [ground truths][ld], ld odd as in mot_eval.hip
//   sums       lanes over rows (rs) and over columns (cs), each a serial walk in ascending order
//   potential  lanes over rows, each walks its columns in ascending order: one term per overlapping pair into the cell of
//              the state that only this lane touches in this call (ids are unique in a frame): no atomics
//   log        lanes over rows and over columns: the slot is written once in its life (reset zeroed what stays unused)
//   counts     gt_count / track_count by the lane that owns the row / column; one lane adds to the header
//   outputs    lanes over ground-truth rows; every word of `out_potential` is written once
// 8 * min(g, 128) * (m | 1) bytes of dynamic LDS beside 13 KB of work arrays.
//
// hota_match_kernel: a grid of (max_frames, n_images) workgroups of ONE wave; a block whose slot is not logged clears its
// row of out_match and returns.  The slot's ids and rectangles -> LDS; lanes over pairs: the IoU again (same function, same
// bits), times the alignment score A of the pair's cell (read from pot, gt_count, track_count in place) -> the score matrix
// in LDS, [V][C | 1]; the shortest-augmenting-path step of mot_eval.hip (its own copy, lanes over columns); per kept pair
// the IoU once more and K, the number of alphas it counts at; one integer atomic per kept pair into the cell's 20-bin
// histogram in `work`; lane k < 19 walks the rows in ascending order for the frame's TP_k (one integer atomic per alpha
// into `work`) and its loc partial (written to the frame's own words of `work`, never added atomically).
// V and C come from the log, so the launch reserves the largest matrix whatever the arguments are: 8 * 128 * 129 B of
// dynamic LDS beside 17 KB of work arrays, one workgroup per CU.
//
// hota_fold_kernel: one workgroup of one wave per image.  The track ids present are compacted into LDS (ballot prefix);
// the identities present are taken 64 at a time in ascending order, one per lane: the lane walks the present track ids in
// ascending order, turns a cell's bins into the 19 matched counts (suffix sums) and adds the cell's three terms per alpha
// to its row sums; the row sums go to LDS and lanes 0..56 (one per alpha and sum) add the chunk's rows to their running
// totals in ascending identity order.  Lane k < 19 adds the frames' loc partials in slot order and writes the alpha's
// words.  Nothing is read back, nothing is allocated; two runs write the same bytes.
#include <climits>
#include <cmath>

#include "dn_internal.h"

namespace {

constexpr int kThreads = 64;
constexpr int kMaxM = 128;          // reported track rows per image
constexpr int kMaxV = 128;          // valid ground-truth rows used per image
constexpr int kMaxG = 1024;         // ground-truth rows per image
constexpr int kMaxGtIds = 1024;     // identities per image
constexpr int kMaxTrackIds = 2048;  // track ids per image
constexpr int kMaxFrames = 4096;    // log slots per image
constexpr int kHeaderBytes = 64;    // int64 frames, logged, gt_dets, dets; int32 status; 28 spare bytes
constexpr int kSlotBytes = 16 + 4 * (kMaxV + kMaxM) + 32 * (kMaxV + kMaxM);   // 9232
constexpr int kAlphas = 19;
constexpr int kBins = 20;           // K = 0 .. 19 of a kept pair
constexpr int kMatchLd = kMaxM | 1;
constexpr int kLdsPerCu = 160 * 1024;
constexpr double kEps = 2.220446049250313e-16;   // 2^-52

struct Params {
  int m, g, ids, tids, frames, ld;
  double scale;
};

__host__ __device__ inline size_t image_bytes(int ids, int tids, int frames) {
  const size_t raw = (size_t)kHeaderBytes + 8 * (size_t)ids * (size_t)tids + (size_t)kSlotBytes * (size_t)frames +
                     4 * ((size_t)ids + (size_t)tids);
  return (raw + 7) & ~(size_t)7;
}
// work, per image: int64 tp[20]; fp64 loc partial [frames][20]; int32 hist[ids][tids][20]
__host__ __device__ inline size_t work_image_bytes(int ids, int tids, int frames) {
  return 8 * (size_t)kBins + 8 * (size_t)kBins * (size_t)frames + 4 * (size_t)kBins * (size_t)ids * (size_t)tids;
}

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }
__device__ __forceinline__ int below(unsigned long long mask, int lane) {
  return __popcll(mask & ((1ull << lane) - 1ull));
}

// The rectangle of a row (x, y, w, h, sin, cos): its four corners in the order and arithmetic of tracking._corners (the
// hypot written sqrt(s s + c c)), each multiplied by scale, then min / max.  Returns whether every corner is finite.
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

__global__ void __launch_bounds__(kThreads) hota_step_kernel(const double* __restrict__ rect, const int* __restrict__ tid,
                                                             const int* __restrict__ tcount,
                                                             const float* __restrict__ gt_boxes,
                                                             const int* __restrict__ gt_ids,
                                                             const int* __restrict__ gt_count, Params p,
                                                             unsigned char* __restrict__ state,
                                                             double* __restrict__ out_potential) {
#pragma clang fp contract(off)
  extern __shared__ double iou_m[];                // [ground truths][p.ld]
  __shared__ double grect[4][kMaxV], trect[4][kMaxM], rs[kMaxV], cs[kMaxM], prow[kMaxV];
  __shared__ int grow[kMaxV], gident[kMaxV];
  __shared__ int traw[kMaxM], ctid[kMaxM], cfin[kMaxM];
  const int img = blockIdx.x, lane = threadIdx.x;
  const int m = p.m, g = p.g, ids = p.ids, tids = p.tids, ld = p.ld;
  unsigned char* st = state + (size_t)img * image_bytes(ids, tids, p.frames);
  long long* hdr = reinterpret_cast<long long*>(st);
  int* status = reinterpret_cast<int*>(st) + 8;
  double* pot = reinterpret_cast<double*>(st + kHeaderBytes);                          // [ids][tids]
  unsigned char* slots = st + kHeaderBytes + 8 * (size_t)ids * (size_t)tids;
  int* gcnt = reinterpret_cast<int*>(slots + (size_t)kSlotBytes * (size_t)p.frames);   // [ids]
  int* tcnt = gcnt + ids;                                                              // [tids]
  unsigned flags = 0;

  // ---- the log is full: the frame is counted and nothing else changes
  const long long logged = hdr[1];
  __syncthreads();                                 // every lane has read the header before one lane rewrites it
  if (logged < 0 || logged >= p.frames) {          // wave-uniform
    if (lane == 0) {
      hdr[0] = hdr[0] + 1;
      *status = *status | 32;
    }
    for (int r = lane; r < g; r += kThreads) out_potential[(size_t)img * g + r] = 0.0;
    return;
  }

  // ---- measure: the first kMaxV valid ground-truth rows, in row order
  const int c = clampi(gt_count[img], g);
  int nv = 0;
  for (int base = 0; base < c; base += kThreads) {
    const int r = base + lane;
    bool ok = false;
    double q[4] = {0, 0, 0, 0};
    int ident = 0;
    if (r < c) {
      const bool fin = row_rect(gt_boxes + 6 * ((size_t)img * g + r), p.scale, q);
      if (!(fin && q[2] - q[0] > 0 && q[3] - q[1] > 0)) {
        flags |= 2u;
      } else {
        ident = gt_ids[(size_t)img * g + r];
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
  // the reported rows' ids
  const int K = clampi(tcount[img], m);
  for (int t = lane; t < K; t += kThreads) traw[t] = tid[(size_t)img * m + t];
  __syncthreads();

  // ---- tracks: the columns, in row order
  int C = 0;
  for (int base = 0; base < K; base += kThreads) {
    const int t = base + lane;
    bool col = false;
    int track = 0;
    if (t < K) {
      track = traw[t];
      if (track < 1 || track > tids) {
        flags |= 16u;
      } else {
        col = true;
        for (int i = 0; i < t; ++i)
          if (traw[i] == track) {
            col = false;
            flags |= 64u;
            break;
          }
      }
    }
    const unsigned long long mask = __ballot(col);
    if (col) {
      const int dst = C + below(mask, lane);
      const double* r = rect + 4 * ((size_t)img * m + t);
      const double r0 = r[0], r1 = r[1], r2 = r[2], r3 = r[3];
      trect[0][dst] = r0; trect[1][dst] = r1; trect[2][dst] = r2; trect[3][dst] = r3;
      cfin[dst] = isfinite(r0) && isfinite(r1) && isfinite(r2) && isfinite(r3) ? 1 : 0;
      ctid[dst] = track;
    }
    C += __popcll(mask);
  }

  // ---- dedupe: a kept row whose id a lower kept row carries leaves; the others close ranks
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

  // ---- iou: lanes over (ground truth, column)
  for (int e = lane; e < V * C; e += kThreads) {
    const int a = e / C, t = e - a * C;
    iou_m[a * ld + t] = cfin[t] ? rect_iou(grect[0][a], grect[1][a], grect[2][a], grect[3][a], trect[0][t], trect[1][t],
                                           trect[2][t], trect[3][t])
                                : 0.0;
  }
  __syncthreads();
  // ---- sums: a row's over its columns, a column's over its rows, ascending from 0.0
  for (int a = lane; a < V; a += kThreads) {
    double s = 0.0;
    for (int t = 0; t < C; ++t) s = s + iou_m[a * ld + t];
    rs[a] = s;
  }
  for (int t = lane; t < C; t += kThreads) {
    double s = 0.0;
    for (int a = 0; a < V; ++a) s = s + iou_m[a * ld + t];
    cs[t] = s;
  }
  __syncthreads();
  // ---- potential: a cell belongs to one (row, column) of this frame, a row to one lane
  for (int a = lane; a < V; a += kThreads) {
    double* cells = pot + (size_t)gident[a] * tids;
    const double ra = rs[a];
    double sum = 0.0;
    for (int t = 0; t < C; ++t) {
      const double s = iou_m[a * ld + t];
      if (s > 0) {
        const double term = s / ((ra + cs[t]) - s);
        cells[ctid[t] - 1] = cells[ctid[t] - 1] + term;
        sum = sum + term;
      }
    }
    prow[a] = sum;
  }

  // ---- log: the slot is written once; what stays unused was zeroed by the reset
  unsigned char* slot = slots + (size_t)kSlotBytes * (size_t)logged;
  int* sint = reinterpret_cast<int*>(slot);
  double* srect = reinterpret_cast<double*>(slot + 16 + 4 * (kMaxV + kMaxM));          // gt [128][4], then track [128][4]
  for (int a = lane; a < V; a += kThreads) {
    sint[4 + a] = gident[a];
    srect[4 * a + 0] = grect[0][a]; srect[4 * a + 1] = grect[1][a];
    srect[4 * a + 2] = grect[2][a]; srect[4 * a + 3] = grect[3][a];
    gcnt[gident[a]] = gcnt[gident[a]] + 1;
  }
  for (int t = lane; t < C; t += kThreads) {
    sint[4 + kMaxV + t] = ctid[t];
    double* d = srect + 4 * kMaxV + 4 * t;
    d[0] = trect[0][t]; d[1] = trect[1][t]; d[2] = trect[2][t]; d[3] = trect[3][t];
    tcnt[ctid[t] - 1] = tcnt[ctid[t] - 1] + 1;
  }
  const unsigned all = (__any(flags & 1u) ? 1u : 0u) | (__any(flags & 2u) ? 2u : 0u) | (__any(flags & 4u) ? 4u : 0u) |
                       (__any(flags & 8u) ? 8u : 0u) | (__any(flags & 16u) ? 16u : 0u) | (__any(flags & 64u) ? 64u : 0u);
  if (lane == 0) {
    sint[0] = V;
    sint[1] = C;
    hdr[0] = hdr[0] + 1;
    hdr[1] = logged + 1;
    hdr[2] = hdr[2] + V;
    hdr[3] = hdr[3] + C;
    *status = *status | (int)all;
  }
  __syncthreads();

  // ---- outputs: every row once; a kept row is found in the ascending list of the rows kept
  for (int r = lane; r < g; r += kThreads) {
    int lo = 0, hi = V;                            // first slot with grow >= r
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (grow[mid] < r) lo = mid + 1;
      else hi = mid;
    }
    out_potential[(size_t)img * g + r] = lo < V && grow[lo] == r ? prow[lo] : 0.0;
  }
}

__global__ void __launch_bounds__(kThreads) hota_match_kernel(const unsigned char* __restrict__ state, int ids, int tids,
                                                              int frames, unsigned char* __restrict__ work,
                                                              int* __restrict__ out_match) {
#pragma clang fp contract(off)
  extern __shared__ double score_m[];              // [ground truths][ld]
  __shared__ double grect[4][kMaxV], trect[4][kMaxM], siou[kMaxV];
  __shared__ int gident[kMaxV], tident[kMaxM], tfin[kMaxM], took[kMaxV], kcount[kMaxV];
  __shared__ double hu[kMaxM + 1], hv[kMaxM + 1], hminv[kMaxM + 1];
  __shared__ int hp[kMaxM + 1], hway[kMaxM + 1], hused[kMaxM + 1];
  const int f = blockIdx.x, img = blockIdx.y, lane = threadIdx.x;
  const unsigned char* st = state + (size_t)img * image_bytes(ids, tids, frames);
  const long long* hdr = reinterpret_cast<const long long*>(st);
  const double* pot = reinterpret_cast<const double*>(st + kHeaderBytes);
  const unsigned char* slots = st + kHeaderBytes + 8 * (size_t)ids * (size_t)tids;
  const int* gcnt = reinterpret_cast<const int*>(slots + (size_t)kSlotBytes * (size_t)frames);
  const int* tcnt = gcnt + ids;
  int* mrow = out_match ? out_match + ((size_t)img * frames + f) * kMaxV : nullptr;
  if ((long long)f >= hdr[1]) {                    // wave-uniform: the slot is not logged
    if (mrow)
      for (int a = lane; a < kMaxV; a += kThreads) mrow[a] = 0;
    return;
  }
  unsigned char* wk = work + (size_t)img * work_image_bytes(ids, tids, frames);
  unsigned long long* tp = reinterpret_cast<unsigned long long*>(wk);                  // [20]
  double* locp = reinterpret_cast<double*>(wk + 8 * kBins) + (size_t)kBins * f;        // this frame's [20]
  int* hist = reinterpret_cast<int*>(wk + 8 * (size_t)kBins * (1 + (size_t)frames));   // [ids][tids][20]

  // ---- the slot
  const unsigned char* slot = slots + (size_t)kSlotBytes * (size_t)f;
  const int* sint = reinterpret_cast<const int*>(slot);
  const double* srect = reinterpret_cast<const double*>(slot + 16 + 4 * (kMaxV + kMaxM));
  const int V = clampi(sint[0], kMaxV), K = clampi(sint[1], kMaxM);
  const int ld = K | 1;
  for (int a = lane; a < V; a += kThreads) {
    gident[a] = clampi(sint[4 + a], ids - 1);
    grect[0][a] = srect[4 * a + 0]; grect[1][a] = srect[4 * a + 1];
    grect[2][a] = srect[4 * a + 2]; grect[3][a] = srect[4 * a + 3];
    took[a] = -1;
  }
  for (int t = lane; t < K; t += kThreads) {
    const int track = sint[4 + kMaxV + t];
    tident[t] = track < 1 ? 1 : (track > tids ? tids : track);
    const double* r = srect + 4 * kMaxV + 4 * t;
    const double r0 = r[0], r1 = r[1], r2 = r[2], r3 = r[3];
    trect[0][t] = r0; trect[1][t] = r1; trect[2][t] = r2; trect[3][t] = r3;
    tfin[t] = isfinite(r0) && isfinite(r1) && isfinite(r2) && isfinite(r3) ? 1 : 0;
  }
  __syncthreads();

  // ---- score = the pair's alignment score x its IoU
  for (int e = lane; e < V * K; e += kThreads) {
    const int a = e / K, t = e - a * K;
    const double s = tfin[t] ? rect_iou(grect[0][a], grect[1][a], grect[2][a], grect[3][a], trect[0][t], trect[1][t],
                                        trect[2][t], trect[3][t])
                             : 0.0;
    const int i = gident[a], j = tident[t] - 1;
    const double pw = pot[(size_t)i * tids + j];
    const double al = pw > 0 ? pw / ((double)(gcnt[i] + tcnt[j]) - pw) : 0.0;
    score_m[a * ld + t] = al * s;
  }
  __syncthreads();

  // ---- assign: tracking.hungarian_max(score), rows the smaller side
  if (V > 0 && K > 0) {   // wave-uniform
    const bool tp_ = V > K;                        // rows are the tracks when there are more ground truths
    const int n = tp_ ? K : V, mm = tp_ ? V : K;
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
      if (lane == 0) hp[0] = i;
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
          const double cost = -(tp_ ? score_m[(j - 1) * ld + (i0 - 1)] : score_m[(i0 - 1) * ld + (j - 1)]);
          const double cur = (cost - ui0) - hv[j];
          double mv = hminv[j];
          if (cur < mv) {
            mv = cur; hminv[j] = cur; hway[j] = j0;
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
        if (bj == INT_MAX) break;                  // nothing to reach (non-finite input only): the row stays free
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
      __syncthreads();                             // every lane has read hp[j0] before the path is rewritten
      if (lane == 0) {
        if (found) {
          for (int s = 0; s <= mm; ++s) {
            const int j1 = clampi(hway[j0], mm);
            hp[j0] = hp[j1];
            j0 = j1;
            if (j0 == 0) break;
          }
        } else {
          hp[0] = 0;
        }
      }
      __syncthreads();
    }
    for (int j = 1 + lane; j <= mm; j += kThreads) {
      const int i = clampi(hp[j], n);
      if (i > 0) took[tp_ ? j - 1 : i - 1] = tp_ ? i - 1 : j - 1;
    }
    __syncthreads();
  }

  // ---- the kept pairs: score > 0; the IoU again, the number of alphas it counts at, the cell's histogram
  for (int a = lane; a < V; a += kThreads) {
    const int t = took[a];
    double s = 0.0;
    int kc = -1;                                   // -1: no kept pair
    if (t >= 0 && score_m[a * ld + t] > 0) {
      s = rect_iou(grect[0][a], grect[1][a], grect[2][a], grect[3][a], trect[0][t], trect[1][t], trect[2][t], trect[3][t]);
      kc = 0;
#pragma unroll
      for (int k = 0; k < kAlphas; ++k) {
        const double thr = 0.05 * (double)(k + 1) - kEps;
        if (!(s < thr)) ++kc;
      }
      atomicAdd(&hist[((size_t)gident[a] * tids + (tident[t] - 1)) * kBins + kc], 1);
    }
    siou[a] = s;
    kcount[a] = kc;
    if (mrow) mrow[a] = kc >= 0 ? tident[t] : 0;
  }
  if (mrow)
    for (int a = V + lane; a < kMaxV; a += kThreads) mrow[a] = 0;
  __syncthreads();
  // ---- per alpha: the frame's TP and its loc partial, rows ascending
  if (lane < kBins) {
    double loc = 0.0;
    int n_tp = 0;
    if (lane < kAlphas)
      for (int a = 0; a < V; ++a)
        if (kcount[a] > lane) {
          loc = loc + siou[a];
          ++n_tp;
        }
    locp[lane] = loc;
    if (n_tp > 0) atomicAdd(&tp[lane], (unsigned long long)n_tp);
  }
}

constexpr int kSums = 3 * kAlphas;   // assa, assre, asspr per alpha

__global__ void __launch_bounds__(kThreads) hota_fold_kernel(const unsigned char* __restrict__ state, int ids, int tids,
                                                             int frames, const unsigned char* __restrict__ work,
                                                             long long* __restrict__ out_counts,
                                                             long long* __restrict__ out_alpha_counts,
                                                             double* __restrict__ out_alpha_sums) {
#pragma clang fp contract(off)
  __shared__ unsigned short colid[kMaxTrackIds];
  __shared__ double rows[kThreads][kSums | 1];     // a chunk's row sums: [identity of the chunk][alpha x sum]
  __shared__ int present[kThreads];
  const int img = blockIdx.x, lane = threadIdx.x;
  const unsigned char* st = state + (size_t)img * image_bytes(ids, tids, frames);
  const long long* hdr = reinterpret_cast<const long long*>(st);
  const unsigned char* slots = st + kHeaderBytes + 8 * (size_t)ids * (size_t)tids;
  const int* gcnt = reinterpret_cast<const int*>(slots + (size_t)kSlotBytes * (size_t)frames);
  const int* tcnt = gcnt + ids;
  const unsigned char* wk = work + (size_t)img * work_image_bytes(ids, tids, frames);
  const long long* tp = reinterpret_cast<const long long*>(wk);
  const double* locp = reinterpret_cast<const double*>(wk + 8 * kBins);
  const int* hist = reinterpret_cast<const int*>(wk + 8 * (size_t)kBins * (1 + (size_t)frames));

  // ---- the track ids present, ascending
  int C = 0;
  for (int base = 0; base < tids; base += kThreads) {
    const int i = base + lane;
    const bool on = i < tids && tcnt[i] > 0;
    const unsigned long long mask = __ballot(on);
    if (on) colid[C + below(mask, lane)] = (unsigned short)i;
    C += __popcll(mask);
  }
  __syncthreads();

  // ---- the association sums: identities 64 at a time, one per lane; lanes 0..56 keep the running totals
  int R = 0;
  double total = 0.0;
  for (int base = 0; base < ids; base += kThreads) {
    const int i = base + lane;
    const int gc = i < ids ? gcnt[i] : 0;
    const unsigned long long on = __ballot(gc > 0);
    R += __popcll(on);
    if (on == 0ull) continue;                      // wave-uniform
    double acc[kSums];
#pragma unroll
    for (int q = 0; q < kSums; ++q) acc[q] = 0.0;
    if (gc > 0) {
      const int* hrow = hist + (size_t)i * tids * kBins;
      for (int jj = 0; jj < C; ++jj) {
        const int j = colid[jj];
        const int* bins = hrow + (size_t)j * kBins;
        int b[kBins];
        int any = 0;
#pragma unroll
        for (int k = 0; k < kBins; ++k) {
          b[k] = bins[k];
          any |= b[k];
        }
        if (any == 0) continue;
        const double tc = (double)tcnt[j], both = (double)(gc + tcnt[j]);
        int cnt = 0;
#pragma unroll
        for (int k = kAlphas - 1; k >= 0; --k) {   // c_k = the bins above k
          cnt += b[k + 1];
          if (cnt > 0) {
            const double cd = (double)cnt;
            acc[3 * k + 0] = acc[3 * k + 0] + cd * (cd / (both - cd));
            acc[3 * k + 1] = acc[3 * k + 1] + cd * (cd / (double)gc);
            acc[3 * k + 2] = acc[3 * k + 2] + cd * (cd / tc);
          }
        }
      }
    }
    __syncthreads();                               // the totals of the chunk before have been taken
#pragma unroll
    for (int q = 0; q < kSums; ++q) rows[lane][q] = acc[q];
    present[lane] = gc > 0 ? 1 : 0;
    __syncthreads();
    if (lane < kSums)
      for (int r = 0; r < kThreads; ++r)
        if (present[r]) total = total + rows[r][lane];
  }

  // ---- outputs: every word once
  double* sums = out_alpha_sums + 4 * (size_t)kAlphas * img;
  if (lane < kSums) sums[4 * (lane / 3) + 1 + lane % 3] = total;
  if (lane < kAlphas) {
    const long long logged = hdr[1] < 0 ? 0 : (hdr[1] > frames ? frames : hdr[1]);
    double loc = 0.0;
    for (long long f = 0; f < logged; ++f) loc = loc + locp[(size_t)kBins * f + lane];
    sums[4 * lane + 0] = loc;
    long long* o = out_alpha_counts + 4 * ((size_t)kAlphas * img + lane);
    o[0] = tp[lane];
    o[1] = hdr[2] - tp[lane];
    o[2] = hdr[3] - tp[lane];
    o[3] = 0;
  }
  if (lane == 0) {
    long long* o = out_counts + 8 * (size_t)img;
    o[0] = hdr[0];
    o[1] = hdr[1];
    o[2] = hdr[2];
    o[3] = hdr[3];
    o[4] = R;
    o[5] = C;
    o[6] = reinterpret_cast<const int*>(st)[8];
    o[7] = 0;
  }
}

bool shapes_ok(int n, int ids, int tids, int frames) {
  return n > 0 && n <= 65535 && ids >= 1 && ids <= kMaxGtIds && tids >= 1 && tids <= kMaxTrackIds && frames >= 1 &&
         frames <= kMaxFrames;
}

// the kernel's static LDS, read once per device
int static_lds_of(const void* kernel, dn::PerDeviceFlag& flag, int* cache, int dynamic_most) {
  int dev = 0;
  (void)hipGetDevice(&dev);
  bool& ready = flag.here();
  if (!ready) {
    hipFuncAttributes attr;
    if (hipFuncGetAttributes(&attr, kernel) != hipSuccess) return -1;
    if (dynamic_most > 0 &&
        hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, dynamic_most) != hipSuccess)
      return -2;
    cache[dev & 63] = (int)attr.sharedSizeBytes;
    ready = true;
  }
  return cache[dev & 63];
}

}  // namespace

#define DN_HOTA_SIZES(who)                                                                                             \
  DN_REQUIRE(n_images > 0 && n_images <= 65535, who ": %d images is out of range [1, 65535]", n_images);               \
  DN_REQUIRE(max_gt_ids >= 1 && max_gt_ids <= kMaxGtIds, who ": max_gt_ids = %d, must be in [1, %d]", max_gt_ids,      \
             kMaxGtIds);                                                                                               \
  DN_REQUIRE(max_track_ids >= 1 && max_track_ids <= kMaxTrackIds, who ": max_track_ids = %d, must be in [1, %d]",      \
             max_track_ids, kMaxTrackIds);                                                                             \
  DN_REQUIRE(max_frames >= 1 && max_frames <= kMaxFrames, who ": max_frames = %d, must be in [1, %d]", max_frames,     \
             kMaxFrames)

extern "C" size_t dn_hota_state_bytes(int n_images, int max_gt_ids, int max_track_ids, int max_frames) {
  if (!shapes_ok(n_images, max_gt_ids, max_track_ids, max_frames)) return 0;
  return (size_t)n_images * image_bytes(max_gt_ids, max_track_ids, max_frames);
}

extern "C" size_t dn_hota_work_bytes(int n_images, int max_gt_ids, int max_track_ids, int max_frames) {
  if (!shapes_ok(n_images, max_gt_ids, max_track_ids, max_frames)) return 0;
  return (size_t)n_images * work_image_bytes(max_gt_ids, max_track_ids, max_frames);
}

extern "C" int dn_hota_reset(void* state, int n_images, int max_gt_ids, int max_track_ids, int max_frames, void* stream) {
  DN_REQUIRE(state, "hota_reset: null state");
  DN_HOTA_SIZES("hota_reset");
  if (dn::zero_fill(state, dn_hota_state_bytes(n_images, max_gt_ids, max_track_ids, max_frames), (hipStream_t)stream) !=
      hipSuccess)
    return dn::fail(DN_ERR_LAUNCH, "hota_reset: the zero-fill launch failed");
  return DN_OK;
}

extern "C" int dn_hota_step(const double* rect, const int32_t* id, const int32_t* count, int n_images, int m,
                            const float* gt_boxes, const int32_t* gt_ids, const int32_t* gt_count, int g, double scale,
                            int max_gt_ids, int max_track_ids, int max_frames, void* state, double* out_potential,
                            void* stream) {
  DN_REQUIRE(rect, "hota_step: null rect");
  DN_REQUIRE(id, "hota_step: null id");
  DN_REQUIRE(count, "hota_step: null count");
  DN_REQUIRE(gt_boxes, "hota_step: null gt_boxes");
  DN_REQUIRE(gt_ids, "hota_step: null gt_ids");
  DN_REQUIRE(gt_count, "hota_step: null gt_count");
  DN_REQUIRE(state, "hota_step: null state");
  DN_REQUIRE(out_potential, "hota_step: null out_potential");
  DN_HOTA_SIZES("hota_step");
  DN_REQUIRE(m >= 1 && m <= kMaxM, "hota_step: M = %d track rows, must be in [1, %d]", m, kMaxM);
  DN_REQUIRE(g >= 1 && g <= kMaxG, "hota_step: G = %d ground-truth rows, must be in [1, %d]", g, kMaxG);
  DN_REQUIRE(std::isfinite(scale) && scale > 0, "hota_step: scale = %g, must be finite and > 0", scale);
  DN_REQUIRE((reinterpret_cast<size_t>(state) & 7) == 0, "hota_step: the state is not 8-byte aligned");
  Params p;
  p.m = m; p.g = g; p.ids = max_gt_ids; p.tids = max_track_ids; p.frames = max_frames;
  p.ld = m | 1;
  p.scale = scale;
  const int lds = (int)(sizeof(double) * (size_t)(g < kMaxV ? g : kMaxV) * p.ld);
  static dn::PerDeviceFlag flag;
  static int cache[64];
  const int fixed = static_lds_of(reinterpret_cast<const void*>(hota_step_kernel), flag, cache,
                                  (int)(sizeof(double) * (size_t)kMaxV * (kMaxM | 1)));
  if (fixed < 0) return dn::fail(DN_ERR_LAUNCH, "hota_step: cannot read or set the kernel's attributes");
  if (fixed + lds > kLdsPerCu)                     // never spill: a launch that does not fit is refused
    return dn::fail(DN_ERR_LAUNCH, "hota_step: %d B of work arrays + %d B of IoU matrix (G = %d, M = %d) do not fit %d B of LDS",
                    fixed, lds, g, m, kLdsPerCu);
  hipLaunchKernelGGL(hota_step_kernel, dim3(n_images), dim3(kThreads), lds, (hipStream_t)stream, rect, id, count, gt_boxes,
                     gt_ids, gt_count, p, static_cast<unsigned char*>(state), out_potential);
  return dn::check_launch("hota_step");
}

extern "C" int dn_hota_finish(const void* state, int n_images, int max_gt_ids, int max_track_ids, int max_frames,
                              void* work, int64_t* out_counts, int64_t* out_alpha_counts, double* out_alpha_sums,
                              int32_t* out_match, void* stream) {
  DN_REQUIRE(state, "hota_finish: null state");
  DN_REQUIRE(work, "hota_finish: null work");
  DN_REQUIRE(out_counts, "hota_finish: null out_counts");
  DN_REQUIRE(out_alpha_counts, "hota_finish: null out_alpha_counts");
  DN_REQUIRE(out_alpha_sums, "hota_finish: null out_alpha_sums");
  DN_HOTA_SIZES("hota_finish");
  DN_REQUIRE((reinterpret_cast<size_t>(state) & 7) == 0, "hota_finish: the state is not 8-byte aligned");
  DN_REQUIRE((reinterpret_cast<size_t>(work) & 7) == 0, "hota_finish: work is not 8-byte aligned");
  const int lds = (int)(sizeof(double) * (size_t)kMaxV * kMatchLd);
  static dn::PerDeviceFlag match_flag, fold_flag;
  static int match_cache[64], fold_cache[64];
  const int fixed = static_lds_of(reinterpret_cast<const void*>(hota_match_kernel), match_flag, match_cache, lds);
  const int fold = static_lds_of(reinterpret_cast<const void*>(hota_fold_kernel), fold_flag, fold_cache, 0);
  if (fixed < 0 || fold < 0) return dn::fail(DN_ERR_LAUNCH, "hota_finish: cannot read or set the kernels' attributes");
  if (fixed + lds > kLdsPerCu || fold > kLdsPerCu) // never spill: a launch that does not fit is refused
    return dn::fail(DN_ERR_LAUNCH, "hota_finish: %d B of work arrays + %d B of score matrix do not fit %d B of LDS", fixed,
                    lds, kLdsPerCu);
  hipStream_t s = (hipStream_t)stream;
  if (dn::zero_fill(work, dn_hota_work_bytes(n_images, max_gt_ids, max_track_ids, max_frames), s) != hipSuccess)
    return dn::fail(DN_ERR_LAUNCH, "hota_finish: the zero-fill launch failed");
  hipLaunchKernelGGL(hota_match_kernel, dim3(max_frames, n_images), dim3(kThreads), lds, s,
                     static_cast<const unsigned char*>(state), max_gt_ids, max_track_ids, max_frames,
                     static_cast<unsigned char*>(work), out_match);
  if (dn::check_launch("hota_match") != DN_OK) return DN_ERR_LAUNCH;
  hipLaunchKernelGGL(hota_fold_kernel, dim3(n_images), dim3(kThreads), 0, s, static_cast<const unsigned char*>(state),
                     max_gt_ids, max_track_ids, max_frames, static_cast<const unsigned char*>(work),
                     reinterpret_cast<long long*>(out_counts), reinterpret_cast<long long*>(out_alpha_counts),
                     out_alpha_sums);
  return dn::check_launch("hota_fold");
}
