// CLEAR MOT evaluation of the tracks behind the tracker: one evaluation step (TP / FP / FN / id switches / segments / the
// IoU sum of MOTP, per identity the frames present and matched) for every image of a call.  The contract is in
// include/disconet_hip.h; the host reference that defines the bits is tracking.HostClearMot.  All arithmetic is fp64 in a
// fixed order, + - * / and sqrt only, and every function carries `#pragma clang fp contract(off)`.
//
// One launch per step (mot_step_kernel), one workgroup of ONE wave per image -- 64 lanes, every phase a lane-strided
// loop, so the phases hand over through LDS with single-wave barriers and every reduction is a wave shuffle:
//   measure    lanes over ground-truth rows, 64 at a time in row order: rectangle of the scaled corners, validity, the id's
//              range, ballot prefix -> the first 128 valid rows in LDS; the reported tracks' rectangles and ids to LDS
//   dedupe     lanes over the kept rows: a row whose id a lower kept row carries leaves (stable compaction)
//   score      lanes over (ground truth, track) pairs -> the matrix in LDS, [ground truths][ld], ld odd so that a column
//              walk is as free of bank conflicts as a row walk: 0 below the threshold, else the IoU, + 1000 for the pair the
//              identity held in the previous frame
//   assign     the shortest-augmenting-path Hungarian step of track.hip (its own copy), lanes over columns: each step one
//              LDS read per lane and one wave arg-min (lowest index among equals); bounded whatever the numbers are
//   state      lanes over identities, each record read and written by ONE lane: pst cleared and set, last, the frames
//              present / matched, the segments; the per-pair flags to LDS
//   count      one lane adds the frame's pairs to the header in ascending ground-truth row order (no atomics)
//   outputs    lanes over ground-truth rows; every word of the three outputs is written once
// The matrix lives in LDS: 8 * min(g, 128) * (m | 1) bytes of dynamic LDS, 132 KB at 128 x 128 beside 21 KB of work
// arrays (one workgroup per CU there).  Nothing is read back, nothing is allocated; two runs write the same bytes.
#include <climits>
#include <cmath>

#include "dn_internal.h"

namespace {

constexpr int kThreads = 64;
constexpr int kMaxM = 128;        // reported track rows per image
constexpr int kMaxV = 128;        // valid ground-truth rows used per image
constexpr int kMaxG = 1024;       // ground-truth rows per image
constexpr int kMaxIds = 1024;     // identities per image
constexpr int kHeaderBytes = 64;  // int64 frames, TP, FP, FN, IDSW; double motp_sum; int32 status; 12 spare bytes
constexpr int kRecBytes = 32;     // int32 last, pst, frames_present, frames_matched, segments, 3 spare
constexpr int kLdsPerCu = 160 * 1024;
constexpr double kContinuity = 1000.0;

struct Params {
  int m, g, ids, ld;
  double thr, scale;
};

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

__global__ void __launch_bounds__(kThreads) mot_step_kernel(const double* __restrict__ rect, const int* __restrict__ tid,
                                                            const int* __restrict__ tcount,
                                                            const float* __restrict__ gt_boxes,
                                                            const int* __restrict__ gt_ids,
                                                            const int* __restrict__ gt_count, Params p,
                                                            unsigned char* __restrict__ state, int* __restrict__ out_match,
                                                            double* __restrict__ out_iou, int* __restrict__ out_flags) {
#pragma clang fp contract(off)
  extern __shared__ double score_m[];              // [ground truths][p.ld]
  __shared__ double grect[4][kMaxV], trect[4][kMaxM], aiou[kMaxV];
  __shared__ int grow[kMaxV], gident[kMaxV], gpst[kMaxV], took[kMaxV], aflags[kMaxV];
  __shared__ int tident[kMaxM], tfin[kMaxM];
  __shared__ short slot_of_id[kMaxIds];
  __shared__ double hu[kMaxM + 1], hv[kMaxM + 1], hminv[kMaxM + 1];
  __shared__ int hp[kMaxM + 1], hway[kMaxM + 1], hused[kMaxM + 1];
  const int img = blockIdx.x, lane = threadIdx.x;
  const int m = p.m, g = p.g, ids = p.ids, ld = p.ld;
  unsigned char* st = state + (size_t)img * (kHeaderBytes + (size_t)kRecBytes * ids);
  int* recs = reinterpret_cast<int*>(st + kHeaderBytes);       // [ids][8]
  unsigned flags = 0;

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
  // the reported tracks
  const int K = clampi(tcount[img], m);
  for (int t = lane; t < K; t += kThreads) {
    const double* r = rect + 4 * ((size_t)img * m + t);
    const double r0 = r[0], r1 = r[1], r2 = r[2], r3 = r[3];
    trect[0][t] = r0; trect[1][t] = r1; trect[2][t] = r2; trect[3][t] = r3;
    tfin[t] = isfinite(r0) && isfinite(r1) && isfinite(r2) && isfinite(r3) ? 1 : 0;
    tident[t] = tid[(size_t)img * m + t];
  }
  for (int i = lane; i < ids; i += kThreads) slot_of_id[i] = -1;
  __syncthreads();

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
      slot_of_id[kid[h]] = (short)dst;
    }
    V += __popcll(mask);
  }
  __syncthreads();

  // ---- score matrix
  for (int a = lane; a < V; a += kThreads) {
    gpst[a] = recs[8 * gident[a] + 1];
    took[a] = -1;
  }
  __syncthreads();
  for (int e = lane; e < V * K; e += kThreads) {
    const int a = e / K, t = e - a * K;
    const double iou = tfin[t] ? rect_iou(grect[0][a], grect[1][a], grect[2][a], grect[3][a], trect[0][t], trect[1][t],
                                          trect[2][t], trect[3][t])
                               : 0.0;
    score_m[a * ld + t] = iou < p.thr ? 0.0 : (tident[t] == gpst[a] ? iou + kContinuity : iou);
  }
  __syncthreads();

  // ---- assign: tracking.hungarian_max(score), rows the smaller side
  if (V > 0 && K > 0) {   // wave-uniform
    const bool tp = V > K;                         // rows are the tracks when there are more ground truths
    const int n = tp ? K : V, mm = tp ? V : K;
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
          const double cost = -(tp ? score_m[(j - 1) * ld + (i0 - 1)] : score_m[(i0 - 1) * ld + (j - 1)]);
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
    for (int j = 1 + lane; j <= mm; j += kThreads) {
      const int i = clampi(hp[j], n);
      if (i > 0) took[tp ? j - 1 : i - 1] = tp ? i - 1 : j - 1;
    }
    __syncthreads();
  }
  // a pair is kept when its score is > 0; its IoU is taken again from the rectangles
  for (int a = lane; a < V; a += kThreads) {
    const int t = took[a];
    double iou = 0.0;
    if (t >= 0) {
      if (score_m[a * ld + t] > 0)
        iou = rect_iou(grect[0][a], grect[1][a], grect[2][a], grect[3][a], trect[0][t], trect[1][t], trect[2][t],
                       trect[3][t]);
      else
        took[a] = -1;
    }
    aiou[a] = iou;
    aflags[a] = 0;
  }
  __syncthreads();

  // ---- state: every identity's record belongs to one lane
  for (int i = lane; i < ids; i += kThreads) {
    int* rec = recs + 8 * i;
    const int a = slot_of_id[i];
    if (a < 0) {
      if (rec[1] != 0) rec[1] = 0;
      continue;
    }
    const int t = took[a];
    rec[2] = rec[2] + 1;
    if (t < 0) {
      rec[1] = 0;
      continue;
    }
    const int track = tident[t], last = rec[0];
    int f = 1;
    if (last != 0 && last != track) f |= 2;
    if (gpst[a] == 0) {
      f |= 4;
      rec[4] = rec[4] + 1;
    }
    rec[0] = track;
    rec[1] = track;
    rec[3] = rec[3] + 1;
    aflags[a] = f;
  }
  __syncthreads();

  // ---- count: one lane, ascending ground-truth row order
  const unsigned all = (__any(flags & 1u) ? 1u : 0u) | (__any(flags & 2u) ? 2u : 0u) | (__any(flags & 4u) ? 4u : 0u) |
                       (__any(flags & 8u) ? 8u : 0u);
  if (lane == 0) {
    long long* hdr = reinterpret_cast<long long*>(st);
    double motp = reinterpret_cast<double*>(st)[5];
    int matched = 0, idsw = 0;
    for (int a = 0; a < V; ++a)
      if (took[a] >= 0) {
        motp = motp + aiou[a];
        ++matched;
        idsw += (aflags[a] >> 1) & 1;
      }
    hdr[0] = hdr[0] + 1;
    hdr[1] = hdr[1] + matched;
    hdr[2] = hdr[2] + (K - matched);
    hdr[3] = hdr[3] + (V - matched);
    hdr[4] = hdr[4] + idsw;
    reinterpret_cast<double*>(st)[5] = motp;
    int* status = reinterpret_cast<int*>(st) + 12;
    *status = *status | (int)all;
  }

  // ---- outputs: every row once; a used row is found in the ascending list of the rows kept
  for (int r = lane; r < g; r += kThreads) {
    int lo = 0, hi = V;                            // first slot with grow >= r
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (grow[mid] < r) lo = mid + 1;
      else hi = mid;
    }
    const bool hit = lo < V && grow[lo] == r && took[lo] >= 0;
    const size_t o = (size_t)img * g + r;
    out_match[o] = hit ? tident[took[lo]] : -1;
    out_iou[o] = hit ? aiou[lo] : 0.0;
    out_flags[o] = hit ? aflags[lo] : 0;
  }
}

bool shapes_ok(int n, int ids) { return n > 0 && n <= 65535 && ids >= 1 && ids <= kMaxIds; }

}  // namespace

extern "C" size_t dn_mot_state_bytes(int n_images, int max_gt_ids) {
  if (!shapes_ok(n_images, max_gt_ids)) return 0;
  return (size_t)n_images * (kHeaderBytes + (size_t)kRecBytes * max_gt_ids);
}

extern "C" int dn_mot_reset(void* state, int n_images, int max_gt_ids, void* stream) {
  DN_REQUIRE(state, "mot_reset: null state");
  DN_REQUIRE(n_images > 0 && n_images <= 65535, "mot_reset: %d images is out of range [1, 65535]", n_images);
  DN_REQUIRE(max_gt_ids >= 1 && max_gt_ids <= kMaxIds, "mot_reset: max_gt_ids = %d, must be in [1, %d]", max_gt_ids, kMaxIds);
  if (dn::zero_fill(state, dn_mot_state_bytes(n_images, max_gt_ids), (hipStream_t)stream) != hipSuccess)
    return dn::fail(DN_ERR_LAUNCH, "mot_reset: the zero-fill launch failed");
  return DN_OK;
}

extern "C" int dn_mot_step(const double* rect, const int32_t* id, const int32_t* count, int n_images, int m,
                           const float* gt_boxes, const int32_t* gt_ids, const int32_t* gt_count, int g, double scale,
                           double iou_threshold, int max_gt_ids, void* state, int32_t* out_match, double* out_iou,
                           int32_t* out_flags, void* stream) {
  DN_REQUIRE(rect, "mot_step: null rect");
  DN_REQUIRE(id, "mot_step: null id");
  DN_REQUIRE(count, "mot_step: null count");
  DN_REQUIRE(gt_boxes, "mot_step: null gt_boxes");
  DN_REQUIRE(gt_ids, "mot_step: null gt_ids");
  DN_REQUIRE(gt_count, "mot_step: null gt_count");
  DN_REQUIRE(state, "mot_step: null state");
  DN_REQUIRE(out_match, "mot_step: null out_match");
  DN_REQUIRE(out_iou, "mot_step: null out_iou");
  DN_REQUIRE(out_flags, "mot_step: null out_flags");
  DN_REQUIRE(n_images > 0 && n_images <= 65535, "mot_step: %d images is out of range [1, 65535]", n_images);
  DN_REQUIRE(m >= 1 && m <= kMaxM, "mot_step: M = %d track rows, must be in [1, %d]", m, kMaxM);
  DN_REQUIRE(g >= 1 && g <= kMaxG, "mot_step: G = %d ground-truth rows, must be in [1, %d]", g, kMaxG);
  DN_REQUIRE(std::isfinite(scale) && scale > 0, "mot_step: scale = %g, must be finite and > 0", scale);
  DN_REQUIRE(std::isfinite(iou_threshold) && iou_threshold > 0 && iou_threshold <= 1,
             "mot_step: iou_threshold = %g, must be in (0, 1]", iou_threshold);
  DN_REQUIRE(max_gt_ids >= 1 && max_gt_ids <= kMaxIds, "mot_step: max_gt_ids = %d, must be in [1, %d]", max_gt_ids, kMaxIds);
  Params p;
  p.m = m; p.g = g; p.ids = max_gt_ids;
  p.ld = m | 1;
  p.thr = iou_threshold; p.scale = scale;
  const int lds = (int)(sizeof(double) * (size_t)(g < kMaxV ? g : kMaxV) * p.ld);
  static dn::PerDeviceFlag lds_flag;
  static int static_lds[64];
  int dev = 0;
  (void)hipGetDevice(&dev);
  bool& lds_ready = lds_flag.here();
  if (!lds_ready) {
    hipFuncAttributes attr;
    if (hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(mot_step_kernel)) != hipSuccess)
      return dn::fail(DN_ERR_LAUNCH, "mot_step: cannot read the kernel's attributes");
    const int most = (int)(sizeof(double) * (size_t)kMaxV * (kMaxM | 1));
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(mot_step_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                            most) != hipSuccess)
      return dn::fail(DN_ERR_LAUNCH, "mot_step: cannot reserve %d B of dynamic LDS", most);
    static_lds[dev & 63] = (int)attr.sharedSizeBytes;
    lds_ready = true;
  }
  if (static_lds[dev & 63] + lds > kLdsPerCu)      // never spill: a launch that does not fit is refused
    return dn::fail(DN_ERR_LAUNCH, "mot_step: %d B of work arrays + %d B of score matrix (G = %d, M = %d) do not fit %d B of LDS",
                    static_lds[dev & 63], lds, g, m, kLdsPerCu);
  hipLaunchKernelGGL(mot_step_kernel, dim3(n_images), dim3(kThreads), lds, (hipStream_t)stream, rect, id, count, gt_boxes,
                     gt_ids, gt_count, p, static_cast<unsigned char*>(state), out_match, out_iou, out_flags);
  return dn::check_launch("mot_step");
}
