// HOTA of the tracks (beside the CLEAR figures of mot_eval.hip and the identity figures of idf_eval.hip): the frame
// matching is weighted by a global alignment score that is known only after the last frame, so the sequence is seen
// twice.  Per frame the step adds to the potential-match matrix and LOGS the frame's rectangles in the device state; at
// the end the finish matches every logged frame, all frames of all images at once.  The contract is in
// include/disconet_hip.h; the host reference that defines the bits is tracking.HostHota.  All arithmetic is fp64 in a fixed
// order, + - * / and sqrt only, and every function that touches fp64 carries `#pragma clang fp contract(off)`.
//
// hota_step_kernel: one launch per frame, one workgroup of ONE wave per image, as mot_step_kernel and idf_step_kernel; the
// single-wave form, the ground-truth phase, rect_iou, the assignment, the kept-slot lookup and the compaction of the ids
// present are track_eval_device.h's:
//   tracks     lanes over reported rows: the id's range (status bit 16), an id a lower row carries (bit 64), ballot prefix
//              -> the columns in LDS, in row order
//   measure    measure_ground_truth -> the rows used
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
// in LDS, [V][C | 1]; assign_rows on it (lanes over columns); per kept pair
// the IoU once more and K, the number of alphas it counts at; one integer atomic per kept pair into the cell's 20-bin
// histogram in `work`; lane k < 19 walks the rows in ascending order for the frame's TP_k (one integer atomic per alpha
// into `work`) and its loc partial (written to the frame's own words of `work`, never added atomically).
// V and C come from the log, so the launch reserves the largest matrix whatever the arguments are: 8 * 128 * 129 B of
// dynamic LDS beside 17 KB of work arrays, one workgroup per CU.
//
// hota_fold_kernel: one workgroup of one wave per image.  The track ids present are compacted into LDS (compact_present);
// the identities present are taken 64 at a time in ascending order, one per lane: the lane walks the present track ids in
// ascending order, turns a cell's bins into the 19 matched counts (suffix sums) and adds the cell's three terms per alpha
// to its row sums; the row sums go to LDS and lanes 0..56 (one per alpha and sum) add the chunk's rows to their running
// totals in ascending identity order.  Lane k < 19 adds the frames' loc partials in slot order and writes the alpha's
// words.  Nothing is read back, nothing is allocated; two runs write the same bytes.
#include <cmath>

#include "dn_internal.h"
#include "track_eval_device.h"

namespace {

using namespace dn::trk;

constexpr int kMaxFrames = 4096;    // log slots per image
constexpr int kHeaderBytes = 64;    // int64 frames, logged, gt_dets, dets; int32 status; 28 spare bytes
constexpr int kSlotBytes = 16 + 4 * (kMaxV + kMaxM) + 32 * (kMaxV + kMaxM);   // 9232
constexpr int kAlphas = 19;
constexpr int kBins = 20;           // K = 0 .. 19 of a kept pair
constexpr int kMatchLd = kMaxM | 1;
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

  // ---- measure: the ground-truth rows used (its barriers stand between the columns above and the pairs)
  const int V = measure_ground_truth(gt_boxes + 6 * (size_t)img * g, gt_ids + (size_t)img * g, clampi(gt_count[img], g), ids,
                                     p.scale, lane, grect, grow, gident, flags, [] {});

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
  const unsigned all = wave_or(flags);
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
    const int a = kept_slot(grow, V, r);
    out_potential[(size_t)img * g + r] = a >= 0 ? prow[a] : 0.0;
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
    assign_rows(n, mm, lane, hu, hv, hminv, hp, hway, hused, [&](int row, int col) {
      return -(tp_ ? score_m[col * ld + row] : score_m[row * ld + col]);
    });
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
  const int C = compact_present(tcnt, tids, lane, colid);
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
  DN_REQUIRE_EVAL_STEP("hota_step", kMaxM, kMaxG);
  DN_REQUIRE(out_potential, "hota_step: null out_potential");
  DN_HOTA_SIZES("hota_step");
  DN_REQUIRE((reinterpret_cast<size_t>(state) & 7) == 0, "hota_step: the state is not 8-byte aligned");
  Params p;
  p.m = m; p.g = g; p.ids = max_gt_ids; p.tids = max_track_ids; p.frames = max_frames;
  p.ld = m | 1;
  p.scale = scale;
  const int lds = (int)(sizeof(double) * (size_t)(g < kMaxV ? g : kMaxV) * p.ld);
  static dn::PerDeviceFlag flag;
  static int cache[64];
  const int fixed = dn::static_lds_of(reinterpret_cast<const void*>(hota_step_kernel), flag, cache,
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
  const int fixed = dn::static_lds_of(reinterpret_cast<const void*>(hota_match_kernel), match_flag, match_cache, lds);
  const int fold = dn::static_lds_of(reinterpret_cast<const void*>(hota_fold_kernel), fold_flag, fold_cache, 0);
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
