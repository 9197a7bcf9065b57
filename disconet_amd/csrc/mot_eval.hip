// CLEAR MOT evaluation of the tracks behind the tracker: one evaluation step (TP / FP / FN / id switches / segments / the
// IoU sum of MOTP, per identity the frames present and matched) for every image of a call.  The contract is in
// include/disconet_hip.h; the host reference that defines the bits is tracking.HostClearMot.  All arithmetic is fp64 in a
// fixed order, + - * / and sqrt only, and every function carries `#pragma clang fp contract(off)`.
//
// One launch per step (mot_step_kernel), one workgroup of ONE wave per image, every phase a lane-strided loop; the
// single-wave form, the ground-truth phase, rect_iou, the assignment and the kept-slot lookup are track_eval_device.h's:
//   tracks     the reported tracks' rectangles and ids to LDS
//   measure    measure_ground_truth -> the rows used, then each identity's slot
//   score      lanes over (ground truth, track) pairs -> the matrix in LDS, [ground truths][ld], ld odd so that a column
//              walk is as free of bank conflicts as a row walk: 0 below the threshold, else the IoU, + 1000 for the pair the
//              identity held in the previous frame
//   assign     assign_rows on the matrix, rows the smaller side
//   state      lanes over identities, each record read and written by ONE lane: pst cleared and set, last, the frames
//              present / matched, the segments; the per-pair flags to LDS
//   count      one lane adds the frame's pairs to the header in ascending ground-truth row order (no atomics)
//   outputs    lanes over ground-truth rows; every word of the three outputs is written once
// The matrix lives in LDS: 8 * min(g, 128) * (m | 1) bytes of dynamic LDS, 132 KB at 128 x 128 beside 21 KB of work
// arrays (one workgroup per CU there).  Nothing is read back, nothing is allocated; two runs write the same bytes.
#include <cmath>

#include "dn_internal.h"
#include "track_eval_device.h"

namespace {

using namespace dn::trk;

constexpr int kHeaderBytes = 64;  // int64 frames, TP, FP, FN, IDSW; double motp_sum; int32 status; 12 spare bytes
constexpr int kRecBytes = 32;     // int32 last, pst, frames_present, frames_matched, segments, 3 spare
constexpr double kContinuity = 1000.0;

struct Params {
  int m, g, ids, ld;
  double thr, scale;
};

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
  __shared__ short slot_of_id[kMaxGtIds];
  __shared__ double hu[kMaxM + 1], hv[kMaxM + 1], hminv[kMaxM + 1];
  __shared__ int hp[kMaxM + 1], hway[kMaxM + 1], hused[kMaxM + 1];
  const int img = blockIdx.x, lane = threadIdx.x;
  const int m = p.m, g = p.g, ids = p.ids, ld = p.ld;
  unsigned char* st = state + (size_t)img * (kHeaderBytes + (size_t)kRecBytes * ids);
  int* recs = reinterpret_cast<int*>(st + kHeaderBytes);       // [ids][8]
  unsigned flags = 0;

  // ---- tracks: the reported rows
  const int K = clampi(tcount[img], m);
  for (int t = lane; t < K; t += kThreads) {
    const double* r = rect + 4 * ((size_t)img * m + t);
    const double r0 = r[0], r1 = r[1], r2 = r[2], r3 = r[3];
    trect[0][t] = r0; trect[1][t] = r1; trect[2][t] = r2; trect[3][t] = r3;
    tfin[t] = isfinite(r0) && isfinite(r1) && isfinite(r2) && isfinite(r3) ? 1 : 0;
    tident[t] = tid[(size_t)img * m + t];
  }
  for (int i = lane; i < ids; i += kThreads) slot_of_id[i] = -1;

  // ---- measure: the ground-truth rows used (its barriers stand between the -1 above and the slots below)
  const int V = measure_ground_truth(gt_boxes + 6 * (size_t)img * g, gt_ids + (size_t)img * g, clampi(gt_count[img], g), ids,
                                     p.scale, lane, grect, grow, gident, flags, [] {});

  // ---- score matrix
  for (int a = lane; a < V; a += kThreads) {
    slot_of_id[gident[a]] = (short)a;
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
    assign_rows(n, mm, lane, hu, hv, hminv, hp, hway, hused, [&](int row, int col) {
      return -(tp ? score_m[col * ld + row] : score_m[row * ld + col]);
    });
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
  const unsigned all = wave_or(flags);
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
    const int a = kept_slot(grow, V, r);
    const bool hit = a >= 0 && took[a] >= 0;
    const size_t o = (size_t)img * g + r;
    out_match[o] = hit ? tident[took[a]] : -1;
    out_iou[o] = hit ? aiou[a] : 0.0;
    out_flags[o] = hit ? aflags[a] : 0;
  }
}

bool shapes_ok(int n, int ids) { return n > 0 && n <= 65535 && ids >= 1 && ids <= kMaxGtIds; }

}  // namespace

extern "C" size_t dn_mot_state_bytes(int n_images, int max_gt_ids) {
  if (!shapes_ok(n_images, max_gt_ids)) return 0;
  return (size_t)n_images * (kHeaderBytes + (size_t)kRecBytes * max_gt_ids);
}

extern "C" int dn_mot_reset(void* state, int n_images, int max_gt_ids, void* stream) {
  DN_REQUIRE(state, "mot_reset: null state");
  DN_REQUIRE(n_images > 0 && n_images <= 65535, "mot_reset: %d images is out of range [1, 65535]", n_images);
  DN_REQUIRE(max_gt_ids >= 1 && max_gt_ids <= kMaxGtIds, "mot_reset: max_gt_ids = %d, must be in [1, %d]", max_gt_ids, kMaxGtIds);
  if (dn::zero_fill(state, dn_mot_state_bytes(n_images, max_gt_ids), (hipStream_t)stream) != hipSuccess)
    return dn::fail(DN_ERR_LAUNCH, "mot_reset: the zero-fill launch failed");
  return DN_OK;
}

extern "C" int dn_mot_step(const double* rect, const int32_t* id, const int32_t* count, int n_images, int m,
                           const float* gt_boxes, const int32_t* gt_ids, const int32_t* gt_count, int g, double scale,
                           double iou_threshold, int max_gt_ids, void* state, int32_t* out_match, double* out_iou,
                           int32_t* out_flags, void* stream) {
  DN_REQUIRE_EVAL_STEP("mot_step", kMaxM, kMaxG);
  DN_REQUIRE(out_match, "mot_step: null out_match");
  DN_REQUIRE(out_iou, "mot_step: null out_iou");
  DN_REQUIRE(out_flags, "mot_step: null out_flags");
  DN_REQUIRE(n_images > 0 && n_images <= 65535, "mot_step: %d images is out of range [1, 65535]", n_images);
  DN_REQUIRE(std::isfinite(iou_threshold) && iou_threshold > 0 && iou_threshold <= 1,
             "mot_step: iou_threshold = %g, must be in (0, 1]", iou_threshold);
  DN_REQUIRE(max_gt_ids >= 1 && max_gt_ids <= kMaxGtIds, "mot_step: max_gt_ids = %d, must be in [1, %d]", max_gt_ids, kMaxGtIds);
  Params p;
  p.m = m; p.g = g; p.ids = max_gt_ids;
  p.ld = m | 1;
  p.thr = iou_threshold; p.scale = scale;
  const int lds = (int)(sizeof(double) * (size_t)(g < kMaxV ? g : kMaxV) * p.ld);
  const int most = (int)(sizeof(double) * (size_t)kMaxV * (kMaxM | 1));
  static dn::PerDeviceFlag lds_flag;
  static int static_lds[64];
  const int fixed = dn::static_lds_of(reinterpret_cast<const void*>(mot_step_kernel), lds_flag, static_lds, most);
  if (fixed == -1) return dn::fail(DN_ERR_LAUNCH, "mot_step: cannot read the kernel's attributes");
  if (fixed < 0) return dn::fail(DN_ERR_LAUNCH, "mot_step: cannot reserve %d B of dynamic LDS", most);
  if (fixed + lds > kLdsPerCu)                     // never spill: a launch that does not fit is refused
    return dn::fail(DN_ERR_LAUNCH, "mot_step: %d B of work arrays + %d B of score matrix (G = %d, M = %d) do not fit %d B of LDS",
                    fixed, lds, g, m, kLdsPerCu);
  hipLaunchKernelGGL(mot_step_kernel, dim3(n_images), dim3(kThreads), lds, (hipStream_t)stream, rect, id, count, gt_boxes,
                     gt_ids, gt_count, p, static_cast<unsigned char*>(state), out_match, out_iou, out_flags);
  return dn::check_launch("mot_step");
}
