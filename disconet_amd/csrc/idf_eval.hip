// Identity metrics of the tracks (IDF1 / IDP / IDR beside the CLEAR figures of mot_eval.hip): per frame the count of
// every (ground-truth identity, track id) pair that overlaps at the threshold, kept on the device for the whole
// sequence; at the end ONE global assignment over that matrix.  The contract is in include/disconet_hip.h; the host
// reference that defines the bits is tracking.HostIdentity.  The IoU is fp64 in a fixed order, + - * / and sqrt only,
// and every function that touches fp64 carries `#pragma clang fp contract(off)`.
//
// idf_step_kernel: one launch per frame, one workgroup of ONE wave per image, as mot_step_kernel; the single-wave form,
// the ground-truth phase, rect_iou and the kept-slot lookup are track_eval_device.h's:
//   measure    measure_ground_truth -> the rows used; ahead of its first barrier
//   tracks     lanes over reported rows: the id's range (status bit 16), the column t - 1, track_count bumped with an
//              integer atomicAdd (the same id may come on two rows of a frame), the rectangle to LDS
//   pairs      lanes over (ground truth, track) pairs: not iou < threshold -> atomicAdd on the matrix word in global
//              memory and on the row's overlap count in LDS.  Integer adds: the result does not depend on the order
//   counts     gt_count by the lane that owns the row (ids are unique after dedupe); one lane adds to the header
//   outputs    lanes over ground-truth rows; every word of `overlaps` is written once
// 10 KB of LDS.
//
// idf_finish_kernel: one workgroup per image, reads the state only.  The ids present (gt_count > 0, track_count > 0)
// are compacted into LDS lists in ascending order (compact_present); then tracking.hungarian_max to the letter --
// assign_rows of track_eval_device.h with int16 / int8 work arrays, in fp64 (all values are integers below 2^31, every
// sum is exact), rows the smaller side.  The weights are NOT copied: each step reads one word per lane from
// the state (1 MB per image at the default sizes: L2-resident); with more identities than track ids a row walk strides
// the matrix by max_track_ids words.  Work arrays in LDS, sized for 2049 columns and 1025 rows:
//   u 8 x 1025, v and minv 8 x 2049 each, p and way 2 x 2049 each (int16: a row <= 1024, a column <= 2048), used 2049,
//   the id lists 2 x 1024 + 2 x 2048, the match row 2 x 1024: 59 488 B (58.1 KB), static, whatever the launch's sizes are.
// The launcher reads the figure from the compiled kernel and refuses a launch beyond 160 KB.
// ONE wave per image, as the siblings: a step is one word per lane and a wave arg-min, and between steps stand four
// barriers, which a single wave passes without waiting.  Real sequences have tens of identities and a few hundred
// track ids, i.e. a handful of column strides per step; 256 lanes would shorten that stride loop but pay a cross-wave
// arg-min through LDS and four real barriers on every step, which is the larger part at those sizes.  The search is
// bounded by rows x (columns + 1) steps whatever the numbers are; its worst case (1024 x 2048) is slow and accepted for
// a once-per-sequence call.  Nothing is read back, nothing is allocated; two runs write the same bytes.
#include <cmath>

#include "dn_internal.h"
#include "track_eval_device.h"

namespace {

using namespace dn::trk;

constexpr int kHeaderBytes = 64;    // int64 frames, gt_dets, dets; int32 status; 36 spare bytes

struct Params {
  int m, g, ids, tids;
  double thr, scale;
};

__host__ __device__ inline size_t image_bytes(int ids, int tids) {
  return (size_t)kHeaderBytes + 4 * ((size_t)ids + (size_t)tids + (size_t)ids * (size_t)tids);
}

// The header's int64 words as two int32 halves: an image's state is a multiple of 4 bytes, not of 8.
__device__ __forceinline__ long long load64(const int* w) {
  return (long long)(((unsigned long long)(unsigned)w[1] << 32) | (unsigned long long)(unsigned)w[0]);
}
__device__ __forceinline__ void store64(int* w, long long v) {
  w[0] = (int)(unsigned)((unsigned long long)v & 0xffffffffull);
  w[1] = (int)(unsigned)((unsigned long long)v >> 32);
}

__global__ void __launch_bounds__(kThreads) idf_step_kernel(const double* __restrict__ rect, const int* __restrict__ tid,
                                                            const int* __restrict__ tcount,
                                                            const float* __restrict__ gt_boxes,
                                                            const int* __restrict__ gt_ids,
                                                            const int* __restrict__ gt_count, Params p,
                                                            unsigned char* __restrict__ state,
                                                            int* __restrict__ out_overlaps) {
#pragma clang fp contract(off)
  __shared__ double grect[4][kMaxV], trect[4][kMaxM];
  __shared__ int grow[kMaxV], gident[kMaxV], hits[kMaxV];
  __shared__ int tcol[kMaxM];                      // the column of a reported row that can overlap, else -1
  const int img = blockIdx.x, lane = threadIdx.x;
  const int m = p.m, g = p.g, ids = p.ids, tids = p.tids;
  unsigned char* st = state + (size_t)img * image_bytes(ids, tids);
  int* hdr = reinterpret_cast<int*>(st);
  int* gcnt = reinterpret_cast<int*>(st + kHeaderBytes);       // [ids]
  int* tcnt = gcnt + ids;                                      // [tids]
  int* pairs = tcnt + tids;                                    // [ids][tids]
  unsigned flags = 0;

  // ---- measure: the ground-truth rows used; behind its measure loop, ahead of its first barrier
  // ---- tracks: the reported rows, their columns and their counts
  const int K = clampi(tcount[img], m);
  int dets = 0;
  const int V = measure_ground_truth(gt_boxes + 6 * (size_t)img * g, gt_ids + (size_t)img * g, clampi(gt_count[img], g), ids,
                                     p.scale, lane, grect, grow, gident, flags, [&] {
    for (int base = 0; base < K; base += kThreads) {
      const int t = base + lane;
      bool counted = false;
      if (t < K) {
        const double* r = rect + 4 * ((size_t)img * m + t);
        const double r0 = r[0], r1 = r[1], r2 = r[2], r3 = r[3];
        trect[0][t] = r0; trect[1][t] = r1; trect[2][t] = r2; trect[3][t] = r3;
        const int track = tid[(size_t)img * m + t];
        counted = track >= 1 && track <= tids;
        if (counted) atomicAdd(&tcnt[track - 1], 1);
        else flags |= 16u;
        tcol[t] = counted && isfinite(r0) && isfinite(r1) && isfinite(r2) && isfinite(r3) ? track - 1 : -1;
      }
      dets += __popcll(__ballot(counted));
    }
    for (int a = lane; a < kMaxV; a += kThreads) hits[a] = 0;
  });

  // ---- pairs: lanes over (ground truth, track); integer atomics, order-free
  for (int e = lane; e < V * K; e += kThreads) {
    const int a = e / K, t = e - a * K;
    const int col = tcol[t];
    if (col < 0) continue;
    const double iou = rect_iou(grect[0][a], grect[1][a], grect[2][a], grect[3][a], trect[0][t], trect[1][t], trect[2][t],
                                trect[3][t]);
    if (iou < p.thr) continue;
    atomicAdd(&pairs[(size_t)gident[a] * tids + col], 1);
    atomicAdd(&hits[a], 1);
  }
  // ---- counts: an identity's word belongs to the lane that owns its row; one lane adds to the header
  for (int a = lane; a < V; a += kThreads) gcnt[gident[a]] = gcnt[gident[a]] + 1;
  const unsigned all = wave_or(flags);
  if (lane == 0) {
    store64(hdr + 0, load64(hdr + 0) + 1);
    store64(hdr + 2, load64(hdr + 2) + V);
    store64(hdr + 4, load64(hdr + 4) + dets);
    hdr[6] = hdr[6] | (int)all;
  }
  __syncthreads();

  // ---- outputs: every row once; a kept row is found in the ascending list of the rows kept
  for (int r = lane; r < g; r += kThreads) {
    const int a = kept_slot(grow, V, r);
    out_overlaps[(size_t)img * g + r] = a >= 0 ? hits[a] : 0;
  }
}

__global__ void __launch_bounds__(kThreads) idf_finish_kernel(const unsigned char* __restrict__ state, int ids, int tids,
                                                              long long* __restrict__ out_counts,
                                                              int* __restrict__ out_match) {
#pragma clang fp contract(off)
  __shared__ double hu[kMaxGtIds + 1], hv[kMaxTrackIds + 1], hminv[kMaxTrackIds + 1];
  __shared__ short hp[kMaxTrackIds + 1], hway[kMaxTrackIds + 1];
  __shared__ unsigned char hused[kMaxTrackIds + 1];
  __shared__ unsigned short rowid[kMaxGtIds], colid[kMaxTrackIds];
  __shared__ short mout[kMaxGtIds];
  const int img = blockIdx.x, lane = threadIdx.x;
  const unsigned char* st = state + (size_t)img * image_bytes(ids, tids);
  const int* hdr = reinterpret_cast<const int*>(st);
  const int* gcnt = reinterpret_cast<const int*>(st + kHeaderBytes);
  const int* tcnt = gcnt + ids;
  const int* pairs = tcnt + tids;

  // ---- the ids present, ascending
  const int R = compact_present(gcnt, ids, lane, rowid), C = compact_present(tcnt, tids, lane, colid);
  for (int i = lane; i < ids; i += kThreads) mout[i] = 0;
  __syncthreads();

  // ---- assign: tracking.hungarian_max(pairs[rows][cols] as fp64), rows the smaller side
  long long idtp = 0;
  if (R > 0 && C > 0) {   // wave-uniform
    const bool tp = R > C;                         // rows are the track ids when there are more identities
    const int n = tp ? C : R, mm = tp ? R : C;
    // a row's words: contiguous ids along the matrix row, or one column of it at a stride of tids words
    assign_rows(n, mm, lane, hu, hv, hminv, hp, hway, hused, [&](int row, int col) {
      const int w = tp ? pairs[(size_t)rowid[col] * tids + colid[row]] : pairs[(size_t)rowid[row] * tids + colid[col]];
      return -(double)w;
    });
    // a pair is kept only when its weight is > 0
    for (int j = 1 + lane; j <= mm; j += kThreads) {
      const int i = clampi(hp[j], n);
      if (i > 0) {
        const int a = rowid[tp ? j - 1 : i - 1], t = colid[tp ? i - 1 : j - 1];
        const int w = pairs[(size_t)a * tids + t];
        if (w > 0) {
          mout[a] = (short)(t + 1);
          idtp += w;
        }
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) idtp += __shfl_xor(idtp, o);
    __syncthreads();
  }

  // ---- outputs: every word once
  for (int i = lane; i < ids; i += kThreads) out_match[(size_t)img * ids + i] = mout[i];
  if (lane == 0) {
    long long* o = out_counts + 8 * (size_t)img;
    o[0] = load64(hdr + 0);
    o[1] = load64(hdr + 2);
    o[2] = load64(hdr + 4);
    o[3] = idtp;
    o[4] = R;
    o[5] = C;
    o[6] = hdr[6];
    o[7] = 0;
  }
}

bool shapes_ok(int n, int ids, int tids) {
  return n > 0 && n <= 65535 && ids >= 1 && ids <= kMaxGtIds && tids >= 1 && tids <= kMaxTrackIds;
}

}  // namespace

#define DN_IDF_SIZES(who)                                                                                              \
  DN_REQUIRE(n_images > 0 && n_images <= 65535, who ": %d images is out of range [1, 65535]", n_images);               \
  DN_REQUIRE(max_gt_ids >= 1 && max_gt_ids <= kMaxGtIds, who ": max_gt_ids = %d, must be in [1, %d]", max_gt_ids,      \
             kMaxGtIds);                                                                                               \
  DN_REQUIRE(max_track_ids >= 1 && max_track_ids <= kMaxTrackIds, who ": max_track_ids = %d, must be in [1, %d]",      \
             max_track_ids, kMaxTrackIds)

extern "C" size_t dn_idf_state_bytes(int n_images, int max_gt_ids, int max_track_ids) {
  if (!shapes_ok(n_images, max_gt_ids, max_track_ids)) return 0;
  return (size_t)n_images * image_bytes(max_gt_ids, max_track_ids);
}

extern "C" int dn_idf_reset(void* state, int n_images, int max_gt_ids, int max_track_ids, void* stream) {
  DN_REQUIRE(state, "idf_reset: null state");
  DN_IDF_SIZES("idf_reset");
  if (dn::zero_fill(state, dn_idf_state_bytes(n_images, max_gt_ids, max_track_ids), (hipStream_t)stream) != hipSuccess)
    return dn::fail(DN_ERR_LAUNCH, "idf_reset: the zero-fill launch failed");
  return DN_OK;
}

extern "C" int dn_idf_step(const double* rect, const int32_t* id, const int32_t* count, int n_images, int m,
                           const float* gt_boxes, const int32_t* gt_ids, const int32_t* gt_count, int g, double scale,
                           double iou_threshold, int max_gt_ids, int max_track_ids, void* state, int32_t* out_overlaps,
                           void* stream) {
  DN_REQUIRE_EVAL_STEP("idf_step", kMaxM, kMaxG);
  DN_REQUIRE(out_overlaps, "idf_step: null out_overlaps");
  DN_IDF_SIZES("idf_step");
  DN_REQUIRE(std::isfinite(iou_threshold) && iou_threshold > 0 && iou_threshold <= 1,
             "idf_step: iou_threshold = %g, must be in (0, 1]", iou_threshold);
  Params p;
  p.m = m; p.g = g; p.ids = max_gt_ids; p.tids = max_track_ids;
  p.thr = iou_threshold; p.scale = scale;
  hipLaunchKernelGGL(idf_step_kernel, dim3(n_images), dim3(kThreads), 0, (hipStream_t)stream, rect, id, count, gt_boxes,
                     gt_ids, gt_count, p, static_cast<unsigned char*>(state), out_overlaps);
  return dn::check_launch("idf_step");
}

extern "C" int dn_idf_finish(const void* state, int n_images, int max_gt_ids, int max_track_ids, int64_t* out_counts,
                             int32_t* out_match, void* stream) {
  DN_REQUIRE(state, "idf_finish: null state");
  DN_REQUIRE(out_counts, "idf_finish: null out_counts");
  DN_REQUIRE(out_match, "idf_finish: null out_match");
  DN_IDF_SIZES("idf_finish");
  static dn::PerDeviceFlag lds_flag;
  static int static_lds[64];
  const int fixed = dn::static_lds_of(reinterpret_cast<const void*>(idf_finish_kernel), lds_flag, static_lds, 0);
  if (fixed < 0) return dn::fail(DN_ERR_LAUNCH, "idf_finish: cannot read the kernel's attributes");
  if (fixed > kLdsPerCu)                           // never spill: a launch that does not fit is refused
    return dn::fail(DN_ERR_LAUNCH, "idf_finish: %d B of work arrays do not fit %d B of LDS", fixed, kLdsPerCu);
  hipLaunchKernelGGL(idf_finish_kernel, dim3(n_images), dim3(kThreads), 0, (hipStream_t)stream,
                     static_cast<const unsigned char*>(state), max_gt_ids, max_track_ids,
                     reinterpret_cast<long long*>(out_counts), out_match);
  return dn::check_launch("idf_finish");
}
