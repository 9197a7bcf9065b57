// Detection mAP, the per-frame part on the GPU: every detection of every image is ranked by score, matched to its best
// ground-truth box (rotated IoU in fp64, rot_iou_device.h), marked true / false positive at up to 8 IoU thresholds
// (mmdetection's tpfp_default: the first claimant of a ground-truth box in score order wins) and, optionally, appended as a
// record to caller-owned arrays at a device-resident cursor.  The host reference is postprocess.host_match_ground_truth.
//
// Launch sequence (fixed: it depends on the shapes only, never on the data; nothing is read back, nothing is allocated):
//   ap_rank      one workgroup per image: rank of every row in the stable descending score order, the number of valid
//                rows (row < count and a finite score), the non-finite status bit, the claim words set to INT_MAX
//   ap_iou       tile (64 rows, 16-column ground-truth piece) per wave: circumscribed-circle test, then the fp64 polygon
//                clip per lane; the piece's best (IoU, lowest column) per row
//   ap_claim     per row: the pieces folded in column order (strict >, so the lowest column that attains the maximum wins);
//                per threshold an integer atomicMin of the row's rank into the claim word of its ground-truth box
//   ap_tp        per row and threshold: true positive when the row's rank is the claim word; the record at
//                cursor + (valid rows of the images before) + rank
//   ap_advance   one thread: cursor += valid rows, the overflow status bit, the per-agent ground-truth counters
// Only integer atomics are used and every order is decided by (score, row index): two runs write the same bytes.
#include <climits>
#include <cmath>

#include "dn_internal.h"
#include "rot_iou_device.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxK = 1024;    // detection rows per image (dn_detect's limit for top_k)
constexpr int kMaxG = 1024;    // ground-truth rows per image
constexpr int kMaxT = 8;       // thresholds: one bit each in a record's flag byte
constexpr int kCols = 16;      // ground-truth columns per tile
constexpr int kMaxAgents = 65536;

struct Thresholds {
  double t[kMaxT];
};

struct Layout {
  size_t nvalid, claim, piou, pgt, total;
};

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

Layout layout(int n, int k, int g, int nt) {
  const size_t pieces = (size_t)(g + kCols - 1) / kCols;
  Layout L;
  size_t o = 0;
  L.nvalid = o; o = align256(o + sizeof(int) * (size_t)n);
  L.claim = o;  o = align256(o + sizeof(int) * (size_t)nt * n * g);
  L.piou = o;   o = align256(o + sizeof(double) * (size_t)n * k * pieces);
  L.pgt = o;    o = align256(o + sizeof(int) * (size_t)n * k * pieces);
  L.total = o;
  return L;
}

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

__global__ void __launch_bounds__(kThreads) ap_rank_kernel(const float* __restrict__ scores,
                                                           const int* __restrict__ count, int k, int g, int nt,
                                                           int* __restrict__ rank, int* __restrict__ nvalid,
                                                           int* __restrict__ claim, unsigned long long* status) {
  __shared__ float s[kMaxK];
  __shared__ int nv;
  const int img = blockIdx.x, n = gridDim.x;
  const int c = clampi(count[img], k);
  if (threadIdx.x == 0) nv = 0;
  for (int i = threadIdx.x; i < c; i += kThreads) s[i] = scores[(size_t)img * k + i];
  __syncthreads();
  bool bad = false;
  for (int i = threadIdx.x; i < k; i += kThreads) {
    int r = -1;
    if (i < c) {
      const float si = s[i];
      if (isfinite(si)) {
        r = 0;
        for (int q = 0; q < c; ++q) {
          const float sq = s[q];
          r += (isfinite(sq) && (sq > si || (sq == si && q < i))) ? 1 : 0;
        }
        atomicAdd(&nv, 1);
      } else {
        bad = true;
      }
    }
    rank[(size_t)img * k + i] = r;
  }
  if (bad && status) atomicOr(status, 2ull);
  for (int e = threadIdx.x; e < nt * g; e += kThreads) {
    const int t = e / g, j = e - t * g;
    claim[((size_t)t * n + img) * g + j] = INT_MAX;
  }
  __syncthreads();
  if (threadIdx.x == 0) nvalid[img] = nv;
}

// Lane t is row i = 64 * rb + t; the tile's columns are j0 .. j0 + 15 of the image's ground truth.
__global__ void __launch_bounds__(64) ap_iou_kernel(const float* __restrict__ boxes, const int* __restrict__ count,
                                                    const int* __restrict__ rank, const float* __restrict__ gt,
                                                    const int* __restrict__ gt_count, int k, int g, int pieces,
                                                    double* __restrict__ piou, int* __restrict__ pgt) {
#pragma clang fp contract(off)
  __shared__ double cxs[4][kCols], cys[4][kCols], ccx[kCols], ccy[kCols], crad[kCols], carea[kCols];
  __shared__ double bufx[2][dn::kClipCap][64], bufy[2][dn::kClipCap][64];
  const int piece = blockIdx.x, rb = blockIdx.y, img = blockIdx.z, t = threadIdx.x;
  const int c = clampi(count[img], k), gc = clampi(gt_count[img], g);
  const int j0 = piece * kCols;
  if (j0 >= gc || rb * 64 >= c) return;
  if (t < kCols && j0 + t < gc) {
    dn::Box64 b;
    dn::box64(gt + 6 * ((size_t)img * g + j0 + t), b);
    for (int q = 0; q < 4; ++q) {
      cxs[q][t] = b.x[q];
      cys[q][t] = b.y[q];
    }
    ccx[t] = b.cx;
    ccy[t] = b.cy;
    crad[t] = b.radius;
    carea[t] = b.area;
  }
  __syncthreads();
  const int i = rb * 64 + t;
  if (i >= c || rank[(size_t)img * k + i] < 0) return;
  dn::Box64 a;
  dn::box64(boxes + 6 * ((size_t)img * k + i), a);
  double best = 0.0;
  int best_j = -1;
  const int jend = gc - j0 < kCols ? gc - j0 : kCols;
  for (int jj = 0; jj < jend; ++jj) {
    const double dist = hypot(ccx[jj] - a.cx, ccy[jj] - a.cy);
    if (!(dist < crad[jj] + a.radius)) continue;   // circumscribed circles apart: IoU 0
    double bx[4], by[4];
    for (int q = 0; q < 4; ++q) {
      bx[q] = cxs[q][jj];
      by[q] = cys[q][jj];
    }
    const double inter = dn::intersection_area(a.x, a.y, bx, by, &bufx[0][0][t], &bufy[0][0][t], &bufx[1][0][t],
                                               &bufy[1][0][t]);
    const double uni = a.area + carea[jj] - inter;
    const double iou = uni > 0 ? inter / uni : 0.0;
    if (iou > best) {
      best = iou;
      best_j = j0 + jj;
    }
  }
  const size_t o = ((size_t)img * k + i) * pieces + piece;
  piou[o] = best;
  pgt[o] = best_j;
}

__global__ void __launch_bounds__(kThreads) ap_claim_kernel(const int* __restrict__ count, const int* __restrict__ rank,
                                                            const int* __restrict__ gt_count, int k, int g, int pieces,
                                                            const double* __restrict__ piou,
                                                            const int* __restrict__ pgt, Thresholds thr, int nt,
                                                            double* __restrict__ best_iou, int* __restrict__ best_gt,
                                                            int* __restrict__ claim) {
  const int img = blockIdx.y, n = gridDim.y;
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= k) return;
  const size_t row = (size_t)img * k + i;
  const int c = clampi(count[img], k), gc = clampi(gt_count[img], g);
  const int r = rank[row];
  double best = 0.0;
  int best_j = -1;
  if (i < c && r >= 0) {
    const int np = (gc + kCols - 1) / kCols;
    for (int p = 0; p < np; ++p) {
      const double v = piou[row * pieces + p];
      if (v > best) {
        best = v;
        best_j = pgt[row * pieces + p];
      }
    }
    if (best_j >= 0)
      for (int t = 0; t < nt; ++t)
        if (best >= thr.t[t]) atomicMin(&claim[((size_t)t * n + img) * g + best_j], r);
  }
  best_iou[row] = best;
  best_gt[row] = best_j;
}

__global__ void __launch_bounds__(kThreads) ap_tp_kernel(const float* __restrict__ scores, const int* __restrict__ rank,
                                                         const int* __restrict__ nvalid,
                                                         const double* __restrict__ best_iou,
                                                         const int* __restrict__ best_gt, const int* __restrict__ claim,
                                                         int k, int g, Thresholds thr, int nt,
                                                         unsigned char* __restrict__ tp, uint2* __restrict__ records,
                                                         long long capacity, const long long* __restrict__ state,
                                                         int batch) {
  __shared__ int before;
  const int img = blockIdx.y, n = gridDim.y;
  if (records) {
    if (threadIdx.x == 0) before = 0;
    __syncthreads();
    int part = 0;
    for (int q = threadIdx.x; q < img; q += kThreads) part += nvalid[q];
    if (part) atomicAdd(&before, part);
    __syncthreads();
  }
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= k) return;
  const size_t row = (size_t)img * k + i;
  const int r = rank[row], j = best_gt[row];
  const double best = best_iou[row];
  unsigned bits = 0;
  for (int t = 0; t < nt; ++t) {
    const bool hit = r >= 0 && j >= 0 && best >= thr.t[t] && claim[((size_t)t * n + img) * g + j] == r;
    tp[((size_t)t * n + img) * k + i] = hit ? 1 : 0;
    bits |= hit ? 1u << t : 0u;
  }
  if (records && r >= 0) {
    const long long pos = state[0] + before + r;
    if (pos < capacity) records[pos] = make_uint2(__float_as_uint(scores[row]), ((unsigned)(img / batch) << 8) | bits);
  }
}

__global__ void ap_advance_kernel(const int* __restrict__ nvalid, const int* __restrict__ gt_count, int n, int g,
                                  long long capacity, long long* state, int batch) {
  long long total = 0;
  for (int q = 0; q < n; ++q) {
    total += nvalid[q];
    state[2 + q / batch] += clampi(gt_count[q], g);
  }
  if (state[0] + total > capacity) state[1] |= 1;
  state[0] += total;
}

__global__ void ap_reset_kernel(long long* state, int words) {
  for (int q = 0; q < words; ++q) state[q] = 0;
}

bool shapes_ok(int n, int k, int g, int nt) {
  return n > 0 && n <= 65535 && k >= 1 && k <= kMaxK && g >= 1 && g <= kMaxG && nt >= 1 && nt <= kMaxT;
}

}  // namespace

extern "C" size_t dn_ap_match_workspace_bytes(int n_images, int k, int g, int n_thr) {
  if (!shapes_ok(n_images, k, g, n_thr)) return 0;
  return layout(n_images, k, g, n_thr).total;
}

extern "C" int dn_ap_match(const float* boxes, const float* scores, const int32_t* count, const float* gt_boxes,
                           const int32_t* gt_count, int n_images, int k, int g, const double* iou_thrs, int n_thr,
                           double* best_iou, int32_t* best_gt, int32_t* rank, uint8_t* tp, void* workspace,
                           size_t workspace_bytes, void* records, long long capacity, long long* state, int n_agents,
                           int batch, void* stream) {
  DN_REQUIRE(boxes && scores && count && gt_boxes && gt_count && iou_thrs && best_iou && best_gt && rank && tp &&
                 workspace, "ap_match: null pointer");
  DN_REQUIRE(n_images > 0 && n_images <= 65535, "ap_match: %d images is out of range [1, 65535]", n_images);
  DN_REQUIRE(k >= 1 && k <= kMaxK, "ap_match: K = %d detection rows, must be in [1, %d]", k, kMaxK);
  DN_REQUIRE(g >= 1 && g <= kMaxG, "ap_match: G = %d ground-truth rows, must be in [1, %d]", g, kMaxG);
  DN_REQUIRE(n_thr >= 1 && n_thr <= kMaxT, "ap_match: T = %d thresholds, must be in [1, %d]", n_thr, kMaxT);
  Thresholds thr = {};
  for (int t = 0; t < n_thr; ++t) {
    DN_REQUIRE(iou_thrs[t] > 0 && iou_thrs[t] <= 1, "ap_match: threshold %d = %g, must be in (0, 1]", t, iou_thrs[t]);
    thr.t[t] = iou_thrs[t];
  }
  const Layout L = layout(n_images, k, g, n_thr);
  DN_REQUIRE(workspace_bytes >= L.total,
             "ap_match: workspace of %zu bytes, %zu needed (dn_ap_match_workspace_bytes)", workspace_bytes, L.total);
  if (records) {
    DN_REQUIRE(state, "ap_match: null accumulator state");
    DN_REQUIRE(capacity > 0, "ap_match: record capacity = %lld, must be positive", capacity);
    DN_REQUIRE(batch >= 1 && n_agents >= 1 && n_agents <= kMaxAgents && (n_images + batch - 1) / batch <= n_agents,
               "ap_match: %d images at batch %d do not fit %d agent counters (at most %d)", n_images, batch, n_agents,
               kMaxAgents);
  }
  hipStream_t s = (hipStream_t)stream;
  char* ws = static_cast<char*>(workspace);
  int* nvalid = reinterpret_cast<int*>(ws + L.nvalid);
  int* claim = reinterpret_cast<int*>(ws + L.claim);
  double* piou = reinterpret_cast<double*>(ws + L.piou);
  int* pgt = reinterpret_cast<int*>(ws + L.pgt);
  const int pieces = (g + kCols - 1) / kCols;
  const dim3 rows((unsigned)((k + kThreads - 1) / kThreads), (unsigned)n_images);
  unsigned long long* status = records ? reinterpret_cast<unsigned long long*>(state + 1) : nullptr;
  hipLaunchKernelGGL(ap_rank_kernel, dim3(n_images), dim3(kThreads), 0, s, scores, count, k, g, n_thr, rank, nvalid,
                     claim, status);
  hipLaunchKernelGGL(ap_iou_kernel, dim3(pieces, (k + 63) / 64, n_images), dim3(64), 0, s, boxes, count, rank, gt_boxes,
                     gt_count, k, g, pieces, piou, pgt);
  hipLaunchKernelGGL(ap_claim_kernel, rows, dim3(kThreads), 0, s, count, rank, gt_count, k, g, pieces, piou, pgt, thr,
                     n_thr, best_iou, best_gt, claim);
  hipLaunchKernelGGL(ap_tp_kernel, rows, dim3(kThreads), 0, s, scores, rank, nvalid, best_iou, best_gt, claim, k, g, thr,
                     n_thr, tp, static_cast<uint2*>(records), capacity, state, batch);
  if (records)
    hipLaunchKernelGGL(ap_advance_kernel, dim3(1), dim3(1), 0, s, nvalid, gt_count, n_images, g, capacity, state, batch);
  return dn::check_launch("ap_match");
}

extern "C" int dn_ap_reset(long long* state, int n_agents, void* stream) {
  DN_REQUIRE(state, "ap_reset: null accumulator state");
  DN_REQUIRE(n_agents >= 1 && n_agents <= kMaxAgents, "ap_reset: %d agent counters, must be in [1, %d]", n_agents,
             kMaxAgents);
  hipLaunchKernelGGL(ap_reset_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, state, 2 + n_agents);
  return dn::check_launch("ap_reset");
}
