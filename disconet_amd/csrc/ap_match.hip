// Detection mAP, the per-frame part on the GPU: every detection of every image is ranked by score, matched to its best
// ground-truth box (rotated IoU in fp64, rot_iou_device.h), marked true / false positive at up to 8 IoU thresholds
// (mmdetection's tpfp_default: the first claimant of a ground-truth box in score order wins) and, optionally, appended as a
// record to caller-owned arrays at a device-resident cursor.  The host reference is postprocess.host_match_ground_truth.
//
// Launch sequence (fixed: it depends on the shapes only, never on the data; nothing is read back, nothing is allocated):
//   ap_rank      one workgroup per image: rank of every row in the stable descending score order, the number of valid
//                rows (row < count and a finite score), the non-finite status bit, the claim words set to INT_MAX
//   ap_iou       tile (64 rows, 16-column ground-truth piece) per wave: rot_iou_device.h's columns, circle test and IoU
//                (stage_columns, circles_meet, pair_iou: the pair body of the NMS and of the anchor assignment); the
//                piece's best (IoU, lowest column) per row
//   ap_claim     per row: the pieces folded in column order (strict >, so the lowest column that attains the maximum wins);
//                per threshold an integer atomicMin of the row's rank into the claim word of its ground-truth box
//   ap_tp        per row and threshold: true positive when the row's rank is the claim word; the record at
//                cursor + (valid rows of the images before) + rank
//   ap_advance   one thread: cursor += valid rows, the overflow status bit, the per-agent ground-truth counters
// Only integer atomics are used and every order is decided by (score, row index): two runs write the same bytes.
//
// Stratified form (dn_ap_match_strata: every ground-truth box carries a stratum, dn_gt_strata computes one): the same
// ap_rank / ap_iou / ap_claim launches, then
//   ap_tp_strata     ap_tp's bits (one device function serves both kernels) and a 16-byte record that adds the stratum of
//                    the row's best_gt and the reach bits (best_iou >= threshold, claim won or not)
//   ap_strata_count  one workgroup per image: the image's boxes per stratum in LDS integer counters, the claim words
//                    as gt_claim, the bad-stratum status bit
//   ap_strata_advance  thread s folds stratum s of every image, in image order, into the agents' counters; thread 0
//                    moves the cursor
#include <climits>
#include <cmath>

#include "dn_internal.h"
#include "rot_iou_device.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxK = dn::kMaxBoxRows;
constexpr int kMaxG = dn::kMaxGtRows;
constexpr int kMaxT = 8;       // thresholds: one bit each in a record's flag byte
constexpr int kCols = 16;      // ground-truth columns per tile
constexpr int kMaxAgents = 65536;
using dn::clampi;

struct Thresholds {
  double t[kMaxT];
};

struct Layout {
  size_t nvalid, claim, piou, pgt, total;
};

Layout layout(int n, int k, int g, int nt) {
  const size_t pieces = (size_t)(g + kCols - 1) / kCols;
  dn::Carver c;
  Layout L;
  L.nvalid = c.take(sizeof(int) * (size_t)n);
  L.claim = c.take(sizeof(int) * (size_t)nt * n * g);
  L.piou = c.take(sizeof(double) * (size_t)n * k * pieces);
  L.pgt = c.take(sizeof(int) * (size_t)n * k * pieces);
  L.total = c.at;
  return L;
}

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
  __shared__ dn::BoxColumns<kCols> cols;
  __shared__ dn::ClipScratch scratch;
  const int piece = blockIdx.x, rb = blockIdx.y, img = blockIdx.z, t = threadIdx.x;
  const int c = clampi(count[img], k), gc = clampi(gt_count[img], g);
  const int j0 = piece * kCols;
  if (j0 >= gc || rb * 64 >= c) return;
  const int jend = gc - j0 < kCols ? gc - j0 : kCols;
  dn::stage_columns(cols, gt + 6 * ((size_t)img * g + j0), jend, t);
  __syncthreads();
  const int i = rb * 64 + t;
  if (i >= c || rank[(size_t)img * k + i] < 0) return;
  dn::Box64 a;
  dn::box64(boxes + 6 * ((size_t)img * k + i), a);
  double best = 0.0;
  int best_j = -1;
  for (int jj = 0; jj < jend; ++jj) {
    if (!dn::circles_meet(cols, jj, a)) continue;   // circumscribed circles apart: IoU 0
    const double iou = dn::pair_iou(cols, jj, a, scratch, t);
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

// The valid rows of the images before `img` (block-wide: every thread of the workgroup calls it).
__device__ __forceinline__ int rows_before(const int* __restrict__ nvalid, int img) {
  __shared__ int before;
  if (threadIdx.x == 0) before = 0;
  __syncthreads();
  int part = 0;
  for (int q = threadIdx.x; q < img; q += kThreads) part += nvalid[q];
  if (part) atomicAdd(&before, part);
  __syncthreads();
  return before;
}

// Row i of image img with rank r, best ground truth j at IoU `best`: its tp bytes, and the same as bits.
__device__ __forceinline__ unsigned tp_bits(int r, int j, double best, const int* __restrict__ claim, int img, int n,
                                            int i, int k, int g, const Thresholds& thr, int nt,
                                            unsigned char* __restrict__ tp) {
  unsigned bits = 0;
  for (int t = 0; t < nt; ++t) {
    const bool hit = r >= 0 && j >= 0 && best >= thr.t[t] && claim[((size_t)t * n + img) * g + j] == r;
    tp[((size_t)t * n + img) * k + i] = hit ? 1 : 0;
    bits |= hit ? 1u << t : 0u;
  }
  return bits;
}

__global__ void __launch_bounds__(kThreads) ap_tp_kernel(const float* __restrict__ scores, const int* __restrict__ rank,
                                                         const int* __restrict__ nvalid,
                                                         const double* __restrict__ best_iou,
                                                         const int* __restrict__ best_gt, const int* __restrict__ claim,
                                                         int k, int g, Thresholds thr, int nt,
                                                         unsigned char* __restrict__ tp, uint2* __restrict__ records,
                                                         long long capacity, const long long* __restrict__ state,
                                                         int batch) {
  const int img = blockIdx.y, n = gridDim.y;
  const int before = records ? rows_before(nvalid, img) : 0;
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= k) return;
  const size_t row = (size_t)img * k + i;
  const int r = rank[row];
  const unsigned bits = tp_bits(r, best_gt[row], best_iou[row], claim, img, n, i, k, g, thr, nt, tp);
  if (records && r >= 0) {
    const long long pos = state[0] + before + r;
    if (pos < capacity) records[pos] = make_uint2(__float_as_uint(scores[row]), ((unsigned)(img / batch) << 8) | bits);
  }
}

// One thread: the cursor past this call's `total` records, the overflow status bit.
__device__ __forceinline__ void advance_cursor(long long total, long long capacity, long long* state) {
  if (state[0] + total > capacity) state[1] |= 1;
  state[0] += total;
}

__global__ void ap_advance_kernel(const int* __restrict__ nvalid, const int* __restrict__ gt_count, int n, int g,
                                  long long capacity, long long* state, int batch) {
  long long total = 0;
  for (int q = 0; q < n; ++q) {
    total += nvalid[q];
    state[2 + q / batch] += clampi(gt_count[q], g);
  }
  advance_cursor(total, capacity, state);
}

__global__ void ap_reset_kernel(long long* state, int words) {
  for (int q = 0; q < words; ++q) state[q] = 0;
}

// ---- the stratified form ---------------------------------------------------------------------------------------------
constexpr int kMaxS = 8;       // strata: (stratum + 1) fits the record's third word beside the reach byte
constexpr int kMaxEdges = kMaxS - 1;

struct Edges {
  double e[kMaxEdges];
};

// a stratum word as the kernels count it: anything outside [-1, ns) is a don't-care box
__device__ __forceinline__ int stratum_of(int word, int ns) { return (word < -1 || word >= ns) ? -1 : word; }

__global__ void __launch_bounds__(kThreads) gt_strata_kernel(const float* __restrict__ gt,
                                                             const int* __restrict__ gt_count,
                                                             const int* __restrict__ own_hits, int g, int mode, Edges edges,
                                                             int ne, int* __restrict__ stratum) {
#pragma clang fp contract(off)
  const int img = blockIdx.y, j = blockIdx.x * kThreads + threadIdx.x;
  if (j >= g) return;
  const size_t row = (size_t)img * g + j;
  int st = -1;
  if (j < clampi(gt_count[img], g)) {
    double v;
    bool ok = true;
    if (mode == 0) {      // edges.e holds the squared edges: no square root, no division
      const float x = gt[6 * row], y = gt[6 * row + 1];
      const double xx = (double)x * (double)x, yy = (double)y * (double)y;
      v = xx + yy;
      ok = isfinite(x) && isfinite(y);
    } else {
      v = (double)own_hits[row];
    }
    if (ok) {
      st = 0;
      for (int e = 0; e < ne; ++e) st += v >= edges.e[e] ? 1 : 0;
    }
  }
  stratum[row] = st;
}

__global__ void __launch_bounds__(kThreads) ap_tp_strata_kernel(
    const float* __restrict__ scores, const int* __restrict__ rank, const int* __restrict__ nvalid,
    const double* __restrict__ best_iou, const int* __restrict__ best_gt, const int* __restrict__ claim,
    const int* __restrict__ gt_stratum, int k, int g, Thresholds thr, int nt, int ns, unsigned char* __restrict__ tp,
    uint4* __restrict__ records, long long capacity, const long long* __restrict__ state, int batch) {
  const int img = blockIdx.y, n = gridDim.y;
  const int before = records ? rows_before(nvalid, img) : 0;
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= k) return;
  const size_t row = (size_t)img * k + i;
  const int r = rank[row], j = best_gt[row];
  const double best = best_iou[row];
  const unsigned bits = tp_bits(r, j, best, claim, img, n, i, k, g, thr, nt, tp);
  if (records && r >= 0) {
    unsigned reach = 0;
    int st = -1;
    if (j >= 0) {      // j < the image's clamped gt_count: ap_iou looks at no other column
      for (int t = 0; t < nt; ++t) reach |= best >= thr.t[t] ? 1u << t : 0u;
      st = stratum_of(gt_stratum[(size_t)img * g + j], ns);
    }
    const long long pos = state[0] + before + r;
    if (pos < capacity)
      records[pos] = make_uint4(__float_as_uint(scores[row]), ((unsigned)(img / batch) << 8) | bits,
                                ((unsigned)(st + 1) << 8) | reach, (unsigned)j);
  }
}

// counts [n][ns + 1]: the image's boxes per stratum, the don't-care boxes at [ns]
__global__ void __launch_bounds__(kThreads) ap_strata_count_kernel(const int* __restrict__ gt_count,
                                                                   const int* __restrict__ gt_stratum,
                                                                   const int* __restrict__ claim, int g, int nt, int ns,
                                                                   int* __restrict__ counts, int* __restrict__ gt_claim,
                                                                   unsigned long long* status) {
  __shared__ int c[kMaxS + 1];
  const int img = blockIdx.x, n = gridDim.x;
  const int gc = clampi(gt_count[img], g);
  if (threadIdx.x <= ns) c[threadIdx.x] = 0;
  __syncthreads();
  bool bad = false;
  for (int j = threadIdx.x; j < gc; j += kThreads) {
    const int word = gt_stratum[(size_t)img * g + j], st = stratum_of(word, ns);
    bad |= st != word;
    atomicAdd(&c[st < 0 ? ns : st], 1);
  }
  if (bad && status) atomicOr(status, 4ull);
  if (gt_claim)
    for (int e = threadIdx.x; e < nt * g; e += kThreads) {
      const int t = e / g, j = e - t * g;
      const size_t o = ((size_t)t * n + img) * g + j;
      const int v = claim[o];
      gt_claim[o] = (j < gc && v != INT_MAX) ? v : -1;
    }
  __syncthreads();
  if (threadIdx.x <= ns) counts[(size_t)img * (ns + 1) + threadIdx.x] = c[threadIdx.x];
}

// ns + 1 threads: thread s owns column s of every agent's counters
__global__ void ap_strata_advance_kernel(const int* __restrict__ nvalid, const int* __restrict__ counts, int n, int ns,
                                         long long capacity, long long* state, int batch) {
  const int s = threadIdx.x;
  for (int q = 0; q < n; ++q) state[2 + (size_t)(q / batch) * (ns + 1) + s] += counts[(size_t)q * (ns + 1) + s];
  if (s == 0) {
    long long total = 0;
    for (int q = 0; q < n; ++q) total += nvalid[q];
    advance_cursor(total, capacity, state);
  }
}

bool shapes_ok(int n, int k, int g, int nt) {
  return n > 0 && n <= dn::kMaxImages && k >= 1 && k <= kMaxK && g >= 1 && g <= kMaxG && nt >= 1 && nt <= kMaxT;
}

// What dn_ap_match and dn_ap_match_strata check alike, under the caller's name; fills `thr`.
int check_match(const char* who, bool pointers, int n_images, int k, int g, const double* iou_thrs, int n_thr,
                size_t workspace_bytes, size_t need, const void* records, long long capacity, const long long* state,
                int n_agents, int batch, Thresholds& thr) {
  DN_REQUIRE(pointers, "%s: null pointer", who);
  DN_REQUIRE(n_images > 0 && n_images <= dn::kMaxImages, "%s: %d images is out of range [1, 65535]", who, n_images);
  DN_REQUIRE(k >= 1 && k <= kMaxK, "%s: K = %d detection rows, must be in [1, %d]", who, k, kMaxK);
  DN_REQUIRE(g >= 1 && g <= kMaxG, "%s: G = %d ground-truth rows, must be in [1, %d]", who, g, kMaxG);
  DN_REQUIRE(n_thr >= 1 && n_thr <= kMaxT, "%s: T = %d thresholds, must be in [1, %d]", who, n_thr, kMaxT);
  for (int t = 0; t < n_thr; ++t) {
    DN_REQUIRE(iou_thrs[t] > 0 && iou_thrs[t] <= 1, "%s: threshold %d = %g, must be in (0, 1]", who, t, iou_thrs[t]);
    thr.t[t] = iou_thrs[t];
  }
  DN_REQUIRE(workspace_bytes >= need, "%s: workspace of %zu bytes, %zu needed (dn_%s_workspace_bytes)", who,
             workspace_bytes, need, who);
  if (records) {
    DN_REQUIRE(state, "%s: null accumulator state", who);
    DN_REQUIRE(capacity > 0, "%s: record capacity = %lld, must be positive", who, capacity);
    DN_REQUIRE(batch >= 1 && n_agents >= 1 && n_agents <= kMaxAgents && (n_images + batch - 1) / batch <= n_agents,
               "%s: %d images at batch %d do not fit %d agent counters (at most %d)", who, n_images, batch, n_agents,
               kMaxAgents);
  }
  return DN_OK;
}

// ap_rank, ap_iou, ap_claim: the phases both entries run, on the first `L.total` bytes of the workspace.
void launch_match(hipStream_t s, const Layout& L, char* ws, const float* boxes, const float* scores, const int32_t* count,
                  const float* gt_boxes, const int32_t* gt_count, int n_images, int k, int g, const Thresholds& thr,
                  int n_thr, double* best_iou, int32_t* best_gt, int32_t* rank, unsigned long long* status) {
  int* nvalid = reinterpret_cast<int*>(ws + L.nvalid);
  int* claim = reinterpret_cast<int*>(ws + L.claim);
  double* piou = reinterpret_cast<double*>(ws + L.piou);
  int* pgt = reinterpret_cast<int*>(ws + L.pgt);
  const int pieces = (g + kCols - 1) / kCols;
  const dim3 rows((unsigned)((k + kThreads - 1) / kThreads), (unsigned)n_images);
  hipLaunchKernelGGL(ap_rank_kernel, dim3(n_images), dim3(kThreads), 0, s, scores, count, k, g, n_thr, rank, nvalid,
                     claim, status);
  hipLaunchKernelGGL(ap_iou_kernel, dim3(pieces, (k + 63) / 64, n_images), dim3(64), 0, s, boxes, count, rank, gt_boxes,
                     gt_count, k, g, pieces, piou, pgt);
  hipLaunchKernelGGL(ap_claim_kernel, rows, dim3(kThreads), 0, s, count, rank, gt_count, k, g, pieces, piou, pgt, thr,
                     n_thr, best_iou, best_gt, claim);
}

size_t strata_counts_bytes(int n, int ns) { return dn::align256(sizeof(int) * (size_t)n * (ns + 1)); }

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
  Thresholds thr = {};
  const bool pointers = boxes && scores && count && gt_boxes && gt_count && iou_thrs && best_iou && best_gt && rank &&
                        tp && workspace;
  const size_t need = shapes_ok(n_images, k, g, n_thr) ? layout(n_images, k, g, n_thr).total : 0;
  if (int rc = check_match("ap_match", pointers, n_images, k, g, iou_thrs, n_thr, workspace_bytes, need, records,
                           capacity, state, n_agents, batch, thr))
    return rc;
  const Layout L = layout(n_images, k, g, n_thr);
  hipStream_t s = (hipStream_t)stream;
  char* ws = static_cast<char*>(workspace);
  unsigned long long* status = records ? reinterpret_cast<unsigned long long*>(state + 1) : nullptr;
  launch_match(s, L, ws, boxes, scores, count, gt_boxes, gt_count, n_images, k, g, thr, n_thr, best_iou, best_gt, rank,
               status);
  const int* nvalid = reinterpret_cast<const int*>(ws + L.nvalid);
  const dim3 rows((unsigned)((k + kThreads - 1) / kThreads), (unsigned)n_images);
  hipLaunchKernelGGL(ap_tp_kernel, rows, dim3(kThreads), 0, s, scores, rank, nvalid, best_iou, best_gt,
                     reinterpret_cast<const int*>(ws + L.claim), k, g, thr, n_thr, tp, static_cast<uint2*>(records),
                     capacity, state, batch);
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

extern "C" int dn_gt_strata(const float* gt_boxes, const int32_t* gt_count, const int32_t* gt_own_hits, int n_images,
                            int g, int mode, const double* edges, int n_edges, int32_t* stratum, void* stream) {
  DN_REQUIRE(gt_boxes && gt_count && edges && stratum, "gt_strata: null pointer");
  DN_REQUIRE(n_images > 0 && n_images <= dn::kMaxImages, "gt_strata: %d images is out of range [1, 65535]", n_images);
  DN_REQUIRE(g >= 1 && g <= kMaxG, "gt_strata: G = %d ground-truth rows, must be in [1, %d]", g, kMaxG);
  DN_REQUIRE(mode == 0 || mode == 1, "gt_strata: mode = %d, must be 0 (range) or 1 (own visibility)", mode);
  DN_REQUIRE(mode == 0 || gt_own_hits, "gt_strata: mode 1 (own visibility) needs gt_own_hits");
  DN_REQUIRE(n_edges >= 1 && n_edges <= kMaxEdges, "gt_strata: %d edges, must be in [1, %d]", n_edges, kMaxEdges);
  Edges e = {};
  for (int q = 0; q < n_edges; ++q) {
    DN_REQUIRE(std::isfinite(edges[q]) && edges[q] > 0 && (q == 0 || edges[q] > edges[q - 1]),
               "gt_strata: edge %d = %g, edges must be finite, positive and strictly ascending", q, edges[q]);
    DN_REQUIRE(mode == 0 || (edges[q] >= 1 && edges[q] <= 2147483647.0 && edges[q] == std::floor(edges[q])),
               "gt_strata: edge %d = %g, the edges of mode 1 are integers >= 1", q, edges[q]);
    e.e[q] = mode == 0 ? edges[q] * edges[q] : edges[q];
  }
  hipLaunchKernelGGL(gt_strata_kernel, dim3((unsigned)((g + kThreads - 1) / kThreads), (unsigned)n_images),
                     dim3(kThreads), 0, (hipStream_t)stream, gt_boxes, gt_count, gt_own_hits, g, mode, e, n_edges, stratum);
  return dn::check_launch("gt_strata");
}

extern "C" size_t dn_ap_match_strata_workspace_bytes(int n_images, int k, int g, int n_thr, int n_strata) {
  if (!shapes_ok(n_images, k, g, n_thr) || n_strata < 1 || n_strata > kMaxS) return 0;
  return layout(n_images, k, g, n_thr).total + strata_counts_bytes(n_images, n_strata);
}

extern "C" int dn_ap_match_strata(const float* boxes, const float* scores, const int32_t* count, const float* gt_boxes,
                                  const int32_t* gt_count, const int32_t* gt_stratum, int n_images, int k, int g,
                                  const double* iou_thrs, int n_thr, int n_strata, double* best_iou, int32_t* best_gt,
                                  int32_t* rank, uint8_t* tp, int32_t* gt_claim, void* workspace, size_t workspace_bytes,
                                  void* records, long long capacity, long long* state, int n_agents, int batch,
                                  void* stream) {
  Thresholds thr = {};
  const bool pointers = boxes && scores && count && gt_boxes && gt_count && gt_stratum && iou_thrs && best_iou &&
                        best_gt && rank && tp && workspace;
  DN_REQUIRE(n_strata >= 1 && n_strata <= kMaxS, "ap_match_strata: S = %d strata, must be in [1, %d]", n_strata, kMaxS);
  const size_t need = dn_ap_match_strata_workspace_bytes(n_images, k, g, n_thr, n_strata);
  if (int rc = check_match("ap_match_strata", pointers, n_images, k, g, iou_thrs, n_thr, workspace_bytes, need, records,
                           capacity, state, n_agents, batch, thr))
    return rc;
  DN_REQUIRE((reinterpret_cast<size_t>(records) & 15) == 0, "ap_match_strata: records must be 16-byte aligned");
  const Layout L = layout(n_images, k, g, n_thr);
  hipStream_t s = (hipStream_t)stream;
  char* ws = static_cast<char*>(workspace);
  unsigned long long* status = records ? reinterpret_cast<unsigned long long*>(state + 1) : nullptr;
  launch_match(s, L, ws, boxes, scores, count, gt_boxes, gt_count, n_images, k, g, thr, n_thr, best_iou, best_gt, rank,
               status);
  const int* nvalid = reinterpret_cast<const int*>(ws + L.nvalid);
  const int* claim = reinterpret_cast<const int*>(ws + L.claim);
  int* counts = reinterpret_cast<int*>(ws + L.total);
  const dim3 rows((unsigned)((k + kThreads - 1) / kThreads), (unsigned)n_images);
  hipLaunchKernelGGL(ap_tp_strata_kernel, rows, dim3(kThreads), 0, s, scores, rank, nvalid, best_iou, best_gt, claim,
                     gt_stratum, k, g, thr, n_thr, n_strata, tp, static_cast<uint4*>(records), capacity, state, batch);
  hipLaunchKernelGGL(ap_strata_count_kernel, dim3(n_images), dim3(kThreads), 0, s, gt_count, gt_stratum, claim, g, n_thr,
                     n_strata, counts, gt_claim, status);
  if (records)
    hipLaunchKernelGGL(ap_strata_advance_kernel, dim3(1), dim3(n_strata + 1), 0, s, nvalid, counts, n_images, n_strata,
                       capacity, state, batch);
  return dn::check_launch("ap_match_strata");
}

extern "C" int dn_ap_strata_reset(long long* state, int n_agents, int n_strata, void* stream) {
  DN_REQUIRE(state, "ap_strata_reset: null accumulator state");
  DN_REQUIRE(n_agents >= 1 && n_agents <= kMaxAgents, "ap_strata_reset: %d agent counters, must be in [1, %d]", n_agents,
             kMaxAgents);
  DN_REQUIRE(n_strata >= 1 && n_strata <= kMaxS, "ap_strata_reset: S = %d strata, must be in [1, %d]", n_strata, kMaxS);
  if (dn::zero_fill(state, sizeof(long long) * (2 + (size_t)n_agents * (n_strata + 1)), (hipStream_t)stream) != hipSuccess)
    return dn::fail(DN_ERR_LAUNCH, "ap_strata_reset: the zero fill failed");
  return dn::check_launch("ap_strata_reset");
}
