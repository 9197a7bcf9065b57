// Identity metrics of the tracks (IDF1 / IDP / IDR beside the CLEAR figures of mot_eval.hip): per frame the count of
// every (ground-truth identity, track id) pair that overlaps at the threshold, kept on the device for the whole
// sequence; at the end ONE global assignment over that matrix.  The contract is in include/disconet_hip.h; the host
// reference that defines the bits is tracking.HostIdentity.  The IoU is fp64 in a fixed order, + - * / and sqrt only,
// and every function that touches fp64 carries `#pragma clang fp contract(off)`.
//
// idf_step_kernel: one launch per frame, one workgroup of ONE wave per image, as mot_step_kernel (its measure and
// dedupe phases and row_rect / rect_iou are copied here; mot_eval.hip is not touched):
//   measure    lanes over ground-truth rows, 64 at a time in row order -> the first 128 valid rows in LDS
//   dedupe     a kept row whose id a lower kept row carries leaves (stable compaction)
//   tracks     lanes over reported rows: the id's range (status bit 16), the column t - 1, track_count bumped with an
//              integer atomicAdd (the same id may come on two rows of a frame), the rectangle to LDS
//   pairs      lanes over (ground truth, track) pairs: not iou < threshold -> atomicAdd on the matrix word in global
//              memory and on the row's overlap count in LDS.  Integer adds: the result does not depend on the order
//   counts     gt_count by the lane that owns the row (ids are unique after dedupe); one lane adds to the header
//   outputs    lanes over ground-truth rows; every word of `overlaps` is written once
// 10 KB of LDS.
//
// idf_finish_kernel: one workgroup per image, reads the state only.  The ids present (gt_count > 0, track_count > 0)
// are compacted into LDS lists in ascending order by ballot prefix; then tracking.hungarian_max to the letter -- the
// shortest-augmenting-path step of track.hip / mot_eval.hip (its own copy), in fp64 (all values are integers below
// 2^31, every sum is exact), rows the smaller side.  The weights are NOT copied: each step reads one word per lane from
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
constexpr int kHeaderBytes = 64;    // int64 frames, gt_dets, dets; int32 status; 36 spare bytes
constexpr int kLdsPerCu = 160 * 1024;

struct Params {
  int m, g, ids, tids;
  double thr, scale;
};

__host__ __device__ inline size_t image_bytes(int ids, int tids) {
  return (size_t)kHeaderBytes + 4 * ((size_t)ids + (size_t)tids + (size_t)ids * (size_t)tids);
}

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }
__device__ __forceinline__ int below(unsigned long long mask, int lane) {
  return __popcll(mask & ((1ull << lane) - 1ull));
}
// The header's int64 words as two int32 halves: an image's state is a multiple of 4 bytes, not of 8.
__device__ __forceinline__ long long load64(const int* w) {
  return (long long)(((unsigned long long)(unsigned)w[1] << 32) | (unsigned long long)(unsigned)w[0]);
}
__device__ __forceinline__ void store64(int* w, long long v) {
  w[0] = (int)(unsigned)((unsigned long long)v & 0xffffffffull);
  w[1] = (int)(unsigned)((unsigned long long)v >> 32);
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

  // ---- tracks: the reported rows, their columns and their counts
  const int K = clampi(tcount[img], m);
  int dets = 0;
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
      hits[dst] = 0;
    }
    V += __popcll(mask);
  }
  __syncthreads();

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
  const unsigned all = (__any(flags & 1u) ? 1u : 0u) | (__any(flags & 2u) ? 2u : 0u) | (__any(flags & 4u) ? 4u : 0u) |
                       (__any(flags & 8u) ? 8u : 0u) | (__any(flags & 16u) ? 16u : 0u);
  if (lane == 0) {
    store64(hdr + 0, load64(hdr + 0) + 1);
    store64(hdr + 2, load64(hdr + 2) + V);
    store64(hdr + 4, load64(hdr + 4) + dets);
    hdr[6] = hdr[6] | (int)all;
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
    out_overlaps[(size_t)img * g + r] = lo < V && grow[lo] == r ? hits[lo] : 0;
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
  int R = 0, C = 0;
  for (int base = 0; base < ids; base += kThreads) {
    const int i = base + lane;
    const bool on = i < ids && gcnt[i] > 0;
    const unsigned long long mask = __ballot(on);
    if (on) rowid[R + below(mask, lane)] = (unsigned short)i;
    R += __popcll(mask);
    if (i < ids) mout[i] = 0;
  }
  for (int base = 0; base < tids; base += kThreads) {
    const int i = base + lane;
    const bool on = i < tids && tcnt[i] > 0;
    const unsigned long long mask = __ballot(on);
    if (on) colid[C + below(mask, lane)] = (unsigned short)i;
    C += __popcll(mask);
  }
  __syncthreads();

  // ---- assign: tracking.hungarian_max(pairs[rows][cols] as fp64), rows the smaller side
  long long idtp = 0;
  if (R > 0 && C > 0) {   // wave-uniform
    const bool tp = R > C;                         // rows are the track ids when there are more identities
    const int n = tp ? C : R, mm = tp ? R : C;
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
      if (lane == 0) hp[0] = (short)i;
      __syncthreads();
      int j0 = 0;
      bool found = false;
      for (int step = 0; step <= mm; ++step) {
        if (lane == 0) hused[j0] = 1;
        __syncthreads();
        const int i0 = hp[j0] < 1 ? 1 : (hp[j0] > n ? n : hp[j0]);
        const double ui0 = hu[i0];
        // the row's words: contiguous ids along the matrix row, or one column of it at a stride of tids words
        const int* wrow = tp ? pairs + colid[i0 - 1] : pairs + (size_t)rowid[i0 - 1] * tids;
        double best = inf;
        int bj = INT_MAX;
        for (int j = 1 + lane; j <= mm; j += kThreads) {
          if (hused[j]) continue;
          const int w = tp ? wrow[(size_t)rowid[j - 1] * tids] : wrow[colid[j - 1]];
          const double cost = -(double)w;
          const double cur = (cost - ui0) - hv[j];
          double mv = hminv[j];
          if (cur < mv) {
            mv = cur; hminv[j] = cur; hway[j] = (short)j0;
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
        if (bj == INT_MAX) break;                  // nothing to reach (cannot happen with integer weights): the row stays free
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
  DN_REQUIRE(rect, "idf_step: null rect");
  DN_REQUIRE(id, "idf_step: null id");
  DN_REQUIRE(count, "idf_step: null count");
  DN_REQUIRE(gt_boxes, "idf_step: null gt_boxes");
  DN_REQUIRE(gt_ids, "idf_step: null gt_ids");
  DN_REQUIRE(gt_count, "idf_step: null gt_count");
  DN_REQUIRE(state, "idf_step: null state");
  DN_REQUIRE(out_overlaps, "idf_step: null out_overlaps");
  DN_IDF_SIZES("idf_step");
  DN_REQUIRE(m >= 1 && m <= kMaxM, "idf_step: M = %d track rows, must be in [1, %d]", m, kMaxM);
  DN_REQUIRE(g >= 1 && g <= kMaxG, "idf_step: G = %d ground-truth rows, must be in [1, %d]", g, kMaxG);
  DN_REQUIRE(std::isfinite(scale) && scale > 0, "idf_step: scale = %g, must be finite and > 0", scale);
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
  int dev = 0;
  (void)hipGetDevice(&dev);
  bool& lds_ready = lds_flag.here();
  if (!lds_ready) {
    hipFuncAttributes attr;
    if (hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(idf_finish_kernel)) != hipSuccess)
      return dn::fail(DN_ERR_LAUNCH, "idf_finish: cannot read the kernel's attributes");
    static_lds[dev & 63] = (int)attr.sharedSizeBytes;
    lds_ready = true;
  }
  if (static_lds[dev & 63] > kLdsPerCu)            // never spill: a launch that does not fit is refused
    return dn::fail(DN_ERR_LAUNCH, "idf_finish: %d B of work arrays do not fit %d B of LDS", static_lds[dev & 63],
                    kLdsPerCu);
  hipLaunchKernelGGL(idf_finish_kernel, dim3(n_images), dim3(kThreads), 0, (hipStream_t)stream,
                     static_cast<const unsigned char*>(state), max_gt_ids, max_track_ids,
                     reinterpret_cast<long long*>(out_counts), out_match);
  return dn::check_launch("idf_finish");
}
