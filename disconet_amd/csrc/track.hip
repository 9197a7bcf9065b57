// Multi-object tracking behind the detection tail: one SORT step (Sort.update of Bewley et al.'s tracker with filterpy's
// constant-velocity Kalman filter, as recalled) for every image of a call.  The contract is in include/disconet_hip.h; the
// host reference that defines the bits is tracking.HostSort.  All arithmetic is fp64 in a fixed order, + - * / and sqrt
// only (the corners' hypot of postprocess._corners is written sqrt(s s + c c)), and every function carries `#pragma clang fp contract(off)`.
//
// One launch per step (track_step_kernel), one workgroup of ONE wave per image, every phase a lane-strided loop; the
// single-wave form, row_rect / rect_iou and the assignment are track_eval_device.h's, shared with the evaluations:
//   measure    lanes over detection rows, 64 at a time in row order: row_rect, validity (a finite score too), ballot
//              prefix -> the first 128 valid rows in LDS
//   predict    lanes over tracks: record (x[7], P[7][7], counters) from the state to registers, predicted, stored to its
//              slot after the wave-level prefix that drops tracks with a non-finite rectangle (stable compaction)
//   iou        lanes over (track, detection) pairs -> the matrix in LDS, [tracks][ld], ld odd so that a column walk
//              (lanes over tracks) is as free of bank conflicts as a row walk
//   associate  SORT's shortcut (<= 1 entry above the threshold in every row and column) or assign_rows on the matrix
//   update     lanes over tracks: Kalman update (Cholesky of S, Joseph form) in registers, deletions decided, stable
//              compaction, the report rows of the surviving tracks
//   birth      lanes over unmatched detections in row order -> free slots, new ids, their report rows
//   tail       output rows past the count and state slots past the list cleared; the header written by one lane
// The matrix lives in LDS: 8 * max_tracks * (min(k, 128) | 1) bytes of dynamic LDS, 132 KB at 128 x 128 (one workgroup per
// CU there, several at the usual sizes).  Nothing is read back, nothing is allocated; two runs write the same bytes.
#include <cmath>

#include "dn_internal.h"
#include "track_eval_device.h"

namespace {

using namespace dn::trk;

constexpr int kMaxD = kMaxV;      // valid detection rows used per image
constexpr int kMaxK = 1024;       // detection rows per image (dn_detect's limit for top_k)
constexpr int kHeaderBytes = 64;  // int32 frame_count, next_id, n_tracks, status, 12 spare words
constexpr int kRecDoubles = 56;   // x[7], P[7][7]
constexpr int kRecInts = 8;       // id, age, hits, hit_streak, time_since_update, 3 spare
constexpr int kRecBytes = 8 * kRecDoubles + 4 * kRecInts;

struct Params {
  int k, m, max_age, min_hits, ld;
  double thr, scale;
};

struct Track {
  double x[7], P[49];
  int id, age, hits, streak, tsu;
};

__device__ __forceinline__ unsigned char* record(unsigned char* img_state, int slot) {
  return img_state + kHeaderBytes + (size_t)kRecBytes * slot;
}

__device__ __forceinline__ void load_track(const unsigned char* rec, Track& t) {
  const double* d = reinterpret_cast<const double*>(rec);
#pragma unroll
  for (int i = 0; i < 7; ++i) t.x[i] = d[i];
#pragma unroll
  for (int i = 0; i < 49; ++i) t.P[i] = d[7 + i];
  const int* w = reinterpret_cast<const int*>(d + kRecDoubles);
  t.id = w[0]; t.age = w[1]; t.hits = w[2]; t.streak = w[3]; t.tsu = w[4];
}

__device__ __forceinline__ void store_track(unsigned char* rec, const Track& t) {
  double* d = reinterpret_cast<double*>(rec);
#pragma unroll
  for (int i = 0; i < 7; ++i) d[i] = t.x[i];
#pragma unroll
  for (int i = 0; i < 49; ++i) d[7 + i] = t.P[i];
  int* w = reinterpret_cast<int*>(d + kRecDoubles);
  w[0] = t.id; w[1] = t.age; w[2] = t.hits; w[3] = t.streak; w[4] = t.tsu;
  w[5] = 0; w[6] = 0; w[7] = 0;
}

// (u, v, s, r, ...) -> (x1, y1, x2, y2): w = sqrt(s r), h = s / w
__device__ __forceinline__ void state_rect(const double* x, double* r) {
#pragma clang fp contract(off)
  const double w = sqrt(x[2] * x[3]);
  const double h = x[2] / w;
  r[0] = x[0] - w / 2.0;
  r[1] = x[1] - h / 2.0;
  r[2] = x[0] + w / 2.0;
  r[3] = x[1] + h / 2.0;
}

__device__ __forceinline__ void predict(Track& t) {
#pragma clang fp contract(off)
  if (t.x[6] + t.x[2] <= 0) t.x[6] = 0.0;
#pragma unroll
  for (int i = 0; i < 3; ++i) t.x[i] = t.x[i] + t.x[i + 4];
  // A = F P (rows 0..2 take rows 4..6), B = A F^T (columns 0..2 take columns 4..6), + Q
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 7; ++j) t.P[7 * i + j] = t.P[7 * i + j] + t.P[7 * (i + 4) + j];
#pragma unroll
  for (int i = 0; i < 7; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) t.P[7 * i + j] = t.P[7 * i + j] + t.P[7 * i + j + 4];
  const double q[7] = {1.0, 1.0, 1.0, 1.0, 0.01, 0.01, 0.0001};
#pragma unroll
  for (int i = 0; i < 7; ++i) t.P[8 * i] = t.P[8 * i] + q[i];
  t.age += 1;
  if (t.tsu > 0) t.streak = 0;
  t.tsu += 1;
}

__device__ __forceinline__ void update(Track& t, const double* z) {
#pragma clang fp contract(off)
  const double R[4] = {1.0, 1.0, 10.0, 10.0};
  t.tsu = 0;
  t.hits += 1;
  t.streak += 1;
  double y[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) y[i] = z[i] - t.x[i];
  double L[16];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j <= i; ++j) {
      double s = i == j ? t.P[7 * i + j] + R[i] : t.P[7 * i + j];
#pragma unroll
      for (int k = 0; k < j; ++k) s = s - L[4 * i + k] * L[4 * j + k];
      L[4 * i + j] = i == j ? sqrt(s) : s / L[4 * j + j];
    }
  double K[28];
#pragma unroll
  for (int r = 0; r < 7; ++r) {
    double w[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      double s = t.P[7 * r + i];
#pragma unroll
      for (int k = 0; k < i; ++k) s = s - L[4 * i + k] * w[k];
      w[i] = s / L[4 * i + i];
    }
#pragma unroll
    for (int i = 3; i >= 0; --i) {
      double s = w[i];
#pragma unroll
      for (int k = i + 1; k < 4; ++k) s = s - L[4 * k + i] * K[4 * r + k];
      K[4 * r + i] = s / L[4 * i + i];
    }
  }
#pragma unroll
  for (int r = 0; r < 7; ++r) {
    double s = K[4 * r] * y[0];
#pragma unroll
    for (int j = 1; j < 4; ++j) s = s + K[4 * r + j] * y[j];
    t.x[r] = t.x[r] + s;
  }
  double A[49];   // I - K H
#pragma unroll
  for (int r = 0; r < 7; ++r)
#pragma unroll
    for (int c = 0; c < 7; ++c) {
      const double e = r == c ? 1.0 : 0.0;
      A[7 * r + c] = c < 4 ? e - K[4 * r + c] : e;
    }
  double AP[49];
#pragma unroll
  for (int r = 0; r < 7; ++r)
#pragma unroll
    for (int c = 0; c < 7; ++c) {
      double s = A[7 * r] * t.P[c];
#pragma unroll
      for (int k = 1; k < 7; ++k) s = s + A[7 * r + k] * t.P[7 * k + c];
      AP[7 * r + c] = s;
    }
#pragma unroll
  for (int r = 0; r < 7; ++r)
#pragma unroll
    for (int c = 0; c < 7; ++c) {
      double s = AP[7 * r] * A[7 * c];
#pragma unroll
      for (int k = 1; k < 7; ++k) s = s + AP[7 * r + k] * A[7 * c + k];
      double g = (K[4 * r] * R[0]) * K[4 * c];
#pragma unroll
      for (int j = 1; j < 4; ++j) g = g + (K[4 * r + j] * R[j]) * K[4 * c + j];
      t.P[7 * r + c] = s + g;
    }
}

__global__ void __launch_bounds__(kThreads) track_step_kernel(const float* __restrict__ boxes,
                                                              const float* __restrict__ scores,
                                                              const int* __restrict__ count, Params p,
                                                              unsigned char* __restrict__ state,
                                                              double* __restrict__ out_rect, int* __restrict__ out_id,
                                                              int* __restrict__ out_det, float* __restrict__ out_score,
                                                              int* __restrict__ out_count, int* __restrict__ det_track) {
#pragma clang fp contract(off)
  extern __shared__ double iou_m[];                // [tracks][p.ld]
  __shared__ double drect[4][kMaxD], trect[4][kMaxM];
  __shared__ int drow[kMaxD], match_t[kMaxM], match_d[kMaxD];
  __shared__ double hu[kMaxM + 1], hv[kMaxM + 1], hminv[kMaxM + 1];
  __shared__ int hp[kMaxM + 1], hway[kMaxM + 1], hused[kMaxM + 1];
  const int img = blockIdx.x, lane = threadIdx.x;
  const int k = p.k, m = p.m, ld = p.ld;
  unsigned char* st = state + (size_t)img * (kHeaderBytes + (size_t)kRecBytes * m);
  int* hdr = reinterpret_cast<int*>(st);
  const int fc = hdr[0] + 1;
  const int next_id = hdr[1];
  const int t0 = clampi(hdr[2], m);
  unsigned flags = 0;
  const float* sc = scores + (size_t)img * k;
  int* dtrk = det_track + (size_t)img * k;

  // ---- measure: the first kMaxD valid rows, in row order
  const int c = clampi(count[img], k);
  int nd = 0;
  for (int base = 0; base < k; base += kThreads) {
    const int r = base + lane;
    bool ok = false;
    double q[4] = {0, 0, 0, 0};
    if (r < k) dtrk[r] = -1;
    if (r < c) {
      const bool fin = row_rect(boxes + 6 * ((size_t)img * k + r), p.scale, q);
      ok = fin && isfinite(sc[r]) && q[2] - q[0] > 0 && q[3] - q[1] > 0;
      if (!ok) flags |= 2u;
    }
    const unsigned long long mask = __ballot(ok);
    const int pos = nd + below(mask, lane);
    if (ok) {
      if (pos < kMaxD) {
        drect[0][pos] = q[0]; drect[1][pos] = q[1]; drect[2][pos] = q[2]; drect[3][pos] = q[3];
        drow[pos] = r;
      } else {
        flags |= 4u;
      }
    }
    nd += __popcll(mask);
  }
  const int D = nd < kMaxD ? nd : kMaxD;

  // ---- predict: tracks with a non-finite rectangle leave, the others close ranks
  int T = 0;
  for (int base = 0; base < t0; base += kThreads) {
    const int t = base + lane;
    Track tr;
    double r[4];
    bool alive = false;
    if (t < t0) {
      load_track(record(st, t), tr);
      predict(tr);
      state_rect(tr.x, r);
      alive = isfinite(r[0]) && isfinite(r[1]) && isfinite(r[2]) && isfinite(r[3]);
    }
    const unsigned long long mask = __ballot(alive);
    const int dst = T + below(mask, lane);
    __syncthreads();                               // every record of the chunk is in registers before a slot is rewritten
    if (alive) {
      store_track(record(st, dst), tr);
      trect[0][dst] = r[0]; trect[1][dst] = r[1]; trect[2][dst] = r[2]; trect[3][dst] = r[3];
    }
    T += __popcll(mask);
  }
  __syncthreads();

  // ---- IoU matrix
  for (int e = lane; e < T * D; e += kThreads) {
    const int t = e / D, d = e - t * D;
    iou_m[t * ld + d] = rect_iou(trect[0][t], trect[1][t], trect[2][t], trect[3][t], drect[0][d], drect[1][d],
                                 drect[2][d], drect[3][d]);
  }
  __syncthreads();

  // ---- associate
  bool multi = false;
  for (int t = lane; t < T; t += kThreads) {
    int cnt = 0, first = -1;
    for (int d = 0; d < D; ++d)
      if (iou_m[t * ld + d] > p.thr) {
        if (cnt == 0) first = d;
        ++cnt;
      }
    match_t[t] = first;
    multi = multi || cnt > 1;
  }
  for (int d = lane; d < D; d += kThreads) {
    int cnt = 0;
    for (int t = 0; t < T; ++t) cnt += iou_m[t * ld + d] > p.thr ? 1 : 0;
    match_d[d] = -1;
    multi = multi || cnt > 1;
  }
  const bool hungarian = __any(multi) && T > 0 && D > 0;
  __syncthreads();
  if (hungarian) {   // wave-uniform
    const bool tp = T > D;                         // rows are the smaller side: the detections when T > D
    const int n = tp ? D : T, mm = tp ? T : D;
    for (int t = lane; t < T; t += kThreads) match_t[t] = -1;
    assign_rows(n, mm, lane, hu, hv, hminv, hp, hway, hused, [&](int row, int col) {
      return -(tp ? iou_m[col * ld + row] : iou_m[row * ld + col]);
    });
    for (int j = 1 + lane; j <= mm; j += kThreads) {
      const int i = clampi(hp[j], n);
      if (i > 0) match_t[tp ? j - 1 : i - 1] = tp ? i - 1 : j - 1;
    }
    __syncthreads();
  }
  for (int t = lane; t < T; t += kThreads) {
    const int d = match_t[t];
    if (d >= 0) {
      if (iou_m[t * ld + d] < p.thr) match_t[t] = -1;
      else match_d[d] = t;
    }
  }
  __syncthreads();

  // ---- update, deletions, the report rows of the tracks that stay
  double* orect = out_rect + (size_t)img * m * 4;
  int* oid = out_id + (size_t)img * m;
  int* odet = out_det + (size_t)img * m;
  float* oscore = out_score + (size_t)img * m;
  int ns = 0, nrep = 0;
  for (int base = 0; base < T; base += kThreads) {
    const int t = base + lane;
    Track tr;
    bool keep = false, rep = false;
    int drw = -1;
    if (t < T) {
      load_track(record(st, t), tr);
      const int d = match_t[t];
      if (d >= 0) {
        const double x1 = drect[0][d], y1 = drect[1][d], w = drect[2][d] - x1, h = drect[3][d] - y1;
        const double z[4] = {x1 + w / 2.0, y1 + h / 2.0, w * h, w / h};
        update(tr, z);
        drw = drow[d];
      }
      keep = !(tr.tsu > p.max_age);
      rep = keep && tr.tsu < 1 && drw >= 0 && (tr.streak >= p.min_hits || fc <= p.min_hits);
    }
    const unsigned long long mk = __ballot(keep), mr = __ballot(rep);
    const int dst = ns + below(mk, lane), rdst = nrep + below(mr, lane);
    __syncthreads();
    if (keep) store_track(record(st, dst), tr);
    if (drw >= 0) dtrk[drw] = tr.id;
    if (rep) {
      double r[4];
      state_rect(tr.x, r);
      orect[4 * rdst] = r[0]; orect[4 * rdst + 1] = r[1]; orect[4 * rdst + 2] = r[2]; orect[4 * rdst + 3] = r[3];
      oid[rdst] = tr.id;
      odet[rdst] = drw;
      oscore[rdst] = sc[drw];
    }
    ns += __popcll(mk);
    nrep += __popcll(mr);
  }
  __syncthreads();

  // ---- births: unmatched detections in row order take the free slots
  const int avail = m - ns;
  const bool rep_new = 0 >= p.min_hits || fc <= p.min_hits;
  int nu = 0;
  for (int base = 0; base < D; base += kThreads) {
    const int d = base + lane;
    const bool un = d < D && match_d[d] < 0;
    const unsigned long long mu = __ballot(un);
    const int ord = nu + below(mu, lane);
    const bool born = un && ord < avail;
    if (un && !born) flags |= 1u;
    const bool rep = born && rep_new;
    const unsigned long long mr = __ballot(rep);
    const int rdst = nrep + below(mr, lane);
    if (born) {
      Track tr;
      const double x1 = drect[0][d], y1 = drect[1][d], w = drect[2][d] - x1, h = drect[3][d] - y1;
      tr.x[0] = x1 + w / 2.0; tr.x[1] = y1 + h / 2.0; tr.x[2] = w * h; tr.x[3] = w / h;
      tr.x[4] = 0.0; tr.x[5] = 0.0; tr.x[6] = 0.0;
      const double p0[7] = {10.0, 10.0, 10.0, 10.0, 1e4, 1e4, 1e4};
#pragma unroll
      for (int i = 0; i < 49; ++i) tr.P[i] = 0.0;
#pragma unroll
      for (int i = 0; i < 7; ++i) tr.P[8 * i] = p0[i];
      tr.id = next_id + ord; tr.age = 0; tr.hits = 0; tr.streak = 0; tr.tsu = 0;
      store_track(record(st, ns + ord), tr);
      dtrk[drow[d]] = tr.id;
      if (rep) {
        double r[4];
        state_rect(tr.x, r);
        orect[4 * rdst] = r[0]; orect[4 * rdst + 1] = r[1]; orect[4 * rdst + 2] = r[2]; orect[4 * rdst + 3] = r[3];
        oid[rdst] = tr.id;
        odet[rdst] = drow[d];
        oscore[rdst] = sc[drow[d]];
      }
    }
    nu += __popcll(mu);
    nrep += __popcll(mr);
  }
  const int nborn = nu < avail ? nu : avail;
  const int nfinal = ns + nborn;

  // ---- tail: rows past the count, slots past the list, the header
  for (int r = nrep + lane; r < m; r += kThreads) {
    orect[4 * r] = 0.0; orect[4 * r + 1] = 0.0; orect[4 * r + 2] = 0.0; orect[4 * r + 3] = 0.0;
    oid[r] = -1;
    odet[r] = -1;
    oscore[r] = 0.f;
  }
  constexpr int kRecWords = kRecBytes / 8;
  for (int e = lane; e < (t0 - nfinal) * kRecWords; e += kThreads) {
    const int s = nfinal + e / kRecWords, w = e % kRecWords;
    reinterpret_cast<unsigned long long*>(record(st, s))[w] = 0ull;
  }
  const unsigned all = wave_or(flags);
  if (lane == 0) {
    hdr[0] = fc;
    hdr[1] = next_id + nborn;
    hdr[2] = nfinal;
    hdr[3] = hdr[3] | (int)all;
    out_count[img] = nrep;
  }
}

__global__ void __launch_bounds__(256) track_reset_kernel(unsigned long long* state, size_t words_per_image, size_t words) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < words; i += stride)
    state[i] = i % words_per_image == 0 ? (1ull << 32) : 0ull;   // word 0 = {frame_count 0, next_id 1}
}

bool shapes_ok(int n, int m) { return n > 0 && n <= 65535 && m >= 1 && m <= kMaxM; }

}  // namespace

extern "C" size_t dn_track_state_bytes(int n_images, int max_tracks) {
  if (!shapes_ok(n_images, max_tracks)) return 0;
  return (size_t)n_images * (kHeaderBytes + (size_t)kRecBytes * max_tracks);
}

extern "C" int dn_track_reset(void* state, int n_images, int max_tracks, void* stream) {
  DN_REQUIRE(state, "track_reset: null state");
  DN_REQUIRE(n_images > 0 && n_images <= 65535, "track_reset: %d images is out of range [1, 65535]", n_images);
  DN_REQUIRE(max_tracks >= 1 && max_tracks <= kMaxM, "track_reset: max_tracks = %d, must be in [1, %d]", max_tracks, kMaxM);
  const size_t per = (kHeaderBytes + (size_t)kRecBytes * max_tracks) / 8, words = per * n_images;
  const unsigned blocks = (unsigned)((words + 255) / 256 < 1024 ? (words + 255) / 256 : 1024);
  hipLaunchKernelGGL(track_reset_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream,
                     static_cast<unsigned long long*>(state), per, words);
  return dn::check_launch("track_reset");
}

extern "C" int dn_track_step(const float* boxes, const float* scores, const int32_t* count, int n_images, int k,
                             int max_tracks, int max_age, int min_hits, double iou_threshold, double scale, void* state,
                             double* out_rect, int32_t* out_id, int32_t* out_det, float* out_score, int32_t* out_count,
                             int32_t* det_track, void* stream) {
  DN_REQUIRE(boxes && scores && count && state && out_rect && out_id && out_det && out_score && out_count && det_track,
             "track_step: null pointer");
  DN_REQUIRE(n_images > 0 && n_images <= 65535, "track_step: %d images is out of range [1, 65535]", n_images);
  DN_REQUIRE(k >= 1 && k <= kMaxK, "track_step: K = %d detection rows, must be in [1, %d]", k, kMaxK);
  DN_REQUIRE(max_tracks >= 1 && max_tracks <= kMaxM, "track_step: max_tracks = %d, must be in [1, %d]", max_tracks, kMaxM);
  DN_REQUIRE(max_age >= 0 && min_hits >= 0, "track_step: max_age = %d, min_hits = %d, both must be >= 0", max_age, min_hits);
  DN_REQUIRE(std::isfinite(iou_threshold) && iou_threshold >= 0, "track_step: iou_threshold = %g, must be finite and >= 0",
             iou_threshold);
  DN_REQUIRE(std::isfinite(scale) && scale > 0, "track_step: scale = %g, must be finite and > 0", scale);
  Params p;
  p.k = k; p.m = max_tracks; p.max_age = max_age; p.min_hits = min_hits;
  p.ld = (k < kMaxD ? k : kMaxD) | 1;
  p.thr = iou_threshold; p.scale = scale;
  const int lds = (int)(sizeof(double) * (size_t)max_tracks * p.ld);
  const int most = (int)(sizeof(double) * (size_t)kMaxM * (kMaxD | 1));
  static dn::PerDeviceFlag lds_flag;
  static int static_lds[64];
  const int fixed = dn::static_lds_of(reinterpret_cast<const void*>(track_step_kernel), lds_flag, static_lds, most);
  if (fixed == -1) return dn::fail(DN_ERR_LAUNCH, "track_step: cannot read the kernel's attributes");
  if (fixed < 0) return dn::fail(DN_ERR_LAUNCH, "track_step: cannot reserve %d B of dynamic LDS", most);
  hipLaunchKernelGGL(track_step_kernel, dim3(n_images), dim3(kThreads), lds, (hipStream_t)stream, boxes, scores, count, p,
                     static_cast<unsigned char*>(state), out_rect, out_id, out_det, out_score, out_count, det_track);
  return dn::check_launch("track_step");
}
