// Detection tail on the GPU: per image, the top-k anchors by foreground score (score descending, anchor index
// ascending -- torch.sort(stable=True)), their decoded boxes, greedy rotated NMS in that order and the kept rows padded to
// top_k.  Exactly the tail of postprocess.host_detections for finite logits; the one documented difference: a NaN score
// is never a candidate (the host path lets it take a top-k slot and drops it afterwards).
//
// Launch sequence (fixed: it depends on the shapes only, never on the data; nothing is read back):
//   zero_fill          the radix histograms and the gather counters
//   detect_score       key of every anchor (score bits + 1, 0 = not a candidate) and the histogram of its top digit
//   detect_radix x3    passes 1-2: the k-th key's next digit, histogram of the following one among the keys that share
//                      the prefix; pass 3: the k-th key T itself and every workgroup's count of keys equal to T
//   detect_gather      keys > T (at most k - 1 of them, any order) and the first `need` keys == T in anchor order: the
//                      per-workgroup tie counts are scanned, so the lowest indices win whatever the schedule
//   detect_sort        the k survivors of one image sorted in LDS by (key desc, index asc), decoded with
//                      decode_device.h (bit for bit dn_decode_boxes), non-candidates (key 0) dropped from the tail
//   detect_iou_mask    one bit per pair i < j of an image: IoU(i, j) > iou_thr, 64x16 tiles; columns, circle test and
//                      IoU are rot_iou_device.h's (stage_columns, circles_meet, pair_iou), shared with the matching kernels
//   detect_reduce      one wave per image walks the rows in order (the "removed" words live in its lanes) and writes
//                      the kept rows, then zero / -1 padding up to top_k
// Keys are 30-bit (a score is in [0, 1] or NaN), so three 10-bit digits find T.  Only integer atomics are used and
// every ordering is decided by (key, index): the outputs are the same bits on every run.
//
// Late fusion (dn_late_fuse, `--com late`) sits behind dn_detect and ends in the same two kernels: per served ego image
//   late_gather_sort   one workgroup: the rows of the ego's list (own rows, then every listed neighbour's carried into the
//                      ego's frame in fp64), 64-bit sort words (score key | inverted list slot) sorted in LDS, the first
//                      top_k rows written where detect_sort writes its own
//   detect_iou_mask, detect_reduce   as above, on those rows; `index` is then the row's source, agent * k_in + row
// Both entry points hand the sorted rows to one tail (NmsLayout, launch_nms): the carve, the casts and the two launches.
#include <cmath>

#include "dn_internal.h"
#include "decode_device.h"
#include "ego_list.h"
#include "rot_iou_device.h"

namespace {

constexpr int kThreads = 256;
constexpr int kItems = 16;
constexpr long kChunk = (long)kThreads * kItems;   // anchors per workgroup of the select passes
constexpr int kBins = 1024;                         // 10-bit digits
constexpr int kMaxK = dn::kMaxBoxRows;

// The NMS tail's part of a workspace: the sorted rows of every image (detect_sort or late_gather_sort writes them),
// the number of them that are valid, and the pair mask.
struct NmsLayout {
  size_t sbox, sscore, sidx, nvalid, mask;
};

NmsLayout nms_layout(dn::Carver& c, int n, int top_k) {
  const size_t rows = (size_t)n * top_k, nb = (top_k + 63) / 64;
  NmsLayout L;
  L.sbox = c.take(sizeof(float) * 6 * rows);
  L.sscore = c.take(sizeof(float) * rows);
  L.sidx = c.take(sizeof(int) * rows);
  L.nvalid = c.take(sizeof(int) * (size_t)n);
  L.mask = c.take(sizeof(unsigned long long) * rows * nb);
  return L;
}

struct NmsArrays {
  float *sbox, *sscore;
  int *sidx, *nvalid;
  unsigned long long* mask;
};

NmsArrays nms_arrays(const NmsLayout& L, char* ws) {
  return {reinterpret_cast<float*>(ws + L.sbox), reinterpret_cast<float*>(ws + L.sscore),
          reinterpret_cast<int*>(ws + L.sidx), reinterpret_cast<int*>(ws + L.nvalid),
          reinterpret_cast<unsigned long long*>(ws + L.mask)};
}

struct Layout {
  size_t keys, hist, gcount, state, ties, cand;
  NmsLayout nms;
  size_t total;
};

Layout layout(int n, long apl, int top_k) {
  const long bpi = (apl + kChunk - 1) / kChunk;
  const size_t hist_bytes = sizeof(unsigned) * (size_t)n * 3 * kBins;
  dn::Carver c;
  Layout L;
  L.keys = c.take(sizeof(unsigned) * (size_t)n * apl);
  L.hist = c.take(hist_bytes + sizeof(unsigned) * (size_t)n);            // hist and gcount: one region, one zero fill
  L.gcount = L.hist + hist_bytes;
  L.state = c.take(sizeof(unsigned) * (size_t)n * 8);
  L.ties = c.take(sizeof(unsigned) * (size_t)n * bpi);
  L.cand = c.take(sizeof(unsigned long long) * (size_t)n * top_k);
  L.nms = nms_layout(c, n, top_k);
  L.total = c.at;
  return L;
}

// 0 = not a candidate (filtered out or NaN); otherwise the score's bits + 1: non-negative floats order like their bits
__device__ __forceinline__ unsigned score_key(float s, int use_thr, float thr) {
  const bool cand = use_thr ? (s > thr) : (s >= 0.f);
  return cand ? (__float_as_uint(s) & 0x7fffffffu) + 1u : 0u;
}

__device__ __forceinline__ unsigned long long sort_word(unsigned key, unsigned anchor) {
  return ((unsigned long long)key << 32) | (unsigned long long)(0xffffffffu - anchor);
}

// exclusive prefix of one value per thread in thread order over the 256-thread block; `total` = the block's sum
__device__ unsigned block_exclusive_scan(unsigned v, unsigned* wave_sums, unsigned& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned x = v;
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned y = __shfl_up(x, d, 64);
    if (lane >= d) x += y;
  }
  if (lane == 63) wave_sums[wave] = x;
  __syncthreads();
  unsigned before = 0;
  total = 0;
  for (int w = 0; w < kThreads / 64; ++w) {
    const unsigned t = wave_sums[w];
    if (w < wave) before += t;
    total += t;
  }
  __syncthreads();
  return before + x - v;
}

// The bin of `hist` (counting from the top) that holds the k-th largest key, and k's rank inside that bin.
__device__ void select_bin(const unsigned* __restrict__ hist, unsigned k, unsigned* wave_sums, unsigned* sel) {
  const int t = threadIdx.x;
  unsigned c[4], s = 0;
  for (int q = 0; q < 4; ++q) {
    c[q] = hist[kBins - 1 - 4 * t - q];
    s += c[q];
  }
  if (t == 0) {
    sel[0] = 0;
    sel[1] = 1;
  }
  unsigned total;
  unsigned above = block_exclusive_scan(s, wave_sums, total);
  if (above < k && k <= above + s) {
    for (int q = 0; q < 4; ++q) {
      if (k <= above + c[q]) {
        sel[0] = kBins - 1 - 4 * t - q;
        sel[1] = k - above;
        break;
      }
      above += c[q];
    }
  }
  __syncthreads();
}

__global__ void __launch_bounds__(kThreads) detect_score_kernel(const float* __restrict__ cls, long apl, int use_thr,
                                                                float thr, unsigned* __restrict__ keys,
                                                                unsigned* __restrict__ hist) {
  __shared__ unsigned h[kBins];
  const int img = blockIdx.y;
  for (int b = threadIdx.x; b < kBins; b += kThreads) h[b] = 0;
  __syncthreads();
  const long base = blockIdx.x * kChunk;
  for (int it = 0; it < kItems; ++it) {
    const long a = base + it * kThreads + threadIdx.x;
    if (a < apl) {
      const long g = (long)img * apl + a;
      const unsigned key = score_key(dn::fg_score(cls, g), use_thr, thr);
      keys[g] = key;
      atomicAdd(&h[key >> 20], 1u);
    }
  }
  __syncthreads();
  unsigned* gh = hist + (size_t)img * 3 * kBins;
  for (int b = threadIdx.x; b < kBins; b += kThreads)
    if (h[b]) atomicAdd(&gh[b], h[b]);
}

// pass 1, 2: digit `pass - 1` of the k-th key from the previous histogram, then the histogram of digit `pass` among the
// keys that share the prefix found so far.  pass 3: the k-th key T and this workgroup's count of keys equal to T.
// Workgroup 0 of each pass records (prefix, rank in the prefix's bucket) for the next launch.
__global__ void __launch_bounds__(kThreads) detect_radix_kernel(const unsigned* __restrict__ keys, long apl, int top_k,
                                                                int pass, unsigned* __restrict__ hist,
                                                                unsigned* __restrict__ state,
                                                                unsigned* __restrict__ ties) {
  __shared__ unsigned h[kBins];
  __shared__ unsigned wave_sums[kThreads / 64];
  __shared__ unsigned sel[2];
  const int img = blockIdx.y;
  unsigned* gh = hist + (size_t)img * 3 * kBins;
  unsigned* st = state + (size_t)img * 8;
  const unsigned kk = (unsigned)(apl < top_k ? apl : top_k);
  const unsigned prev = pass == 1 ? 0u : st[2 * (pass - 1)];
  const unsigned k = pass == 1 ? kk : st[2 * (pass - 1) + 1];
  select_bin(gh + (size_t)(pass - 1) * kBins, k, wave_sums, sel);
  const unsigned prefix = (prev << 10) | sel[0];
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    st[2 * pass] = prefix;
    st[2 * pass + 1] = sel[1];
  }
  const long base = blockIdx.x * kChunk;
  const unsigned* kp = keys + (size_t)img * apl;
  if (pass == 3) {
    unsigned n = 0;
    for (int it = 0; it < kItems; ++it) {
      const long a = base + it * kThreads + threadIdx.x;
      if (a < apl && kp[a] == prefix) ++n;
    }
    unsigned total;
    (void)block_exclusive_scan(n, wave_sums, total);
    if (threadIdx.x == 0) ties[(size_t)img * gridDim.x + blockIdx.x] = total;
    return;
  }
  for (int b = threadIdx.x; b < kBins; b += kThreads) h[b] = 0;
  __syncthreads();
  const int shift = pass == 1 ? 20 : 10;
  for (int it = 0; it < kItems; ++it) {
    const long a = base + it * kThreads + threadIdx.x;
    if (a < apl) {
      const unsigned key = kp[a];
      if ((key >> shift) == prefix) atomicAdd(&h[(key >> (shift - 10)) & (kBins - 1)], 1u);
    }
  }
  __syncthreads();
  for (int b = threadIdx.x; b < kBins; b += kThreads)
    if (h[b]) atomicAdd(&gh[(size_t)pass * kBins + b], h[b]);
}

__global__ void __launch_bounds__(kThreads) detect_gather_kernel(const unsigned* __restrict__ keys, long apl, int top_k,
                                                                 const unsigned* __restrict__ state,
                                                                 const unsigned* __restrict__ ties,
                                                                 unsigned* __restrict__ gcount,
                                                                 unsigned long long* __restrict__ cand) {
  __shared__ unsigned wave_sums[kThreads / 64];
  const int img = blockIdx.y;
  const unsigned kk = (unsigned)(apl < top_k ? apl : top_k);
  const unsigned T = state[(size_t)img * 8 + 6];
  const unsigned need = state[(size_t)img * 8 + 7] < kk ? state[(size_t)img * 8 + 7] : kk;
  const unsigned greater = kk - need;
  unsigned part = 0, running;
  for (unsigned b = threadIdx.x; b < blockIdx.x; b += kThreads) part += ties[(size_t)img * gridDim.x + b];
  (void)block_exclusive_scan(part, wave_sums, running);   // ties in the workgroups before this one
  unsigned long long* out = cand + (size_t)img * top_k;
  const unsigned* kp = keys + (size_t)img * apl;
  const long base = blockIdx.x * kChunk;
  for (int it = 0; it < kItems; ++it) {
    const long a = base + it * kThreads + threadIdx.x;
    const unsigned key = a < apl ? kp[a] : 0u;
    if (a < apl && key > T) {
      const unsigned pos = atomicAdd(&gcount[img], 1u);   // slot order is free: detect_sort orders by (key, index)
      if (pos < greater) out[pos] = sort_word(key, (unsigned)a);
    }
    const bool tie = a < apl && key == T;
    unsigned n;
    const unsigned r = running + block_exclusive_scan(tie ? 1u : 0u, wave_sums, n);
    if (tie && r < need) out[greater + r] = sort_word(key, (unsigned)a);
    running += n;
  }
}

// One workgroup per image: sort the kk survivors, drop non-candidates, decode the rest.
constexpr int kSortThreads = 512;
__global__ void __launch_bounds__(kSortThreads) detect_sort_kernel(const float* __restrict__ cls,
                                                                   const float* __restrict__ loc,
                                                                   const float* __restrict__ anchors, long apl,
                                                                   int top_k,
                                                                   const unsigned long long* __restrict__ cand,
                                                                   float* __restrict__ sbox, float* __restrict__ sscore,
                                                                   int* __restrict__ sidx, int* __restrict__ nvalid) {
  __shared__ unsigned long long s[kMaxK];
  __shared__ int nv;
  const int img = blockIdx.x;
  const int kk = (int)(apl < top_k ? apl : top_k);
  int p = 1;
  while (p < kk) p <<= 1;
  if (threadIdx.x == 0) nv = 0;
  for (int i = threadIdx.x; i < p; i += kSortThreads) s[i] = i < kk ? cand[(size_t)img * top_k + i] : 0ull;
  __syncthreads();
  for (int size = 2; size <= p; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int i = threadIdx.x; i < p / 2; i += kSortThreads) {
        const int lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
        const bool desc = (lo & size) == 0;
        const unsigned long long x = s[lo], y = s[hi];
        if ((x < y) == desc) {
          s[lo] = y;
          s[hi] = x;
        }
      }
      __syncthreads();
    }
  }
  for (int i = threadIdx.x; i < kk; i += kSortThreads) {
    const unsigned key = (unsigned)(s[i] >> 32);
    if (key != 0 && (i + 1 == kk || (unsigned)(s[i + 1] >> 32) == 0)) nv = i + 1;
    const unsigned a = 0xffffffffu - (unsigned)s[i];
    if (key == 0 || a >= apl) continue;
    const size_t row = (size_t)img * top_k + i;
    float b[6];
    sscore[row] = dn::decode_anchor(cls, loc, anchors, (long)img * apl + a, apl, b);
    for (int q = 0; q < 6; ++q) sbox[6 * row + q] = b[q];
    sidx[row] = (int)a;
  }
  __syncthreads();
  if (threadIdx.x == 0) nvalid[img] = nv;
}

// Tile (row block, 16-column piece) of one image: lane t is row i = 64 * rb + t; bit jj of its 16-bit piece q of mask
// word cb is IoU(i, j = 64 * cb + 16 * q + jj) > iou_thr for i < j < nvalid.  Four pieces per word keep four times as
// many waves busy as whole 64-column tiles would (each lane clips its pairs one after another).
constexpr int kMaskCols = 16;
__global__ void __launch_bounds__(64) detect_iou_mask_kernel(const float* __restrict__ sbox,
                                                             const int* __restrict__ nvalid, int top_k, int nb,
                                                             double iou_thr,
                                                             unsigned long long* __restrict__ mask) {
#pragma clang fp contract(off)
  __shared__ dn::BoxColumns<kMaskCols> cols;
  __shared__ dn::ClipScratch scratch;
  const int cb = blockIdx.x / 4, q = blockIdx.x % 4, rb = blockIdx.y, img = blockIdx.z, t = threadIdx.x;
  const int nv = nvalid[img];
  if (cb < rb || cb * 64 >= nv) return;
  const int j0 = cb * 64 + q * kMaskCols;
  const int jend = nv - j0 < kMaskCols ? nv - j0 : kMaskCols;   // <= 0: the piece lies behind the last valid row
  dn::stage_columns(cols, sbox + 6 * ((size_t)img * top_k + j0), jend, t);
  __syncthreads();
  const int i = rb * 64 + t;
  if (i >= nv) return;
  dn::Box64 a;
  dn::box64(sbox + 6 * ((size_t)img * top_k + i), a);
  unsigned bits = 0;
  for (int jj = 0; jj < jend; ++jj) {
    if (j0 + jj <= i) continue;
    if (!dn::circles_meet(cols, jj, a)) continue;   // circumscribed circles apart: IoU 0
    if (dn::pair_iou(cols, jj, a, scratch, t) > iou_thr) bits |= 1u << jj;   // iou_thr >= 0: an IoU of 0 never sets a bit
  }
  reinterpret_cast<unsigned short*>(mask + ((size_t)img * top_k + i) * nb + cb)[q] = (unsigned short)bits;
}

// One workgroup per image: the mask rows into LDS, wave 0 walks them in order, then every thread writes output rows.
__global__ void __launch_bounds__(kThreads) detect_reduce_kernel(const float* __restrict__ sbox,
                                                                 const float* __restrict__ sscore,
                                                                 const int* __restrict__ sidx,
                                                                 const int* __restrict__ nvalid,
                                                                 const unsigned long long* __restrict__ mask, int top_k,
                                                                 int nb, float* __restrict__ boxes,
                                                                 float* __restrict__ scores, int* __restrict__ index,
                                                                 int* __restrict__ count) {
  extern __shared__ unsigned long long lm[];   // [nvalid][nb]
  __shared__ int keep[kMaxK];
  __shared__ int kept_n;
  const int img = blockIdx.x;
  const int nv = nvalid[img];
  const int nw = (nv + 63) / 64;
  const unsigned long long* gm = mask + (size_t)img * top_k * nb;
  // words left of the diagonal and right of the last valid column were never written: they read as 0
  for (int e = threadIdx.x; e < nv * nb; e += kThreads) {
    const int row = e / nb, w = e - row * nb;
    lm[e] = (w >= row / 64 && w < nw) ? gm[e] : 0ull;
  }
  __syncthreads();
  if (threadIdx.x < 64) {
    const int lane = threadIdx.x;
    unsigned long long removed = 0;   // lane l: word l of the "removed" set
    int n = 0;
    for (int w = 0; w < nw; ++w) {
      unsigned long long r = __shfl(removed, w, 64);
      const int row = w * 64 + lane;
      const unsigned long long diag = row < nv ? lm[(size_t)row * nb + w] : 0ull;
      const int left = nv - w * 64;
      const unsigned long long valid = left >= 64 ? ~0ull : ((1ull << left) - 1);
      unsigned long long kept = 0, todo = ~r & valid;
      while (todo) {
        const int b = __ffsll((long long)todo) - 1;
        kept |= 1ull << b;
        r |= __shfl(diag, b, 64);
        todo = ~r & valid & ~((2ull << b) - 1);
      }
      if (lane > w && lane < nw) {
        unsigned long long acc = 0, bits = kept;
        while (bits) {
          const int b = __ffsll((long long)bits) - 1;
          bits &= bits - 1;
          acc |= lm[(size_t)(w * 64 + b) * nb + lane];
        }
        removed |= acc;
      }
      if ((kept >> lane) & 1) keep[n + __popcll(kept & ((1ull << lane) - 1))] = row;
      n += __popcll(kept);
    }
    if (lane == 0) kept_n = n;
  }
  __syncthreads();
  const int n = kept_n;
  for (int r = threadIdx.x; r < top_k; r += kThreads) {
    const size_t o = (size_t)img * top_k + r;
    if (r < n) {
      const size_t src = (size_t)img * top_k + keep[r];
      for (int q = 0; q < 6; ++q) boxes[6 * o + q] = sbox[6 * src + q];
      scores[o] = sscore[src];
      index[o] = sidx[src];
    } else {
      for (int q = 0; q < 6; ++q) boxes[6 * o + q] = 0.f;
      scores[o] = 0.f;
      index[o] = -1;
    }
  }
  if (threadIdx.x == 0) count[img] = n;
}

// The NMS tail of dn_detect and dn_late_fuse on the sorted rows of n images.  detect_reduce's dynamic LDS (the mask rows
// of one image, up to 128 KB) is reserved once per device, by whichever entry point runs first.
int launch_nms(const char* who, const NmsLayout& L, char* ws, int n, int top_k, double iou_thr, float* boxes,
               float* scores, int* index, int* count, hipStream_t s) {
  static dn::PerDeviceFlag lds_flag;
  if (const int rc = dn::reserve_dynamic_lds(reinterpret_cast<const void*>(detect_reduce_kernel), lds_flag,
                                             sizeof(unsigned long long) * (size_t)kMaxK * ((kMaxK + 63) / 64), who))
    return rc;
  const NmsArrays a = nms_arrays(L, ws);
  const int nb = (top_k + 63) / 64;
  hipLaunchKernelGGL(detect_iou_mask_kernel, dim3(4 * nb, nb, n), dim3(64), 0, s, a.sbox, a.nvalid, top_k, nb, iou_thr,
                     a.mask);
  hipLaunchKernelGGL(detect_reduce_kernel, dim3(n), dim3(kThreads), sizeof(unsigned long long) * (size_t)top_k * nb, s,
                     a.sbox, a.sscore, a.sidx, a.nvalid, a.mask, top_k, nb, boxes, scores, index, count);
  return dn::check_launch(who);
}

// ---- late fusion ----------------------------------------------------------------------------------------------------
constexpr int kLateMaxAgents = 16;
constexpr int kLateMaxSlots = 8192;      // agents * k_in: 64 KB of sort words in LDS
constexpr int kLateThreads = 512;

bool late_shape_ok(int batch, int agents, int k_in, int top_k, int ego_first, int ego_count) {
  return batch > 0 && agents > 0 && agents <= kLateMaxAgents && k_in >= 1 && k_in <= kMaxK &&
         agents * k_in <= kLateMaxSlots && top_k >= 1 && top_k <= kMaxK && ego_first >= 0 && ego_count > 0 &&
         ego_first + ego_count <= agents && (long)batch * ego_count <= dn::kMaxImages;
}

struct LateExtents {
  double xlo, xhi, ylo, yhi;
  int use;
};

// A neighbour's row (x, y, w, h, sin, cos) under M = trans[b][i][j] (row-major 4 x 4, fp32), in fp64: every product and
// every sum rounded on its own, each result rounded once to fp32 (dn_voxelize_views' discipline; a product of two fp32
// values is exact in fp64, so only the order of the additions counts).  w and h are copied, the heading is not renormalised.
__device__ inline void carry_row(const float* __restrict__ row, const float* __restrict__ M, float* out) {
#pragma clang fp contract(off)
  const double m00 = M[0], m01 = M[1], m03 = M[3], m10 = M[4], m11 = M[5], m13 = M[7];
  const double x = row[0], y = row[1], sn = row[4], cs = row[5];
  out[0] = (float)((m00 * x + m01 * y) + m03);
  out[1] = (float)((m10 * x + m11 * y) + m13);
  out[2] = row[2];
  out[3] = row[3];
  out[4] = (float)(m10 * cs + m11 * sn);
  out[5] = (float)(m00 * cs + m01 * sn);
}

// One workgroup per served ego image (i, b).  list[0] = i, then the listed neighbours ascending; slot = position * k_in +
// row.  A slot is a candidate when its row is below its agent's clamped count, its score is finite and >= 0 (-0 counts,
// and its key is +0's) and, for a neighbour's row under use_extents, the carried centre is strictly inside the extents.
__global__ void __launch_bounds__(kLateThreads) late_gather_sort_kernel(
    const float* __restrict__ boxes, const float* __restrict__ scores, const int* __restrict__ count,
    const float* __restrict__ trans, const int* __restrict__ num_agent, int batch, int agents, int k_in, int only_v2i,
    int ego_first, int top_k, LateExtents ext, float* __restrict__ sbox, float* __restrict__ sscore,
    int* __restrict__ sidx, int* __restrict__ nvalid) {
  extern __shared__ unsigned long long sw[];   // [p]: p = the power of two that holds the list's slots
  __shared__ int list[kLateMaxAgents], cnt[kLateMaxAgents];
  __shared__ int len_s, nv;
  const int img = blockIdx.x;                  // (i - ego_first) * batch + b
  const int b = img % batch, i = ego_first + img / batch;
  if (threadIdx.x == 0) {
    const int n = live_count(num_agent, b, agents);
    int len = 0;
    list[len++] = i;
    if (i < n)
      for (int j = 0; j < n; ++j)
        if (DN_LISTED_LIVE(i, j, only_v2i)) list[len++] = j;
    for (int p = 0; p < len; ++p) {
      const int c = count[list[p] * batch + b];
      cnt[p] = c < 0 ? 0 : (c > k_in ? k_in : c);
    }
    len_s = len;
    nv = 0;
  }
  __syncthreads();
  const int len = len_s;
  const int slots = len * k_in;
  int p = 1;
  while (p < slots) p <<= 1;
  for (int e = threadIdx.x; e < p; e += kLateThreads) {
    unsigned long long word = 0ull;
    if (e < slots) {
      const int pos = e / k_in, r = e - pos * k_in;
      if (r < cnt[pos]) {
        const int j = list[pos];
        const size_t row = ((size_t)j * batch + b) * k_in + r;
        const float s = scores[row];
        bool cand = s >= 0.f && s < INFINITY;            // a NaN fails both
        if (cand && pos > 0 && ext.use) {
          float t[6];
          carry_row(boxes + 6 * row, trans + (((size_t)b * agents + i) * agents + j) * 16, t);
          const double x = (double)t[0], y = (double)t[1];
          cand = ext.xlo < x && x < ext.xhi && ext.ylo < y && y < ext.yhi;
        }
        if (cand) word = sort_word((__float_as_uint(s) & 0x7fffffffu) + 1u, (unsigned)e);
      }
    }
    sw[e] = word;
  }
  __syncthreads();
  for (int size = 2; size <= p; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int t = threadIdx.x; t < p / 2; t += kLateThreads) {
        const int lo = 2 * t - (t & (stride - 1)), hi = lo + stride;
        const bool desc = (lo & size) == 0;
        const unsigned long long x = sw[lo], y = sw[hi];
        if ((x < y) == desc) {
          sw[lo] = y;
          sw[hi] = x;
        }
      }
      __syncthreads();
    }
  }
  const int lim = top_k < p ? top_k : p;
  for (int q = threadIdx.x; q < lim; q += kLateThreads) {
    const unsigned long long word = sw[q];
    if (word == 0ull) continue;
    if (q + 1 == lim || sw[q + 1] == 0ull) nv = q + 1;
    const int e = (int)(0xffffffffu - (unsigned)word);
    const int pos = e / k_in, r = e - pos * k_in;
    const int j = list[pos];
    const size_t row = ((size_t)j * batch + b) * k_in + r;
    const size_t o = (size_t)img * top_k + q;
    float t[6];
    if (pos == 0) {
      for (int c = 0; c < 6; ++c) t[c] = boxes[6 * row + c];
    } else {
      carry_row(boxes + 6 * row, trans + (((size_t)b * agents + i) * agents + j) * 16, t);
    }
    for (int c = 0; c < 6; ++c) sbox[6 * o + c] = t[c];
    sscore[o] = scores[row];
    sidx[o] = j * k_in + r;
  }
  __syncthreads();
  if (threadIdx.x == 0) nvalid[img] = nv;
}

}  // namespace

extern "C" size_t dn_detect_workspace_bytes(int n_images, long anchors_per_image, int top_k) {
  if (n_images <= 0 || anchors_per_image <= 0 || top_k < 1 || top_k > kMaxK) return 0;
  return layout(n_images, anchors_per_image, top_k).total;
}

extern "C" int dn_detect(const float* cls, const float* loc, const float* anchors, int n_images,
                         long anchors_per_image, int top_k, int use_score_thr, float score_thr, double iou_thr,
                         float* boxes, float* scores, int* index, int* count, void* workspace,
                         size_t workspace_bytes, void* stream) {
  DN_REQUIRE(cls && loc && anchors && boxes && scores && index && count && workspace, "detect: null pointer");
  DN_REQUIRE(n_images > 0 && n_images <= dn::kMaxImages && anchors_per_image > 0 && anchors_per_image < (1L << 31),
             "detect: %d images of %ld anchors is out of range", n_images, anchors_per_image);
  DN_REQUIRE(top_k >= 1 && top_k <= kMaxK, "detect: top_k = %d, must be in [1, %d]", top_k, kMaxK);
  DN_REQUIRE(std::isfinite(iou_thr) && iou_thr >= 0, "detect: iou_thr = %g, must be finite and >= 0", iou_thr);
  const Layout L = layout(n_images, anchors_per_image, top_k);
  DN_REQUIRE(workspace_bytes >= L.total, "detect: workspace of %zu bytes, %zu needed (dn_detect_workspace_bytes)",
             workspace_bytes, L.total);
  const long apl = anchors_per_image;
  hipStream_t s = (hipStream_t)stream;
  char* ws = static_cast<char*>(workspace);
  unsigned* keys = reinterpret_cast<unsigned*>(ws + L.keys);
  unsigned* hist = reinterpret_cast<unsigned*>(ws + L.hist);
  unsigned* gcount = reinterpret_cast<unsigned*>(ws + L.gcount);
  unsigned* state = reinterpret_cast<unsigned*>(ws + L.state);
  unsigned* ties = reinterpret_cast<unsigned*>(ws + L.ties);
  unsigned long long* cand = reinterpret_cast<unsigned long long*>(ws + L.cand);
  const NmsArrays a = nms_arrays(L.nms, ws);

  if (dn::zero_fill(hist, L.gcount + sizeof(unsigned) * n_images - L.hist, s) != hipSuccess)
    return dn::fail(DN_ERR_LAUNCH, "detect: zero fill of the histograms failed");
  const dim3 grid((unsigned)((apl + kChunk - 1) / kChunk), (unsigned)n_images);
  hipLaunchKernelGGL(detect_score_kernel, grid, dim3(kThreads), 0, s, cls, apl, use_score_thr, score_thr, keys, hist);
  for (int pass = 1; pass <= 3; ++pass)
    hipLaunchKernelGGL(detect_radix_kernel, grid, dim3(kThreads), 0, s, keys, apl, top_k, pass, hist, state, ties);
  hipLaunchKernelGGL(detect_gather_kernel, grid, dim3(kThreads), 0, s, keys, apl, top_k, state, ties, gcount, cand);
  hipLaunchKernelGGL(detect_sort_kernel, dim3(n_images), dim3(kSortThreads), 0, s, cls, loc, anchors, apl, top_k, cand,
                     a.sbox, a.sscore, a.sidx, a.nvalid);
  return launch_nms("detect", L.nms, ws, n_images, top_k, iou_thr, boxes, scores, index, count, s);
}

extern "C" size_t dn_late_fuse_workspace_bytes(int batch, int agents, int k_in, int top_k, int ego_first, int ego_count) {
  if (!late_shape_ok(batch, agents, k_in, top_k, ego_first, ego_count)) return 0;
  dn::Carver c;
  (void)nms_layout(c, batch * ego_count, top_k);
  return c.at;
}

extern "C" int dn_late_fuse(const float* boxes, const float* scores, const int32_t* count, const float* trans,
                            const int32_t* num_agent, int batch, int agents, int k_in, int only_v2i, int ego_first,
                            int ego_count, int top_k, double iou_thr, int use_extents, const double* xy_extents_host,
                            float* out_boxes, float* out_scores, int32_t* out_source, int32_t* out_count,
                            void* workspace, size_t workspace_bytes, void* stream) {
  DN_REQUIRE(batch > 0 && agents > 0 && agents <= kLateMaxAgents, "late fuse: batch = %d, agents = %d, must be >= 1 and at most %d agents",
             batch, agents, kLateMaxAgents);
  DN_REQUIRE(k_in >= 1 && k_in <= kMaxK, "late fuse: k_in = %d, must be in [1, %d]", k_in, kMaxK);
  DN_REQUIRE(agents * k_in <= kLateMaxSlots, "late fuse: agents * k_in = %d rows in one list, at most %d", agents * k_in,
             kLateMaxSlots);
  DN_REQUIRE(top_k >= 1 && top_k <= kMaxK, "late fuse: top_k = %d, must be in [1, %d]", top_k, kMaxK);
  DN_REQUIRE(std::isfinite(iou_thr) && iou_thr >= 0, "late fuse: iou_thr = %g, must be finite and >= 0", iou_thr);
  DN_REQUIRE(ego_first >= 0 && ego_count > 0 && ego_first + ego_count <= agents,
             "late fuse: ego range [%d, %d) outside 0..%d", ego_first, ego_first + ego_count, agents);
  DN_REQUIRE((long)batch * ego_count <= dn::kMaxImages, "late fuse: %ld output images, at most 65535", (long)batch * ego_count);
  // (the shapes first: a refused shape may come with empty, null outputs)
  DN_REQUIRE(boxes && scores && count && trans && num_agent && out_boxes && out_scores && out_source && out_count &&
                 workspace, "late fuse: null pointer");
  LateExtents ext = {0.0, 0.0, 0.0, 0.0, use_extents ? 1 : 0};
  if (use_extents) {
    DN_REQUIRE(xy_extents_host, "late fuse: use_extents without xy_extents");
    ext.xlo = xy_extents_host[0];
    ext.xhi = xy_extents_host[1];
    ext.ylo = xy_extents_host[2];
    ext.yhi = xy_extents_host[3];
    DN_REQUIRE(ext.xlo < ext.xhi && ext.ylo < ext.yhi, "late fuse: extents (%g, %g) x (%g, %g) are empty or not numbers",
               ext.xlo, ext.xhi, ext.ylo, ext.yhi);
  }
  const int n = batch * ego_count;
  dn::Carver carve;
  const NmsLayout L = nms_layout(carve, n, top_k);
  DN_REQUIRE(workspace_bytes >= carve.at, "late fuse: workspace of %zu bytes, %zu needed (dn_late_fuse_workspace_bytes)",
             workspace_bytes, carve.at);
  static dn::PerDeviceFlag sort_flag;
  if (const int rc = dn::reserve_dynamic_lds(reinterpret_cast<const void*>(late_gather_sort_kernel), sort_flag,
                                             sizeof(unsigned long long) * (size_t)kLateMaxSlots, "late fuse"))
    return rc;
  hipStream_t s = (hipStream_t)stream;
  char* ws = static_cast<char*>(workspace);
  const NmsArrays a = nms_arrays(L, ws);
  int p = 1;                                   // the launch depends on the shapes only: LDS for the longest possible list
  while (p < agents * k_in) p <<= 1;
  hipLaunchKernelGGL(late_gather_sort_kernel, dim3(n), dim3(kLateThreads), sizeof(unsigned long long) * (size_t)p, s,
                     boxes, scores, count, trans, num_agent, batch, agents, k_in, only_v2i, ego_first, top_k, ext, a.sbox,
                     a.sscore, a.sidx, a.nvalid);
  return launch_nms("late fuse", L, ws, n, top_k, iou_thr, out_boxes, out_scores, out_source, out_count, s);
}
