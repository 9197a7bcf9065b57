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
//   detect_iou_mask    one bit per pair i < j of an image: IoU(i, j) > iou_thr, 64x16 tiles, fp64 polygon clip per lane
//   detect_reduce      one wave per image walks the rows in order (the "removed" words live in its lanes) and writes
//                      the kept rows, then zero / -1 padding up to top_k
// Keys are 30-bit (a score is in [0, 1] or NaN), so three 10-bit digits find T.  Only integer atomics are used and
// every ordering is decided by (key, index): the outputs are the same bits on every run.
#include <cmath>

#include "dn_internal.h"
#include "decode_device.h"
#include "rot_iou_device.h"   // Box64, box64, intersection_area: rotated IoU in fp64 (shared with ap_match.hip)

namespace {

constexpr int kThreads = 256;
constexpr int kItems = 16;
constexpr long kChunk = (long)kThreads * kItems;   // anchors per workgroup of the select passes
constexpr int kBins = 1024;                         // 10-bit digits
constexpr int kMaxK = 1024;
using dn::Box64;
using dn::box64;
using dn::intersection_area;
using dn::kClipCap;

struct Layout {
  size_t keys, hist, gcount, state, ties, cand, sbox, sscore, sidx, nvalid, mask, total;
};

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

Layout layout(int n, long apl, int top_k) {
  const long bpi = (apl + kChunk - 1) / kChunk;
  const long nb = (top_k + 63) / 64;
  Layout L;
  size_t o = 0;
  L.keys = o;   o = align256(o + sizeof(unsigned) * (size_t)n * apl);
  L.hist = o;   o += sizeof(unsigned) * (size_t)n * 3 * kBins;          // hist and gcount: one zero fill
  L.gcount = o; o = align256(o + sizeof(unsigned) * (size_t)n);
  L.state = o;  o = align256(o + sizeof(unsigned) * (size_t)n * 8);
  L.ties = o;   o = align256(o + sizeof(unsigned) * (size_t)n * bpi);
  L.cand = o;   o = align256(o + sizeof(unsigned long long) * (size_t)n * top_k);
  L.sbox = o;   o = align256(o + sizeof(float) * 6 * (size_t)n * top_k);
  L.sscore = o; o = align256(o + sizeof(float) * (size_t)n * top_k);
  L.sidx = o;   o = align256(o + sizeof(int) * (size_t)n * top_k);
  L.nvalid = o; o = align256(o + sizeof(int) * (size_t)n);
  L.mask = o;   o = align256(o + sizeof(unsigned long long) * (size_t)n * top_k * nb);
  L.total = o;
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
  __shared__ double cxs[4][kMaskCols], cys[4][kMaskCols], ccx[kMaskCols], ccy[kMaskCols], crad[kMaskCols],
      carea[kMaskCols];
  __shared__ double bufx[2][kClipCap][64], bufy[2][kClipCap][64];
  const int cb = blockIdx.x / 4, q = blockIdx.x % 4, rb = blockIdx.y, img = blockIdx.z, t = threadIdx.x;
  const int nv = nvalid[img];
  if (cb < rb || cb * 64 >= nv) return;
  const int j0 = cb * 64 + q * kMaskCols;
  if (t < kMaskCols && j0 + t < nv) {
    Box64 b;
    box64(sbox + 6 * ((size_t)img * top_k + j0 + t), b);
    for (int k = 0; k < 4; ++k) {
      cxs[k][t] = b.x[k];
      cys[k][t] = b.y[k];
    }
    ccx[t] = b.cx;
    ccy[t] = b.cy;
    crad[t] = b.radius;
    carea[t] = b.area;
  }
  __syncthreads();
  const int i = rb * 64 + t;
  if (i >= nv) return;
  Box64 a;
  box64(sbox + 6 * ((size_t)img * top_k + i), a);
  unsigned bits = 0;
  const int jend = nv - j0 < kMaskCols ? nv - j0 : kMaskCols;
  for (int jj = 0; jj < jend; ++jj) {
    if (j0 + jj <= i) continue;
    const double dist = hypot(ccx[jj] - a.cx, ccy[jj] - a.cy);
    if (!(dist < crad[jj] + a.radius)) continue;   // circumscribed circles apart: IoU 0
    double bx[4], by[4];
    for (int k = 0; k < 4; ++k) {
      bx[k] = cxs[k][jj];
      by[k] = cys[k][jj];
    }
    const double inter = intersection_area(a.x, a.y, bx, by, &bufx[0][0][t], &bufy[0][0][t], &bufx[1][0][t],
                                           &bufy[1][0][t]);
    const double uni = a.area + carea[jj] - inter;
    if (uni > 0 && inter / uni > iou_thr) bits |= 1u << jj;
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
  DN_REQUIRE(n_images > 0 && n_images <= 65535 && anchors_per_image > 0 && anchors_per_image < (1L << 31),
             "detect: %d images of %ld anchors is out of range", n_images, anchors_per_image);
  DN_REQUIRE(top_k >= 1 && top_k <= kMaxK, "detect: top_k = %d, must be in [1, %d]", top_k, kMaxK);
  DN_REQUIRE(std::isfinite(iou_thr) && iou_thr >= 0, "detect: iou_thr = %g, must be finite and >= 0", iou_thr);
  const Layout L = layout(n_images, anchors_per_image, top_k);
  DN_REQUIRE(workspace_bytes >= L.total, "detect: workspace of %zu bytes, %zu needed (dn_detect_workspace_bytes)",
             workspace_bytes, L.total);
  const long apl = anchors_per_image;
  const int nb = (top_k + 63) / 64;
  const size_t reduce_lds = sizeof(unsigned long long) * (size_t)kMaxK * ((kMaxK + 63) / 64);
  static dn::PerDeviceFlag lds_flag;
  bool& lds_ready = lds_flag.here();
  if (!lds_ready) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(detect_reduce_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)reduce_lds);
    if (e != hipSuccess)
      return dn::fail(DN_ERR_LAUNCH, "detect: hipFuncSetAttribute(%zu B LDS): %s", reduce_lds, hipGetErrorString(e));
    lds_ready = true;
  }
  hipStream_t s = (hipStream_t)stream;
  char* ws = static_cast<char*>(workspace);
  unsigned* keys = reinterpret_cast<unsigned*>(ws + L.keys);
  unsigned* hist = reinterpret_cast<unsigned*>(ws + L.hist);
  unsigned* gcount = reinterpret_cast<unsigned*>(ws + L.gcount);
  unsigned* state = reinterpret_cast<unsigned*>(ws + L.state);
  unsigned* ties = reinterpret_cast<unsigned*>(ws + L.ties);
  unsigned long long* cand = reinterpret_cast<unsigned long long*>(ws + L.cand);
  float* sbox = reinterpret_cast<float*>(ws + L.sbox);
  float* sscore = reinterpret_cast<float*>(ws + L.sscore);
  int* sidx = reinterpret_cast<int*>(ws + L.sidx);
  int* nvalid = reinterpret_cast<int*>(ws + L.nvalid);
  unsigned long long* mask = reinterpret_cast<unsigned long long*>(ws + L.mask);

  if (dn::zero_fill(hist, L.gcount + sizeof(unsigned) * n_images - L.hist, s) != hipSuccess)
    return dn::fail(DN_ERR_LAUNCH, "detect: zero fill of the histograms failed");
  const dim3 grid((unsigned)((apl + kChunk - 1) / kChunk), (unsigned)n_images);
  hipLaunchKernelGGL(detect_score_kernel, grid, dim3(kThreads), 0, s, cls, apl, use_score_thr, score_thr, keys, hist);
  for (int pass = 1; pass <= 3; ++pass)
    hipLaunchKernelGGL(detect_radix_kernel, grid, dim3(kThreads), 0, s, keys, apl, top_k, pass, hist, state, ties);
  hipLaunchKernelGGL(detect_gather_kernel, grid, dim3(kThreads), 0, s, keys, apl, top_k, state, ties, gcount, cand);
  hipLaunchKernelGGL(detect_sort_kernel, dim3(n_images), dim3(kSortThreads), 0, s, cls, loc, anchors, apl, top_k, cand,
                     sbox, sscore, sidx, nvalid);
  hipLaunchKernelGGL(detect_iou_mask_kernel, dim3(4 * nb, nb, n_images), dim3(64), 0, s, sbox, nvalid, top_k, nb, iou_thr,
                     mask);
  hipLaunchKernelGGL(detect_reduce_kernel, dim3(n_images), dim3(kThreads),
                     sizeof(unsigned long long) * (size_t)top_k * nb, s, sbox, sscore, sidx, nvalid, mask, top_k, nb,
                     boxes, scores, index, count);
  return dn::check_launch("detect");
}
