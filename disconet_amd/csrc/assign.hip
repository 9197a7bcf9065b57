// Training targets from ground-truth boxes: every anchor of every image is matched to its best ground-truth box (rotated
// IoU in fp64, rot_iou_device.h: the geometry of the NMS and of the mAP matching), labelled positive / negative / don't
// care against two thresholds, every ground-truth box may force its best anchor positive, and a positive anchor gets the
// box code that dn_decode_boxes inverts.  The host reference is targets.host_assign_targets.
//
// Launch sequence (fixed: it depends on the shapes only, never on the data; nothing is read back, nothing is allocated):
//   assign_init    per (image, row): the row's maximum IoU word = 0, its anchor word = INT_MAX
//   assign_iou     one wave per 64 neighbouring anchors, the image's ground truth through LDS 64 rows at a time with
//                  rot_iou_device.h's columns, circle test and IoU (stage_columns, circles_meet, pair_iou: the pair body
//                  of the NMS and of the mAP matching); the anchor's best (IoU, lowest row);
//                  per row the wave's maximum by a 64-bit integer max in LDS (positive doubles order as integers), then
//                  one global atomicMax of it
//   assign_arg     (force match only) per anchor and row: candidates are the anchors whose own best IoU reaches the row's
//                  maximum -- no other anchor can attain it; their IoU against the row is computed again (the same
//                  operations give the same bits) and an anchor that attains the maximum enters atomicMin(row's anchor word)
//   assign_write   per anchor: the lowest row that forces it (LDS atomicMin over the rows whose anchor word lies in the
//                  block), else the threshold match; label, mask, box code, matched row, best IoU
// Only integer atomics are used: two runs write the same bytes.
#include <climits>
#include <cmath>

#include "dn_internal.h"
#include "rot_iou_device.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxG = dn::kMaxGtRows;
constexpr int kChunk = 64;     // ground-truth rows held in LDS at a time
using dn::clampi;
using dn::kMaxImages;
using GtChunk = dn::BoxColumns<kChunk>;

struct Layout {
  size_t rowmax, rowarg, biou, bgt, total;
};

Layout layout(int n, long apl, int g) {
  dn::Carver c;
  Layout L;
  L.rowmax = c.take(sizeof(unsigned long long) * (size_t)n * g);
  L.rowarg = c.take(sizeof(int) * (size_t)n * g);
  L.biou = c.take(sizeof(double) * (size_t)n * apl);
  L.bgt = c.take(sizeof(int) * (size_t)n * apl);
  L.total = c.at;
  return L;
}

bool shapes_ok(int n, long apl, int g) {
  return n >= 1 && n <= kMaxImages && apl >= 1 && apl <= (long)INT_MAX - 64 && g >= 1 && g <= kMaxG;
}

__global__ void __launch_bounds__(kThreads) assign_init_kernel(unsigned long long* __restrict__ rowmax,
                                                               int* __restrict__ rowarg, int rows) {
  const int e = blockIdx.x * kThreads + threadIdx.x;
  if (e >= rows) return;
  rowmax[e] = 0ull;
  rowarg[e] = INT_MAX;
}

// Lane t is anchor i = 64 * blockIdx.x + t of image blockIdx.y.
__global__ void __launch_bounds__(64) assign_iou_kernel(const float* __restrict__ anchors, const float* __restrict__ gt,
                                                        const int* __restrict__ gt_count, long apl, int g,
                                                        unsigned long long* __restrict__ rowmax,
                                                        double* __restrict__ biou, int* __restrict__ bgt) {
#pragma clang fp contract(off)
  __shared__ GtChunk c;
  __shared__ unsigned long long wmax[kChunk];
  __shared__ dn::ClipScratch scratch;
  const int img = blockIdx.y, t = threadIdx.x;
  const long i = (long)blockIdx.x * 64 + t;
  const bool live = i < apl;
  const int gc = clampi(gt_count[img], g);
  dn::Box64 a;
  if (live) dn::box64(anchors + 6 * i, a);
  double best = 0.0;
  int best_j = -1;
  for (int j0 = 0; j0 < gc; j0 += kChunk) {
    const int rows = gc - j0 < kChunk ? gc - j0 : kChunk;
    __syncthreads();
    dn::stage_columns(c, gt + 6 * ((size_t)img * g + j0), rows, t);
    wmax[t] = 0ull;
    __syncthreads();
    if (live) {
      for (int jj = 0; jj < rows; ++jj) {
        if (!dn::circles_meet(c, jj, a)) continue;
        const double iou = dn::pair_iou(c, jj, a, scratch, t);
        if (iou > 0) atomicMax(&wmax[jj], (unsigned long long)__double_as_longlong(iou));
        if (iou > best) {
          best = iou;
          best_j = j0 + jj;
        }
      }
    }
    __syncthreads();
    if (t < rows && wmax[t] != 0ull) atomicMax(&rowmax[(size_t)img * g + j0 + t], wmax[t]);
  }
  if (live) {
    biou[(size_t)img * apl + i] = best;
    bgt[(size_t)img * apl + i] = best_j;
  }
}

__global__ void __launch_bounds__(64) assign_arg_kernel(const float* __restrict__ anchors, const float* __restrict__ gt,
                                                        const int* __restrict__ gt_count, long apl, int g,
                                                        const unsigned long long* __restrict__ rowmax,
                                                        const double* __restrict__ biou, int* __restrict__ rowarg) {
#pragma clang fp contract(off)
  __shared__ GtChunk c;
  __shared__ double rmax[kChunk];
  __shared__ dn::ClipScratch scratch;
  const int img = blockIdx.y, t = threadIdx.x;
  const long i = (long)blockIdx.x * 64 + t;
  const bool live = i < apl;
  const int gc = clampi(gt_count[img], g);
  const double mine = live ? biou[(size_t)img * apl + i] : 0.0;
  if (__ballot(mine > 0) == 0) return;          // no anchor of this wave touches a box (wave-uniform)
  dn::Box64 a;
  if (live) dn::box64(anchors + 6 * i, a);
  for (int j0 = 0; j0 < gc; j0 += kChunk) {
    const int rows = gc - j0 < kChunk ? gc - j0 : kChunk;
    __syncthreads();
    dn::stage_columns(c, gt + 6 * ((size_t)img * g + j0), rows, t);
    if (t < rows) rmax[t] = __longlong_as_double((long long)rowmax[(size_t)img * g + j0 + t]);
    __syncthreads();
    if (live && mine > 0) {
      for (int jj = 0; jj < rows; ++jj) {
        const double m = rmax[jj];
        if (!(m > 0) || mine < m) continue;     // an anchor that attains the row's maximum has a best IoU of at least it
        if (!dn::circles_meet(c, jj, a)) continue;
        const double iou = dn::pair_iou(c, jj, a, scratch, t);
        if (iou == m) atomicMin(&rowarg[(size_t)img * g + j0 + jj], (int)i);
      }
    }
  }
}

__global__ void __launch_bounds__(kThreads) assign_write_kernel(
    const float* __restrict__ anchors, const float* __restrict__ gt, const int* __restrict__ gt_count, long apl, int g,
    double pos_thr, double neg_thr, int force, const int* __restrict__ rowarg, const double* __restrict__ biou,
    const int* __restrict__ bgt, float* __restrict__ labels, float* __restrict__ reg, float* __restrict__ mask,
    int* __restrict__ matched, double* __restrict__ best_iou) {
#pragma clang fp contract(off)
  __shared__ int forced[kThreads];
  const int img = blockIdx.y, t = threadIdx.x;
  const long i0 = (long)blockIdx.x * kThreads, i = i0 + t;
  forced[t] = INT_MAX;
  __syncthreads();
  if (force) {
    const int gc = clampi(gt_count[img], g);
    for (int j = t; j < gc; j += kThreads) {
      const long w = rowarg[(size_t)img * g + j];          // INT_MAX: no anchor touches row j
      if (w >= i0 && w < i0 + kThreads) atomicMin(&forced[w - i0], j);
    }
  }
  __syncthreads();
  if (i >= apl) return;
  const size_t row = (size_t)img * apl + i;
  const double best = biou[row];
  int target = -1;
  float l0 = 0.f, l1 = 0.f;
  if (forced[t] != INT_MAX) {
    target = forced[t];
  } else if (best >= pos_thr) {
    target = bgt[row];
  } else if (best < neg_thr) {
    l0 = 1.f;
  }
  float code[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (target >= 0) {
    l1 = 1.f;
    const float* b = gt + 6 * ((size_t)img * g + target);
    const float* a = anchors + 6 * i;
    const double xa = a[0], ya = a[1], wa = a[2], ha = a[3], sa = a[4], ca = a[5];
    const double x = b[0], y = b[1], w = b[2], h = b[3], sn = b[4], cs = b[5];
    const double n = fmax(hypot(sn, cs), 1e-12);
    const double s = sn / n, c = cs / n;
    code[0] = (float)((x - xa) / wa);
    code[1] = (float)((y - ya) / ha);
    code[2] = (float)log(w / wa);
    code[3] = (float)log(h / ha);
    code[4] = (float)(s * ca - c * sa);
    code[5] = (float)(c * ca + s * sa);
  }
  labels[2 * row] = l0;
  labels[2 * row + 1] = l1;
  for (int q = 0; q < 6; ++q) reg[6 * row + q] = code[q];
  mask[row] = target >= 0 ? 1.f : 0.f;
  if (matched) matched[row] = target;
  if (best_iou) best_iou[row] = best;
}

}  // namespace

extern "C" size_t dn_assign_targets_workspace_bytes(int n_images, long anchors_per_image, int g) {
  if (!shapes_ok(n_images, anchors_per_image, g)) return 0;
  return layout(n_images, anchors_per_image, g).total;
}

extern "C" int dn_assign_targets(const float* anchors, const float* gt_boxes, const int32_t* gt_count, int n_images,
                                 long anchors_per_image, int g, double pos_thr, double neg_thr, int force_match,
                                 float* labels, float* reg_targets, float* reg_mask, int32_t* matched_gt,
                                 double* best_iou, void* workspace, size_t workspace_bytes, void* stream) {
  DN_REQUIRE(anchors && gt_boxes && gt_count && labels && reg_targets && reg_mask && workspace,
             "assign_targets: null pointer");
  DN_REQUIRE(n_images >= 1 && n_images <= kMaxImages, "assign_targets: %d images is out of range [1, %d]", n_images,
             kMaxImages);
  DN_REQUIRE(anchors_per_image >= 1 && anchors_per_image <= (long)INT_MAX - 64,
             "assign_targets: %ld anchors per image, must be in [1, %ld]", anchors_per_image, (long)INT_MAX - 64);
  DN_REQUIRE(g >= 1 && g <= kMaxG, "assign_targets: G = %d ground-truth rows, must be in [1, %d]", g, kMaxG);
  DN_REQUIRE(neg_thr > 0 && neg_thr <= pos_thr && pos_thr <= 1,
             "assign_targets: thresholds neg %g, pos %g: 0 < neg_thr <= pos_thr <= 1 is required", neg_thr, pos_thr);
  const Layout L = layout(n_images, anchors_per_image, g);
  DN_REQUIRE(workspace_bytes >= L.total,
             "assign_targets: workspace of %zu bytes, %zu needed (dn_assign_targets_workspace_bytes)", workspace_bytes,
             L.total);
  hipStream_t s = (hipStream_t)stream;
  char* ws = static_cast<char*>(workspace);
  unsigned long long* rowmax = reinterpret_cast<unsigned long long*>(ws + L.rowmax);
  int* rowarg = reinterpret_cast<int*>(ws + L.rowarg);
  double* biou = reinterpret_cast<double*>(ws + L.biou);
  int* bgt = reinterpret_cast<int*>(ws + L.bgt);
  const long apl = anchors_per_image;
  const int rows = n_images * g;
  const dim3 waves((unsigned)((apl + 63) / 64), (unsigned)n_images);
  hipLaunchKernelGGL(assign_init_kernel, dim3((rows + kThreads - 1) / kThreads), dim3(kThreads), 0, s, rowmax, rowarg,
                     rows);
  hipLaunchKernelGGL(assign_iou_kernel, waves, dim3(64), 0, s, anchors, gt_boxes, gt_count, apl, g, rowmax, biou, bgt);
  if (force_match)
    hipLaunchKernelGGL(assign_arg_kernel, waves, dim3(64), 0, s, anchors, gt_boxes, gt_count, apl, g, rowmax, biou,
                       rowarg);
  hipLaunchKernelGGL(assign_write_kernel, dim3((unsigned)((apl + kThreads - 1) / kThreads), (unsigned)n_images),
                     dim3(kThreads), 0, s, anchors, gt_boxes, gt_count, apl, g, pos_thr, neg_thr, force_match ? 1 : 0,
                     rowarg, biou, bgt, labels, reg_targets, reg_mask, matched_gt, best_iou);
  return dn::check_launch("assign_targets");
}
