// Segmentation evaluation (include/disconet_seg.h): dn_seg_confusion -- per pixel the arg-max of the class logits and
// the (label, prediction) cell of its image's confusion matrix, counted on the device.  One launch behind the forward, no
// host sync, no allocation: the state [n_images][classes^2 + 1] int64 stays on the device for the whole evaluation and
// MeanIoU.compute() (disconet_amd/seg.py) copies it once.
//
// The launch is a streaming pass (classes * 4 + 4 bytes read per pixel, 4 written when the prediction is wanted): grid
// (blocks, n_images), a workgroup sees one image and covers its pixels in a grid-stride loop.
//   * classes == 8 && ld == 8 on a 16-byte aligned map: the row is two 16-byte loads; everything else (any class count, a
//     channel slice of a wider map whose rows are not aligned) reads the row with scalar loads.
//   * counters: per-workgroup int32 in LDS, flushed once per non-zero cell with a 64-bit global atomic.  Label maps have
//     large uniform regions, so the 64 lanes of a wave mostly hit one or two cells: the wave aggregates its first two
//     DISTINCT cells (ballot of the lanes that share the first pending lane's cell, one LDS atomic of the population count
//     by that lane); whatever is left -- a wave on a class boundary, or noise -- counts itself with one LDS atomic a lane.
// The counts are integers: the order of the atomics does not matter, the result is deterministic.
#include "dn_internal.h"
#include "disconet_seg.h"

namespace {

typedef float f32x4c __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;
constexpr int kMaxClasses = 32;
constexpr int kWaveRounds = 2;      // distinct cells a wave aggregates before its remaining lanes count themselves

// torch.argmax / numpy.argmax: the first NaN if the row has one, else the first maximum (-0.0 == +0.0; all -inf -> 0)
__device__ inline void argmax_step(float v, int c, float& best, int& at) {
  if (best == best && (v > best || v != v)) { best = v; at = c; }
}

template <bool ROW8>
__global__ __launch_bounds__(kThreads) void seg_confusion_kernel(const float* __restrict__ logits, int ld,
                                                                 const int32_t* __restrict__ labels,
                                                                 const uint8_t* __restrict__ live, long pixels, int classes,
                                                                 unsigned long long* __restrict__ state,
                                                                 int32_t* __restrict__ pred) {
  __shared__ int hist[kMaxClasses * kMaxClasses + 1];
  const int img = blockIdx.y;
  const int cells = classes * classes;                     // hist[cells] = the ignored pixels
  for (int i = threadIdx.x; i <= cells; i += kThreads) hist[i] = 0;
  __syncthreads();
  const bool alive = live ? live[img] != 0 : true;
  const long base = (long)img * pixels;
  const int lane = threadIdx.x & 63;
  // p0 depends on the workgroup alone: every lane of a wave makes the same trips, the ballots below see whole waves
  for (long p0 = (long)blockIdx.x * kThreads; p0 < pixels; p0 += (long)gridDim.x * kThreads) {
    const long p = p0 + threadIdx.x;
    const bool in = p < pixels;
    int cell = -1;
    if (in) {
      const float* z = logits + (base + p) * ld;
      float best;
      int at = 0;
      if constexpr (ROW8) {
        const f32x4c a = *reinterpret_cast<const f32x4c*>(z), b = *reinterpret_cast<const f32x4c*>(z + 4);
        best = a[0];
#pragma unroll
        for (int c = 1; c < 4; ++c) argmax_step(a[c], c, best, at);
#pragma unroll
        for (int c = 0; c < 4; ++c) argmax_step(b[c], 4 + c, best, at);
      } else {
        best = z[0];
        for (int c = 1; c < classes; ++c) argmax_step(z[c], c, best, at);
      }
      const int y = labels[base + p];
      if (pred) pred[base + p] = at;
      cell = (alive && y >= 0 && y < classes) ? y * classes + at : cells;
    }
    unsigned long long todo = __ballot(in);
    for (int round = 0; todo && round < kWaveRounds; ++round) {   // wave-uniform: one round per distinct cell of the wave
      const int leader = __ffsll((long long)todo) - 1;
      const int c = __shfl(cell, leader);
      const unsigned long long same = __ballot(cell == c);   // a lane outside the map holds -1, never a cell
      if (lane == leader) atomicAdd(&hist[c], __popcll(same));
      todo &= ~same;
    }
    if ((todo >> lane) & 1) atomicAdd(&hist[cell], 1);       // a wave on a class boundary or on noise: the rest lane by lane
  }
  __syncthreads();
  unsigned long long* row = state + (size_t)img * (cells + 1);
  for (int i = threadIdx.x; i <= cells; i += kThreads) {
    const int v = hist[i];
    if (v) atomicAdd(&row[i], (unsigned long long)v);
  }
}

}  // namespace

extern "C" int dn_seg_confusion(const float* logits, int ld, const int32_t* labels, const uint8_t* live, int n_images,
                                long pixels_per_image, int classes, int64_t* state, int32_t* pred, void* stream) {
  DN_REQUIRE(logits && labels && state, "seg_confusion: null logits, labels or state");
  DN_REQUIRE(classes >= 2 && classes <= kMaxClasses, "seg_confusion: %d classes (2 .. %d are built)", classes, kMaxClasses);
  DN_REQUIRE(ld >= classes, "seg_confusion: ld %d < %d classes", ld, classes);
  DN_REQUIRE(n_images > 0 && n_images <= 65535, "seg_confusion: %d images (1 .. 65535)", n_images);
  // a workgroup's int32 counters: at most 1024 workgroups an image, each below 2^31 pixels
  DN_REQUIRE(pixels_per_image > 0 && pixels_per_image <= (1L << 40), "seg_confusion: %ld pixels per image (1 .. 2^40)",
             pixels_per_image);
  DN_REQUIRE((reinterpret_cast<uintptr_t>(state) & 7) == 0 && (reinterpret_cast<uintptr_t>(logits) & 3) == 0 &&
                 (reinterpret_cast<uintptr_t>(labels) & 3) == 0 && (reinterpret_cast<uintptr_t>(pred) & 3) == 0,
             "seg_confusion: state must be 8-byte aligned, logits / labels / pred 4-byte aligned");
  // four trips of the grid-stride loop a workgroup where the map is large enough: fewer flushes, still > 1000 workgroups at 20 images
  long blocks = (pixels_per_image + 4 * kThreads - 1) / (4 * kThreads);
  blocks = blocks < 1 ? 1 : (blocks > 1024 ? 1024 : blocks);
  const dim3 grid((unsigned)blocks, (unsigned)n_images);
  const bool row8 = classes == 8 && ld == 8 && (reinterpret_cast<uintptr_t>(logits) & 15) == 0;
  if (row8)
    hipLaunchKernelGGL(seg_confusion_kernel<true>, grid, dim3(kThreads), 0, (hipStream_t)stream, logits, ld, labels, live,
                       pixels_per_image, classes, reinterpret_cast<unsigned long long*>(state), pred);
  else
    hipLaunchKernelGGL(seg_confusion_kernel<false>, grid, dim3(kThreads), 0, (hipStream_t)stream, logits, ld, labels, live,
                       pixels_per_image, classes, reinterpret_cast<unsigned long long*>(state), pred);
  return dn::check_launch("seg_confusion_kernel");
}
