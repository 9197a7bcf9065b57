// Detection decode: foreground probability (2-class softmax) and anchor-relative
// box decode for every anchor of every BEV cell, one coalesced pass (HBM-bound:
// 32 B in, 28 B out per anchor).
//
// Replaces the dense part of upstream:coperception/utils/postprocess.py
// (softmax + box decode vs anchors) that CoDetModule.predict_all runs on the CPU
// after the forward.  The per-anchor expression lives in decode_device.h: detect.hip
// (top-k + rotated NMS on the GPU) decodes its selected anchors with the same function.
#include "dn_internal.h"
#include "decode_device.h"

namespace {

__global__ void decode_kernel(const float* __restrict__ cls, const float* __restrict__ loc,
                              const float* __restrict__ anchors, long per_image, long total,
                              float* __restrict__ scores, float* __restrict__ boxes) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    float b[6];
    scores[i] = dn::decode_anchor(cls, loc, anchors, i, per_image, b);
    float* o = boxes + 6 * i;
    for (int q = 0; q < 6; ++q) o[q] = b[q];
  }
}

}  // namespace

extern "C" int dn_decode_boxes(const float* cls, const float* loc, const float* anchors,
                               int n_images, long anchors_per_image, float* scores, float* boxes,
                               void* stream) {
  DN_REQUIRE(cls && loc && anchors && scores && boxes, "decode: null pointer");
  DN_REQUIRE(n_images > 0 && anchors_per_image > 0, "decode: empty problem");
  const long total = (long)n_images * anchors_per_image;
  const int blocks = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
  hipLaunchKernelGGL(decode_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, cls, loc,
                     anchors, anchors_per_image, total, scores, boxes);
  return dn::check_launch("decode_kernel");
}
