// One anchor's detection decode, shared by decode.hip (every anchor) and detect.hip (the selected ones): both kernels
// inline this same expression, so the scores detect.hip orders by and the boxes it returns are bit for bit what
// dn_decode_boxes writes for those anchors.
#pragma once
#include <hip/hip_runtime.h>

namespace dn {

// foreground probability of anchor i: softmax over {background, foreground}, max-shifted like F.softmax
__device__ __forceinline__ float fg_score(const float* __restrict__ cls, long i) {
  const float c0 = cls[2 * i], c1 = cls[2 * i + 1];
  const float m = fmaxf(c0, c1);
  const float e0 = expf(c0 - m), e1 = expf(c1 - m);
  return e1 / (e0 + e1);
}

// score and box (x, y, w, h, sin, cos) of anchor i of a batch whose images hold `per_image` anchors each
__device__ __forceinline__ float decode_anchor(const float* __restrict__ cls, const float* __restrict__ loc,
                                               const float* __restrict__ anchors, long i, long per_image,
                                               float* __restrict__ o) {
  const float* a = anchors + 6 * (i % per_image);
  const float* t = loc + 6 * i;
  o[0] = a[0] + t[0] * a[2];
  o[1] = a[1] + t[1] * a[3];
  o[2] = a[2] * expf(t[2]);
  o[3] = a[3] * expf(t[3]);
  o[4] = a[4] * t[5] + a[5] * t[4];
  o[5] = a[5] * t[5] - a[4] * t[4];
  return fg_score(cls, i);
}

}  // namespace dn
