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

// box (x, y, w, h, sin, cos) of the six box codes t against the anchor row a = (x, y, w, h, sin, cos).  The one decode
// expression of the library: decode_anchor below and the corner loss (train_ops.hip :: corner_one, which decodes the
// predicted and the target codes of an anchor) inline these lines.
//   centre (a0 + t0 a2, a1 + t1 a3), size (a2 exp t2, a3 exp t3), pair sin = a4 t5 + a5 t4, cos = a5 t5 - a4 t4
// The fused multiply-adds are WRITTEN OUT -- they are the ones the compiler chose for these expressions in dn_decode_boxes and
// dn_detect while contraction was left to it (read from both kernels' ISA: the same products and fused operations, so the
// same bits; only their order in the instruction stream moved) -- because left to itself it fuses two
// inlined copies of one expression differently (cos as fma(a5, t5, -(a4 t4)) in one, fma(-a4, t4, a5 t5) in the other), and the
// corner loss needs equal codes to decode to equal bits.
__device__ __forceinline__ void decode_box(const float* __restrict__ a, const float* __restrict__ t, float* __restrict__ o) {
#pragma clang fp contract(off)
  o[0] = fmaf(t[0], a[2], a[0]);
  o[1] = fmaf(t[1], a[3], a[1]);
  o[2] = a[2] * expf(t[2]);
  o[3] = a[3] * expf(t[3]);
  o[4] = fmaf(a[4], t[5], a[5] * t[4]);
  o[5] = fmaf(a[5], t[5], -(a[4] * t[4]));
}

// score and box (x, y, w, h, sin, cos) of anchor i of a batch whose images hold `per_image` anchors each
__device__ __forceinline__ float decode_anchor(const float* __restrict__ cls, const float* __restrict__ loc,
                                               const float* __restrict__ anchors, long i, long per_image,
                                               float* __restrict__ o) {
  decode_box(anchors + 6 * (i % per_image), loc + 6 * i, o);
  return fg_score(cls, i);
}

}  // namespace dn
