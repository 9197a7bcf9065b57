// Device phases that the kernels of `--com agent` share (upstream AgentWiseWeightedFusion; the contract is
// include/disconet_hip.h :: dn_agent_fuse): the score launch (fuse_mlp.hip, AG), the combine launch (agent_fuse.hip) and
// the training list kernels (train_ops.hip) sum, fold and weigh in ONE order, so that their scalars agree bit for bit on
// the same scores.  Every function that rounds carries `#pragma clang fp contract(off)`: products are rounded to fp32
// before they are added, as the contract says.
#pragma once
#include <hip/hip_runtime.h>

namespace agentw {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kMaxList = 16;      // entries of one ego's list (train.fusion_lists refuses longer ones; inference: agents <= 8)

// one term of a_k: conv1_5's weight of the pixel times its score; a lane past the end of the map contributes +0
__device__ inline float score_term(float s, float w5, bool valid) {
#pragma clang fp contract(off)
  const float v = s * w5;
  return valid ? v : 0.f;
}

// The sum over a tile of 32 consecutive pixels.  Lane l (and lane l + 32, which holds the same term) carries pixel l of the
// tile; the terms are added as a binary tree over the pixel index: first l with l + 16, then with l + 8, + 4, + 2, + 1.  Every
// lane returns the same bits.
__device__ inline float tile_sum32(float v) {
#pragma clang fp contract(off)
#pragma unroll
  for (int d = 16; d > 0; d >>= 1) v = v + __shfl_xor(v, d, 64);
  return v;
}

// a_k = relu(b5 + the tiles' sums folded in ascending tile order)
__device__ inline float fold_tile(float acc, float tile_sum, bool first) {
#pragma clang fp contract(off)
  return first ? tile_sum : acc + tile_sum;
}
__device__ inline float agent_scalar(float folded, float b5) {
#pragma clang fp contract(off)
  return fmaxf(folded + b5, 0.f);
}

// w[k] = expf(a[k] - max a) / sum, the sum taken in list order; n >= 1.  In place (w may be a).
__device__ inline void list_softmax(const float* a, int n, float* w) {
#pragma clang fp contract(off)
  float m = a[0];
  for (int k = 1; k < n; ++k) m = fmaxf(m, a[k]);
  float sum = 0.f;
  for (int k = 0; k < n; ++k) {
    const float e = expf(a[k] - m);
    w[k] = e;
    sum = k == 0 ? e : sum + e;
  }
  for (int k = 0; k < n; ++k) w[k] = w[k] / sum;
}

// the weighted sum in list order: the first product, then each further product rounded and added
__device__ inline f32x4 weigh(const f32x4 v, float w) {
#pragma clang fp contract(off)
  return v * w;
}
__device__ inline f32x4 weigh_add(const f32x4 acc, const f32x4 v, float w) {
#pragma clang fp contract(off)
  const f32x4 p = v * w;
  return acc + p;
}

}  // namespace agentw
