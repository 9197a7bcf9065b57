// `--com agent` (upstream AgentWiseWeightedFusion): one scalar weight per agent of the ego's list,
// softmax over the list, weighted sum.  Two launches behind dn_warp_neighbors / dn_warp_neighbors_fm:
//   score    disco_fuse_mlp_kernel<.., AG> (fuse_mlp.hip): layers 1-4 of the weight net on (ego, map_k), the scores times
//            conv1_5's weights summed per 32-pixel tile -> one partial per (ego, list slot, tile) in the workspace
//   combine  agent_combine_kernel (here): per ego the partials folded in tile order, + b5, ReLU, the softmax over the list
//            (at most 8 scalars, re-derived by every workgroup of the ego: 8 x tiles floats from L2), then the weighted sum
//            over the ego's map and the SAME warped rows the score launch read -- each pair is warped once per step
// No atomics, no host synchronisation, the workspace is written before it is read in stream order: graph-capturable and
// bit-identical from run to run and in every launch form of the score kernel.  The contract is include/disconet_hip.h ::
// dn_agent_fuse; the order of every sum is agent_device.h's.
#include "agent_device.h"
#include "dn_internal.h"
#include "ego_list.h"

namespace {

using agentw::f32x4;

constexpr int MAX_AGENTS = 8;     // fuse_mlp.hip's
constexpr int QPT = 4;            // 16-byte pieces per thread
constexpr int TCH = 256;          // partials staged per trip of the fold

__device__ inline f32x4 ldq(const float* p) { return *reinterpret_cast<const f32x4*>(p); }

// grid (pieces of the map, ego_count * batch); 256 threads, QPT pieces of four channels each.
// FM: `warped` is fragment-major (dn_warp_neighbors_fm): the pieces are walked in ITS order (every load instruction of a wave
// is one contiguous 1 KB run) and the ego's map / the output are addressed through it; else everything is pixel-major.
template <bool FM>
__global__ void __launch_bounds__(256)
agent_combine_kernel(const float* __restrict__ feat, const float* __restrict__ warped, const int32_t* __restrict__ num_agent,
                     const float* __restrict__ partials, const float* __restrict__ b5, int batch, int agents, int hw, int c,
                     int only_v2i, int ego_first, int ego_count, int tiles, float* __restrict__ fused,
                     float* __restrict__ agent_weights) {
  __shared__ float part_s[MAX_AGENTS][TCH];
  __shared__ float a_s[MAX_AGENTS], w_s[MAX_AGENTS];
  __shared__ int jl_s[MAX_AGENTS];
  const int out_image = blockIdx.y;                       // (i - ego_first) * batch + b
  const int b = out_image % batch, il = out_image / batch, i = ego_first + il;
  const int live = live_count(num_agent, b, agents);
  const int tid = threadIdx.x;
  const size_t quads = (size_t)hw * (c >> 2);
  const float* ego = feat + ((size_t)i * batch + b) * hw * c;
  float* out = fused + (size_t)out_image * hw * c;
  const size_t q0 = (size_t)blockIdx.x * (256 * QPT);
  float* wout = agent_weights ? agent_weights + ((size_t)b * ego_count + il) * agents : nullptr;

  if (i >= live || partials == nullptr) {                 // a padded ego, or agents == 1: its map passes through, the same bits
#pragma unroll
    for (int u = 0; u < QPT; ++u) {
      const size_t q = q0 + (size_t)u * 256 + tid;
      if (q < quads) *reinterpret_cast<f32x4*>(out + 4 * q) = ldq(ego + 4 * q);
    }
    if (wout && blockIdx.x == 0 && tid < agents) wout[tid] = (tid == 0 && i < live) ? 1.f : 0.f;
    return;
  }

  // the list, in the reference's order: the ego, then j ascending (workgroup-uniform)
  int n = 1;
  for (int j = 0; j < live; ++j)
    if (DN_LISTED_LIVE(i, j, only_v2i)) {
      if (tid == 0) jl_s[n] = j;
      ++n;
    }
  if (tid == 0) jl_s[0] = i;

  // a_k: thread k folds the tiles of list slot k in ascending order, TCH tiles per trip through LDS
  const float* part = partials + ((size_t)b * ego_count + il) * agents * tiles;
  float folded = 0.f;
  for (int t0 = 0; t0 < tiles; t0 += TCH) {
    if (t0 + tid < tiles)
      for (int k = 0; k < n; ++k) part_s[k][tid] = part[(size_t)k * tiles + t0 + tid];
    __syncthreads();
    if (tid < n) {
      const int m = tiles - t0 < TCH ? tiles - t0 : TCH;
      for (int t = 0; t < m; ++t) folded = agentw::fold_tile(folded, part_s[tid][t], t0 + t == 0);
    }
    __syncthreads();
  }
  if (tid < n) a_s[tid] = agentw::agent_scalar(folded, b5[0]);
  __syncthreads();
  if (tid == 0) agentw::list_softmax(a_s, n, w_s);
  __syncthreads();
  if (wout && blockIdx.x == 0 && tid < agents) wout[tid] = tid < n ? w_s[tid] : 0.f;

  // fused = sum_k w_k map_k: the first product, then product by product in list order
  const float* wbase = warped + ((size_t)b * ego_count + il) * (size_t)(agents - 1) * hw * c;
  const int KS = c >> 4;
#pragma unroll
  for (int u = 0; u < QPT; ++u) {
    const size_t q = q0 + (size_t)u * 256 + tid;
    if (q >= quads) break;
    size_t o = 4 * q;                                     // this piece in a pixel-major map
    if (FM) {   // piece q of a fragment-major block: [tile][k-step][half r][lane = 32 hh + j] = channels 16 ks + 8 hh + 4 r of pixel 32 t + j
      const int lane = (int)(q & 63), r = (int)((q >> 6) & 1);
      const size_t step = q >> 7;
      const int ks = (int)(step % KS);
      const size_t t = step / KS;
      o = (t * 32 + (lane & 31)) * c + 16 * ks + 8 * (lane >> 5) + 4 * r;
    }
    f32x4 acc = agentw::weigh(ldq(ego + o), w_s[0]);
    for (int k = 1; k < n; ++k) {
      const int j = jl_s[k];
      const float* nb = wbase + (size_t)(j - (j > i ? 1 : 0)) * hw * c;
      acc = agentw::weigh_add(acc, ldq(nb + 4 * q), w_s[k]);
    }
    *reinterpret_cast<f32x4*>(out + o) = acc;
  }
}

size_t partial_floats(int batch, int agents, int ego_count, int hw) {
  return (size_t)batch * ego_count * agents * ((hw + 31) / 32);
}

}  // namespace

extern "C" size_t dn_agent_fuse_workspace_bytes(int batch, int agents, int ego_count, int hw) {
  if (batch <= 0 || agents <= 0 || ego_count <= 0 || hw <= 0) return 0;
  return (partial_floats(batch, agents, ego_count, hw) * sizeof(float) + 15) / 16 * 16;
}

extern "C" int dn_agent_fuse(const float* feat, const float* warped, int warped_fm, const int32_t* num_agent,
                             const dn_fuse_mlp_params* p, const float* w5, const float* b5, int batch, int agents, int hw,
                             int c, int only_v2i, int ego_first, int ego_count, void* workspace, size_t workspace_bytes,
                             float* fused, float* agent_weights, void* stream) {
  DN_REQUIRE(feat && num_agent && p && w5 && b5 && fused && workspace, "agent fuse: null pointer");
  DN_REQUIRE(batch > 0 && agents > 0 && hw > 0, "agent fuse: empty problem");
  DN_REQUIRE(dn_fuse_mlp_supported(c), "agent fuse: %d channels unsupported (64, 128 or 256)", c);
  DN_REQUIRE(ego_first >= 0 && ego_count > 0 && ego_first + ego_count <= agents,
             "agent fuse: ego range [%d, %d) outside 0..%d", ego_first, ego_first + ego_count, agents);
  DN_REQUIRE(agents <= MAX_AGENTS, "agent fuse: at most %d agents supported (got %d)", MAX_AGENTS, agents);
  DN_REQUIRE(agents < 2 || warped, "agent fuse: neighbours present but warped is null");
  DN_REQUIRE(!warped_fm || hw % 32 == 0, "agent fuse (fragment-major): hw %d must be a multiple of 32", hw);
  DN_REQUIRE(workspace_bytes >= dn_agent_fuse_workspace_bytes(batch, agents, ego_count, hw),
             "agent fuse: workspace of %zu bytes, dn_agent_fuse_workspace_bytes asks for %zu", workspace_bytes,
             dn_agent_fuse_workspace_bytes(batch, agents, ego_count, hw));
  auto aligned16 = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; };
  DN_REQUIRE(aligned16(feat) && aligned16(warped) && aligned16(fused) && aligned16(workspace),
             "agent fuse: buffers must be 16-byte aligned");
  DN_REQUIRE((long)batch * ego_count <= 65535, "agent fuse: %ld output images, at most 65535", (long)batch * ego_count);
  DN_REQUIRE((size_t)hw * c < ((size_t)1 << 31), "agent fuse: a map of %d x %d floats is too large", hw, c);
  hipStream_t s = (hipStream_t)stream;
  float* partials = agents > 1 ? (float*)workspace : nullptr;      // agents == 1: every list is the ego alone -- a copy
  if (partials) {
    const int rc = dn::fuse_mlp_agent_scores(feat, warped, warped_fm, num_agent, p, w5, batch, agents, hw, c, only_v2i,
                                             ego_first, ego_count, partials, s);
    if (rc) return rc;
  }
  const size_t quads = (size_t)hw * (c >> 2);
  dim3 grid((unsigned)((quads + 256 * QPT - 1) / (256 * QPT)), batch * ego_count);
  const int tiles = (hw + 31) / 32;
  if (warped_fm && partials)
    hipLaunchKernelGGL(agent_combine_kernel<true>, grid, dim3(256), 0, s, feat, warped, num_agent, partials, b5, batch, agents,
                       hw, c, only_v2i, ego_first, ego_count, tiles, fused, agent_weights);
  else
    hipLaunchKernelGGL(agent_combine_kernel<false>, grid, dim3(256), 0, s, feat, warped, num_agent, partials, b5, batch, agents,
                       hw, c, only_v2i, ego_first, ego_count, tiles, fused, agent_weights);
  return dn::check_launch("agent_combine_kernel");
}
