// Occlusion-aware lidar scenes (dn_lidar_scan): every agent's rays cast against the scene's solids, the nearest hit kept,
// and the ground truth that some live agent of the scene sees.  The contract is in include/disconet_hip.h; the host
// statement that defines the bytes is lidar.host_scan.  This is the project's own sensor model, not recalled from upstream.
// All geometry is fp64, + - * / and comparisons only, and every function that computes it carries
// `#pragma clang fp contract(off)`.
//
// lidar_scan_kernel    grid (ceil(R / 256), A*S), one ray per lane.  The workgroup first carries the scene's solids into its
//                      agent's frame (one solid per lane, K <= 256) and keeps, per solid, the ray origin in the solid's
//                      frame, the heading, the half sizes and the z slab in LDS: 8 doubles = 64 B a solid, 16 KB at the
//                      most.  In the ray loop all lanes read the same LDS address, a broadcast.  A ragged last block only
//                      masks its rays: every lane reaches both barriers.  The returns are counted in LDS first (integer
//                      atomics), then one global atomic per solid the workgroup hit.
// lidar_visible_kernel grid A*S, one object per lane: the box in the agent's frame, the strict extents test, the hits
//                      summed over the scene's live agents; the kept rows are compacted in k order (64-bit ballot,
//                      popcount prefix per wave, wave counts through LDS, as render.hip bins its rows).  With gt_ids
//                      (dn_lidar_scan_ids) each kept row's k is written beside it, -1 beyond the count.
#include <cmath>

#include "dn_internal.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
static_assert(DN_LIDAR_MAX_SOLIDS <= kThreads, "one solid per lane");

struct Frame {
  double cx, cy, s, c;
};

// synthetic.boxes_in_agent_frame's expressions on T = sensor_from_world[s][a] (row-major 4 x 4)
__device__ __forceinline__ Frame into_agent_frame(const double* T, const double* solid) {
#pragma clang fp contract(off)
  const double x = solid[0], y = solid[1], sn = solid[4], cs = solid[5];
  Frame f;
  f.cx = (T[0] * x + T[1] * y) + T[3];
  f.cy = (T[4] * x + T[5] * y) + T[7];
  f.s = T[4] * cs + T[5] * sn;
  f.c = T[0] * cs + T[1] * sn;
  return f;
}

// one axis of the slab test; false: the ray runs along the slab outside it
__device__ __forceinline__ bool slab(double lo, double hi, double o, double e, double& tmin, double& tmax) {
#pragma clang fp contract(off)
  if (e == 0.0) return lo <= o && o <= hi;
  const double t0 = (lo - o) / e, t1 = (hi - o) / e;
  const double tn = t0 < t1 ? t0 : t1, tf = t0 < t1 ? t1 : t0;
  tmin = tn > tmin ? tn : tmin;
  tmax = tf < tmax ? tf : tmax;
  return true;
}

__global__ void __launch_bounds__(kThreads)
lidar_scan_kernel(const double* __restrict__ solids, const int32_t* __restrict__ solid_count,
                  const double* __restrict__ sensor_from_world, const int32_t* __restrict__ num_agent,
                  const double* __restrict__ dirs, const float* __restrict__ jitter, int S, int A, int K, int R,
                  double max_range, double ground_z, int keep_ground, float* __restrict__ points, int32_t* __restrict__ hit,
                  int32_t* __restrict__ solid_hits) {
#pragma clang fp contract(off)
  __shared__ double l_ox[DN_LIDAR_MAX_SOLIDS], l_oy[DN_LIDAR_MAX_SOLIDS], l_c[DN_LIDAR_MAX_SOLIDS], l_s[DN_LIDAR_MAX_SOLIDS];
  __shared__ double l_hw[DN_LIDAR_MAX_SOLIDS], l_hl[DN_LIDAR_MAX_SOLIDS], l_zlo[DN_LIDAR_MAX_SOLIDS], l_zhi[DN_LIDAR_MAX_SOLIDS];
  __shared__ int l_cnt[DN_LIDAR_MAX_SOLIDS];

  const int tid = threadIdx.x;
  const int img = blockIdx.y, a = img / S, s = img - a * S;
  int n = 0;                                                   // a padded agent's image: no solids, no ground
  const bool live = a < num_agent[s];
  if (live) {
    n = solid_count[s];
    n = n < 0 ? 0 : (n > K ? K : n);
  }
  if (tid < n) {
    const double* row = solids + ((size_t)s * K + tid) * 8;
    const Frame f = into_agent_frame(sensor_from_world + ((size_t)s * A + a) * 16, row);
    const double mx = -f.cx, my = -f.cy;
    l_ox[tid] = mx * f.c + my * f.s;
    l_oy[tid] = my * f.c - mx * f.s;
    l_c[tid] = f.c;
    l_s[tid] = f.s;
    l_hw[tid] = row[2] / 2.0;
    l_hl[tid] = row[3] / 2.0;
    l_zlo[tid] = row[6];
    l_zhi[tid] = row[7];
  }
  l_cnt[tid] = 0;
  __syncthreads();

  const int r = blockIdx.x * kThreads + tid;
  if (r < R) {
    const double dx = dirs[3 * (size_t)r], dy = dirs[3 * (size_t)r + 1], dz = dirs[3 * (size_t)r + 2];
    double best = INFINITY;
    int best_k = -2;
    for (int k = 0; k < n; ++k) {
      const double c = l_c[k], sn = l_s[k], hw = l_hw[k], hl = l_hl[k];
      const double ex = dx * c + dy * sn, ey = dy * c - dx * sn;
      double tmin = -INFINITY, tmax = INFINITY;
      if (!slab(-hw, hw, l_ox[k], ex, tmin, tmax)) continue;
      if (!slab(-hl, hl, l_oy[k], ey, tmin, tmax)) continue;
      if (!slab(l_zlo[k], l_zhi[k], 0.0, dz, tmin, tmax)) continue;
      if (0.0 < tmin && tmin <= tmax && tmin <= max_range && tmin < best) {
        best = tmin;
        best_k = k;
      }
    }
    if (live && dz < 0.0) {
      const double t = ground_z / dz;
      if (0.0 < t && t <= max_range && t < best) {
        best = t;
        best_k = -1;
      }
    }
    if (best_k == -1 && !keep_ground) best_k = -2;
    const size_t at = (size_t)img * R + r;
    float4 p;
    if (best_k == -2) {
      const float nan = __uint_as_float(0x7fc00000u);
      p = make_float4(nan, nan, nan, nan);
    } else {
      const double t = jitter ? best + (double)jitter[at] : best;
      p = make_float4((float)(t * dx), (float)(t * dy), (float)(t * dz), best_k >= 0 ? 1.0f : 0.0f);
    }
    reinterpret_cast<float4*>(points)[at] = p;
    hit[at] = best_k;
    if (best_k >= 0) atomicAdd(&l_cnt[best_k], 1);
  }
  __syncthreads();
  if (tid < n) {
    const int c = l_cnt[tid];
    if (c) atomicAdd(&solid_hits[(size_t)img * K + tid], c);
  }
}

__global__ void __launch_bounds__(kThreads)
lidar_visible_kernel(const double* __restrict__ solids, const int32_t* __restrict__ solid_count,
                     const int32_t* __restrict__ object_count, const double* __restrict__ sensor_from_world,
                     const int32_t* __restrict__ num_agent, const int32_t* __restrict__ solid_hits, int S, int A, int K,
                     int min_points, double half_extent, int G, float* __restrict__ gt_boxes, int32_t* __restrict__ gt_count,
                     int32_t* __restrict__ gt_own_hits, int32_t* __restrict__ gt_ids) {
#pragma clang fp contract(off)
  __shared__ int wave_count[kWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int img = blockIdx.x, a = img / S, s = img - a * S;
  int live = num_agent[s];
  live = live < 0 ? 0 : (live > A ? A : live);
  int n = 0;
  if (a < live) {
    int ns = solid_count[s];
    ns = ns < 0 ? 0 : (ns > K ? K : ns);
    n = object_count[s];
    n = n < 0 ? 0 : (n > ns ? ns : n);
  }
  bool keep = false;
  Frame f = {0.0, 0.0, 0.0, 0.0};
  const double* row = nullptr;
  if (tid < n) {
    row = solids + ((size_t)s * K + tid) * 8;
    f = into_agent_frame(sensor_from_world + ((size_t)s * A + a) * 16, row);
    int seen = 0;
    for (int j = 0; j < live; ++j) seen += solid_hits[((size_t)j * S + s) * K + tid];
    keep = fabs(f.cx) < half_extent && fabs(f.cy) < half_extent && seen >= min_points;
  }
  const unsigned long long ballot = __ballot(keep);
  const int before = __popcll(ballot & ((1ull << lane) - 1ull));
  if (lane == 0) wave_count[wave] = __popcll(ballot);
  __syncthreads();
  int offset = 0, total = 0;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) {
    const int c = wave_count[w];
    if (w < wave) offset += c;
    total += c;
  }
  const int kept = total < G ? total : G;
  if (keep && offset + before < G) {
    const size_t e = (size_t)img * G + offset + before;
    float* o = gt_boxes + 6 * e;
    o[0] = (float)f.cx; o[1] = (float)f.cy; o[2] = (float)row[2]; o[3] = (float)row[3]; o[4] = (float)f.s; o[5] = (float)f.c;
    gt_own_hits[e] = solid_hits[(size_t)img * K + tid];
    if (gt_ids) gt_ids[e] = tid;
  }
  for (int g = kept + tid; g < G; g += kThreads) {
    const size_t e = (size_t)img * G + g;
#pragma unroll
    for (int j = 0; j < 6; ++j) gt_boxes[6 * e + j] = 0.0f;
    gt_own_hits[e] = 0;
    if (gt_ids) gt_ids[e] = -1;
  }
  if (tid == 0) gt_count[img] = kept;
}

// both entry points: gt_ids is null for dn_lidar_scan
int lidar_scan(const double* solids, const int32_t* solid_count, const int32_t* object_count,
               const double* sensor_from_world, const int32_t* num_agent, const double* dirs, const float* range_jitter,
               int n_scenes, int n_agents, int k, int n_rays, double max_range, double ground_z, int keep_ground,
               int min_points, double half_extent, int gt_rows, float* points, int32_t* hit, int32_t* solid_hits,
               float* gt_boxes, int32_t* gt_count, int32_t* gt_own_hits, int32_t* gt_ids, void* stream) {
  DN_REQUIRE(k >= 0 && k <= DN_LIDAR_MAX_SOLIDS, "lidar_scan: K = %d solids, must be in [0, %d]", k, DN_LIDAR_MAX_SOLIDS);
  DN_REQUIRE(n_rays >= 1 && n_scenes >= 1 && n_agents >= 1 && gt_rows >= 1,
             "lidar_scan: R = %d, S = %d, A = %d, G = %d, every one must be >= 1", n_rays, n_scenes, n_agents, gt_rows);
  DN_REQUIRE((long long)n_scenes * n_agents <= 65535, "lidar_scan: %d x %d images, at most 65535", n_agents, n_scenes);
  DN_REQUIRE(solids || k == 0, "lidar_scan: null solids");
  DN_REQUIRE(solid_count && object_count, "lidar_scan: null solid_count / object_count");
  DN_REQUIRE(sensor_from_world, "lidar_scan: null sensor_from_world");
  DN_REQUIRE(num_agent, "lidar_scan: null num_agent");
  DN_REQUIRE(dirs, "lidar_scan: null dirs");
  DN_REQUIRE(points && hit && (solid_hits || k == 0), "lidar_scan: null points / hit / solid_hits");
  DN_REQUIRE(gt_boxes && gt_count && gt_own_hits, "lidar_scan: null gt_boxes / gt_count / gt_own_hits");
  DN_REQUIRE((reinterpret_cast<size_t>(points) & 15) == 0, "lidar_scan: points must be 16-byte aligned");
  DN_REQUIRE(std::isfinite(max_range) && max_range > 0, "lidar_scan: max_range = %g, must be finite and > 0", max_range);
  DN_REQUIRE(std::isfinite(half_extent) && half_extent > 0, "lidar_scan: half_extent = %g, must be finite and > 0", half_extent);
  DN_REQUIRE(std::isfinite(ground_z), "lidar_scan: ground_z = %g, must be finite", ground_z);
  hipStream_t s = (hipStream_t)stream;
  const int images = n_scenes * n_agents;
  if (k > 0 && dn::zero_fill(solid_hits, (size_t)images * k * sizeof(int32_t), s) != hipSuccess)
    return dn::fail(DN_ERR_LAUNCH, "lidar_scan: zero fill of solid_hits failed");
  const dim3 grid((n_rays + kThreads - 1) / kThreads, images);
  hipLaunchKernelGGL(lidar_scan_kernel, grid, dim3(kThreads), 0, s, solids, solid_count, sensor_from_world, num_agent, dirs,
                     range_jitter, n_scenes, n_agents, k, n_rays, max_range, ground_z, keep_ground, points, hit, solid_hits);
  if (int rc = dn::check_launch("lidar_scan_kernel")) return rc;
  hipLaunchKernelGGL(lidar_visible_kernel, dim3(images), dim3(kThreads), 0, s, solids, solid_count, object_count,
                     sensor_from_world, num_agent, solid_hits, n_scenes, n_agents, k, min_points, half_extent, gt_rows,
                     gt_boxes, gt_count, gt_own_hits, gt_ids);
  return dn::check_launch("lidar_visible_kernel");
}

}  // namespace

extern "C" int dn_lidar_scan(const double* solids, const int32_t* solid_count, const int32_t* object_count,
                             const double* sensor_from_world, const int32_t* num_agent, const double* dirs,
                             const float* range_jitter, int n_scenes, int n_agents, int k, int n_rays, double max_range,
                             double ground_z, int keep_ground, int min_points, double half_extent, int gt_rows, float* points,
                             int32_t* hit, int32_t* solid_hits, float* gt_boxes, int32_t* gt_count, int32_t* gt_own_hits,
                             void* stream) {
  return lidar_scan(solids, solid_count, object_count, sensor_from_world, num_agent, dirs, range_jitter, n_scenes, n_agents,
                    k, n_rays, max_range, ground_z, keep_ground, min_points, half_extent, gt_rows, points, hit, solid_hits,
                    gt_boxes, gt_count, gt_own_hits, nullptr, stream);
}

extern "C" int dn_lidar_scan_ids(const double* solids, const int32_t* solid_count, const int32_t* object_count,
                                 const double* sensor_from_world, const int32_t* num_agent, const double* dirs,
                                 const float* range_jitter, int n_scenes, int n_agents, int k, int n_rays, double max_range,
                                 double ground_z, int keep_ground, int min_points, double half_extent, int gt_rows,
                                 float* points, int32_t* hit, int32_t* solid_hits, float* gt_boxes, int32_t* gt_count,
                                 int32_t* gt_own_hits, int32_t* gt_ids, void* stream) {
  DN_REQUIRE(gt_ids, "lidar_scan_ids: null gt_ids");
  return lidar_scan(solids, solid_count, object_count, sensor_from_world, num_agent, dirs, range_jitter, n_scenes, n_agents,
                    k, n_rays, max_range, ground_z, keep_ground, min_points, half_extent, gt_rows, points, hit, solid_hits,
                    gt_boxes, gt_count, gt_own_hits, gt_ids, stream);
}
