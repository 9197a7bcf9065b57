// Lidar sequences (dn_lidar_world_step): the world of dn_lidar_scan at frame f -- the solids moved, every sensor's
// sensor_from_world and the scene's trans_matrices -- computed on the device from the frame-0 description, so that a
// sequence is F replays of one captured graph with nothing uploaded between them.  The contract is in
// include/disconet_hip.h; the host statement that defines the bytes is lidar.host_world_step.  Motion is closed-form
// (state(f) depends on f only), all of it fp64 with + - * only, and every function that computes it carries
// `#pragma clang fp contract(off)`.
//
// lidar_world_kernel   grid S, one workgroup per scene, 256 lanes.  Every lane reads the scene's cursor, then the barrier,
//                      then lane 0 writes cursor + 1: no lane can read the advanced value, and no workgroup touches another
//                      scene's cursor.  Solids are one row per lane (K <= 256); agents and the A x A pairs are strided over
//                      the lanes.  A pair's lane recomputes agent i's six pose entries from the frame-0 row (the same
//                      operations, so the same bytes as the sensor_from_world it stands for) and reads nothing that
//                      another lane wrote.
#include "dn_internal.h"

namespace {

constexpr int kThreads = 256;
static_assert(DN_LIDAR_MAX_SOLIDS <= kThreads, "one solid per lane");

struct Pose {
  double x, y, sn, cs;         // the sensor's world pose at the frame
  double t00, t01, t03, t10, t11, t13;
};

__device__ __forceinline__ Pose pose_at(const double* agent0, const double* vel, double t) {
#pragma clang fp contract(off)
  Pose p;
  p.x = agent0[0] + t * vel[0];
  p.y = agent0[1] + t * vel[1];
  p.sn = agent0[2];
  p.cs = agent0[3];
  p.t00 = p.cs;
  p.t01 = p.sn;
  p.t03 = -((p.cs * p.x) + (p.sn * p.y));
  p.t10 = -p.sn;
  p.t11 = p.cs;
  p.t13 = (p.sn * p.x) - (p.cs * p.y);
  return p;
}

__global__ void __launch_bounds__(kThreads)
lidar_world_kernel(const long long* __restrict__ solids0, const double* __restrict__ solid_vel,
                   const int32_t* __restrict__ solid_count, const double* __restrict__ agent0,
                   const double* __restrict__ agent_vel, int32_t* frame, int A, int K, long long* __restrict__ solids,
                   double* __restrict__ sensor_from_world, float* __restrict__ trans) {
#pragma clang fp contract(off)
  const int tid = threadIdx.x, s = blockIdx.x;
  const int32_t f = frame[s];
  __syncthreads();
  if (tid == 0) frame[s] = (int32_t)((uint32_t)f + 1u);
  const double t = (double)f;

  if (tid < K) {
    int n = solid_count[s];
    n = n < 0 ? 0 : (n > K ? K : n);
    const long long* src = solids0 + ((size_t)s * K + tid) * 8;      // the rows as 64-bit words, on both sides: what is
    long long* dst = solids + ((size_t)s * K + tid) * 8;             // copied never passes through a double
    if (tid < n) {
      const double* v = solid_vel + ((size_t)s * K + tid) * 2;
      dst[0] = __double_as_longlong(__longlong_as_double(src[0]) + t * v[0]);
      dst[1] = __double_as_longlong(__longlong_as_double(src[1]) + t * v[1]);
    } else {                                                   // beyond the count: bytes, no arithmetic
      dst[0] = src[0];
      dst[1] = src[1];
    }
#pragma unroll
    for (int c = 2; c < 8; ++c) dst[c] = src[c];
  }

  const double* ag = agent0 + (size_t)s * A * 4;
  const double* av = agent_vel + (size_t)s * A * 2;
  for (int a = tid; a < A; a += kThreads) {
    const Pose p = pose_at(ag + 4 * a, av + 2 * a, t);
    double* T = sensor_from_world + ((size_t)s * A + a) * 16;
    T[0] = p.t00; T[1] = p.t01; T[2] = 0.0; T[3] = p.t03;
    T[4] = p.t10; T[5] = p.t11; T[6] = 0.0; T[7] = p.t13;
    T[8] = 0.0; T[9] = 0.0; T[10] = 1.0; T[11] = 0.0;
    T[12] = 0.0; T[13] = 0.0; T[14] = 0.0; T[15] = 1.0;
  }

  const long long pairs = (long long)A * A;
  for (long long e = tid; e < pairs; e += kThreads) {
    const int i = (int)(e / A), j = (int)(e - (long long)i * A);
    float r00 = 1.0f, r01 = 0.0f, r03 = 0.0f, r10 = 0.0f, r11 = 1.0f, r13 = 0.0f;
    if (i != j) {
      const Pose ti = pose_at(ag + 4 * i, av + 2 * i, t), pj = pose_at(ag + 4 * j, av + 2 * j, t);
      r00 = (float)(ti.t00 * pj.cs + ti.t01 * pj.sn);
      r01 = (float)(ti.t01 * pj.cs - ti.t00 * pj.sn);
      r10 = (float)(ti.t10 * pj.cs + ti.t11 * pj.sn);
      r11 = (float)(ti.t11 * pj.cs - ti.t10 * pj.sn);
      r03 = (float)((ti.t00 * pj.x + ti.t01 * pj.y) + ti.t03);
      r13 = (float)((ti.t10 * pj.x + ti.t11 * pj.y) + ti.t13);
    }
    float* R = trans + ((size_t)s * pairs + (size_t)e) * 16;
    R[0] = r00; R[1] = r01; R[2] = 0.0f; R[3] = r03;
    R[4] = r10; R[5] = r11; R[6] = 0.0f; R[7] = r13;
    R[8] = 0.0f; R[9] = 0.0f; R[10] = 1.0f; R[11] = 0.0f;
    R[12] = 0.0f; R[13] = 0.0f; R[14] = 0.0f; R[15] = 1.0f;
  }
}

}  // namespace

extern "C" int dn_lidar_world_step(const double* solids0, const double* solid_vel, const int32_t* solid_count,
                                   const double* agent0, const double* agent_vel, int32_t* frame, int n_scenes,
                                   int n_agents, int k, double* solids, double* sensor_from_world, float* trans,
                                   void* stream) {
  DN_REQUIRE(k >= 0 && k <= DN_LIDAR_MAX_SOLIDS, "lidar_world_step: K = %d solids, must be in [0, %d]", k,
             DN_LIDAR_MAX_SOLIDS);
  DN_REQUIRE(n_scenes >= 1 && n_agents >= 1, "lidar_world_step: S = %d, A = %d, both must be >= 1", n_scenes, n_agents);
  DN_REQUIRE((solids0 && solid_vel && solids) || k == 0, "lidar_world_step: null solids0 / solid_vel / solids");
  DN_REQUIRE(solid_count, "lidar_world_step: null solid_count");
  DN_REQUIRE(agent0 && agent_vel, "lidar_world_step: null agent0 / agent_vel");
  DN_REQUIRE(frame, "lidar_world_step: null frame");
  DN_REQUIRE(sensor_from_world && trans, "lidar_world_step: null sensor_from_world / trans");
  hipLaunchKernelGGL(lidar_world_kernel, dim3(n_scenes), dim3(kThreads), 0, (hipStream_t)stream,
                     reinterpret_cast<const long long*>(solids0), solid_vel, solid_count, agent0, agent_vel, frame, n_agents, k,
                     reinterpret_cast<long long*>(solids), sensor_from_world, trans);
  return dn::check_launch("lidar_world_kernel");
}
