// Training-step kernels around the convs (include/disconet_train.h): batch-norm in
// training mode and its backward, bias / channel sums, the training form of the
// DiscoGraph fusion tail, the detection loss and Adam.  All HBM-bound row-major
// streaming over NHWC maps: lanes run along the channel axis (coalesced rows),
// per-channel sums are kept in double (the batch variance is E[z^2] - mean^2 over
// up to 1.3 M pixels) in LDS per workgroup and merged with one double atomic per
// (workgroup, channel).
//
// Replaces the autograd graph of upstream:coperception/utils/CoDetModule.py :: step
// (nn.BatchNorm2d / BatchNorm3d in train(), F.relu, torch.exp / div / mul of the fusion
// loop in upstream:.../det/DiscoNet.py :: forward, loss.py's focal / smooth-L1 losses,
// torch.optim.Adam).
#include <hip/hip_runtime.h>

#include <cstdlib>

#include <cmath>
#include <initializer_list>
#include <type_traits>

#include "agent_device.h"
#include "decode_device.h"
#include "disconet_train.h"
#include "dn_internal.h"
#include "sp_layout.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int kMaxC = 512;      // channels of the widest map on the path (conv4_*)

__device__ inline int lanes_for(int c) {   // power-of-two channel lanes per row, <= 64
  int t = 1;
  while (t < c && t < 64) t <<= 1;
  return t;
}

// loss VALUES only (det_loss_kernel, kd_kl_kernel): one f64 atomic per workgroup; the reported scalar may differ in
// its last bits between runs, no gradient or parameter depends on it
__device__ inline void atomic_add_f64(double* p, double v) { atomicAdd(p, v); }

// V channels of one pixel, held by one thread: a float (any c, stride, alignment) or a float4 (c % 4 == 0, 16-byte aligned rows)
template <int V> struct vec_of { typedef float type; };
template <> struct vec_of<4> { typedef f32x4 type; };
template <int V> using vec = typename vec_of<V>::type;
template <int V> __device__ inline vec<V> ldv(const float* p) { return *reinterpret_cast<const vec<V>*>(p); }
template <int V> __device__ inline void stv(float* p, const vec<V> v) { *reinterpret_cast<vec<V>*>(p) = v; }
__device__ inline f32x4 ldv4(const float* p) { return ldv<4>(p); }
__device__ inline float lane(float v, int) { return v; }
__device__ inline float lane(const f32x4 v, int e) { return v[e]; }
__device__ inline void set_lane(float& v, int, float x) { v = x; }
__device__ inline void set_lane(f32x4& v, int e, float x) { v[e] = x; }

// ---------------------------------------------------------------------------------
// per-(group, channel) sums of up to two quantities over the rows of a group -- DETERMINISTIC: the rows a thread
// adds, the order in which a workgroup adds its threads' partials (LDS, by row-lane index) and the order in which
// the workgroups' partials are added (fold, by block index) are all fixed by the launch shape,
// so two runs of a training step produce the same bits (round 2 used f64 atomics in LDS and in global memory).
// ---------------------------------------------------------------------------------
// F(row_in_group, first channel, &q0, &q1) yields the two addends of V channels; grid = (blocks per group, groups).  The
// workgroup's partial goes to part_g[blockIdx.x * NQ * c + q * c + channel].  Lanes run over groups of V channels.
// U: rows a thread fetches before it adds them.  The adds stay in row order (the same sums, bit for bit, as U = 1), but U rows'
// loads are in flight at once: with one row per iteration the kernels moved 3.8-4.5 TB/s, bound by bytes in flight per CU
// (16 waves x 64 lanes x 2 loads of 16 B against ~2 us of HBM latency), not by the HBM (round 5, profiles/r05_train_pmc.txt).
// SQ (the batch statistics): the second quantity is q0 * q0 TAKEN IN DOUBLE -- a float x float product is exact there, so the sum
// of squares carries no fp32 rounding of numbers of size mean^2 (squared in fp32, var = E[z^2] - mean^2 lost 2^-24 mean^2: 2e-3 of
// a variance of 1 at a mean of 1000); F leaves q1 alone.
constexpr int kRedSlots = 2048;     // ty_n * c <= 2048 for every launch shape (c <= kMaxC)
template <int NQ, int V, int U, bool SQ = false, class F>
__device__ inline void group_channel_sums(int c, long rows_per_group, double* part_g, F f) {
  __shared__ double red[2][kRedSlots];
  const int cvn = V == 4 ? c >> 2 : c;
  const int tx_n = lanes_for(cvn), ty_n = blockDim.x / tx_n;
  const int tx = threadIdx.x % tx_n, ty = threadIdx.x / tx_n;
  const long chunk = (rows_per_group + gridDim.x - 1) / gridDim.x;
  const long r0 = blockIdx.x * chunk;
  const long r1 = r0 + chunk < rows_per_group ? r0 + chunk : rows_per_group;
  for (int cv = tx; cv < cvn; cv += tx_n) {
    double s0[V], s1[V];
#pragma unroll
    for (int e = 0; e < V; ++e) s0[e] = s1[e] = 0.0;
    const auto add = [&](const vec<V> q0, const vec<V> q1) {
#pragma unroll
      for (int e = 0; e < V; ++e) {
        s0[e] += lane(q0, e);
        if constexpr (SQ) s1[e] = __builtin_fma((double)lane(q0, e), (double)lane(q0, e), s1[e]);
        else if (NQ > 1) s1[e] += lane(q1, e);
      }
    };
    long r = r0 + ty;
    if constexpr (U > 1) {
      for (; r + (long)(U - 1) * ty_n < r1; r += (long)U * ty_n) {
        vec<V> q0[U], q1[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          q1[u] = vec<V>{};
          f(r + (long)u * ty_n, V * cv, q0[u], q1[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) add(q0[u], q1[u]);
      }
    }
    for (; r < r1; r += ty_n) {
      vec<V> q0, q1 = vec<V>{};
      f(r, V * cv, q0, q1);
      add(q0, q1);
    }
#pragma unroll
    for (int e = 0; e < V; ++e) {
      red[0][ty * c + V * cv + e] = s0[e];
      if (NQ > 1) red[1][ty * c + V * cv + e] = s1[e];
    }
  }
  __syncthreads();
  double* out = part_g + (size_t)blockIdx.x * NQ * c;
  for (int i = threadIdx.x; i < NQ * c; i += blockDim.x) {
    const int q = i / c, cc = i % c;
    double t = 0.0;
    for (int y = 0; y < ty_n; ++y) t += red[q][y * c + cc];
    out[i] = t;
  }
}

// t[q] = sum over the blocks b of p[b * stride + q * q_stride]   (NQ quantities of one channel: the same blocks), in a FIXED
// order: one wavefront per output; lane l adds blocks l, l + 64, l + 128, ... in that order, then the 64 lane sums go through a
// xor butterfly (a fixed tree).  (A single thread walking up to 2048 partials was a 1 ms serial chain per reduction.)
// FOLD_BATCH: partials a lane fetches before it adds them (in the same order: the same bits), all NQ fetches of a batch in
// flight together.  With one load per iteration a lane's up to 16 partials were 16 L2 round trips in a row: 7-11 us per launch,
// 72 launches per step (profiles/r06_fold_batch_ab.txt).
constexpr int FOLD_BATCH = 8;
template <int NQ>
__device__ inline void fold(const double* __restrict__ p, size_t q_stride, int n_blocks, size_t stride, int lane, double (&t)[NQ]) {
#pragma unroll
  for (int q = 0; q < NQ; ++q) t[q] = 0.0;
  int b = lane;
  for (; b + 64 * (FOLD_BATCH - 1) < n_blocks; b += 64 * FOLD_BATCH) {
    double v[FOLD_BATCH][NQ];
#pragma unroll
    for (int u = 0; u < FOLD_BATCH; ++u)
#pragma unroll
      for (int q = 0; q < NQ; ++q) v[u][q] = p[(size_t)(b + 64 * u) * stride + q * q_stride];
#pragma unroll
    for (int u = 0; u < FOLD_BATCH; ++u)
#pragma unroll
      for (int q = 0; q < NQ; ++q) t[q] += v[u][q];
  }
  for (; b < n_blocks; b += 64) {
    double v[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) v[q] = p[(size_t)b * stride + q * q_stride];
#pragma unroll
    for (int q = 0; q < NQ; ++q) t[q] += v[q];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
#pragma unroll
    for (int q = 0; q < NQ; ++q) t[q] += __shfl_xor(t[q], o, 64);
}

// ---- what a fold's sums become: each rule once, called by the standalone kernel (two-phase and multi-group paths) and by the
// fused fold kernel (one launch instead of a fold and a 3-5 us finish launch behind it)
// batch statistics of one (group, channel) from its sums of z and z^2 over `rows` rows
__device__ inline void bn_stats_finish(double s0, double s1, long rows, float& mean, float& var) {
  const double m = s0 / rows;
  const double v = __builtin_fma(-m, m, s1 / rows);
  mean = (float)m;
  var = (float)(v > 0.0 ? v : 0.0);
}
// one group's step of the running statistics.  Every product is rounded (no contraction): which of the two products of a sum
// hipcc fused differed between the fused kernel (neither) and the first of bn_update_running_kernel's eight unrolled steps.
__device__ inline float bn_unbias(long rows) { return rows > 1 ? (float)rows / (float)(rows - 1) : 1.f; }
__device__ inline void bn_running_step(float& rm, float& rv, float mean, float var, float unbias, float momentum) {
#pragma clang fp contract(off)
  rm = (1.f - momentum) * rm + momentum * mean;
  rv = (1.f - momentum) * rv + momentum * (var * unbias);
}
// a finished per-channel sum into its fp32 gradient (dgamma, dbeta, bias gradients)
__device__ inline void store_channel_sum(float* __restrict__ out, int cc, double s, int accumulate) {
  out[cc] = (accumulate ? out[cc] : 0.f) + (float)s;
}

// sums[g][i] = sum over the group's blocks of part[g][blk][i]   (i < per = NQ * c)
__global__ void __launch_bounds__(256) fold_partials_kernel(const double* __restrict__ part, int n_blocks, int per,
                                                            int n_groups, double* __restrict__ sums) {
  const int idx = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (idx >= n_groups * per) return;
  const int g = idx / per, i = idx % per;
  double t[1];
  fold<1>(part + (size_t)g * n_blocks * per + i, 0, n_blocks, per, lane, t);
  if (lane == 0) sums[idx] = t[0];
}

__global__ void bn_stats_finalize_kernel(const double* __restrict__ sums, int n, int c, long rows,
                                         float* __restrict__ mean, float* __restrict__ var) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;   // (group, channel)
  if (i >= n) return;
  const int g = i / c, cc = i % c;
  bn_stats_finish(sums[(size_t)g * 2 * c + cc], sums[(size_t)g * 2 * c + c + cc], rows, mean[i], var[i]);
}

__global__ void bn_update_running_kernel(const float* __restrict__ mean, const float* __restrict__ var,
                                         int n_groups, long rows, int c, const int* __restrict__ order,
                                         float momentum, float* __restrict__ rmean,
                                         float* __restrict__ rvar) {
  const int cc = blockIdx.x * blockDim.x + threadIdx.x;
  if (cc >= c) return;
  float rm = rmean[cc], rv = rvar[cc];
  const float unbias = bn_unbias(rows);
  // the recurrence runs in group order; the groups' statistics are fetched eight at a time (one round trip instead of eight)
  for (int k0 = 0; k0 < n_groups; k0 += 8) {
    float m[8], v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int k = k0 + u < n_groups ? k0 + u : n_groups - 1;
      const int g = order ? order[k] : k;
      m[u] = mean[g * c + cc];
      v[u] = var[g * c + cc];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (k0 + u < n_groups) bn_running_step(rm, rv, m[u], v[u], unbias, momentum);
  }
  rmean[cc] = rm;
  rvar[cc] = rv;
}

__global__ void bn_param_grad_kernel(const double* __restrict__ sums, int n_groups, int c,
                                     float* __restrict__ dgamma, float* __restrict__ dbeta,
                                     int accumulate) {
  const int cc = blockIdx.x * blockDim.x + threadIdx.x;
  if (cc >= c) return;
  double s1 = 0.0, s2 = 0.0;
  int g = 0;
  for (; g + 7 < n_groups; g += 8) {      // group order, eight groups' sums in flight
    double a[8], b[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      a[u] = sums[(size_t)(g + u) * 2 * c + cc];
      b[u] = sums[(size_t)(g + u) * 2 * c + c + cc];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      s1 += a[u];
      s2 += b[u];
    }
  }
  for (; g < n_groups; ++g) {
    s1 += sums[(size_t)g * 2 * c + cc];
    s2 += sums[(size_t)g * 2 * c + c + cc];
  }
  store_channel_sum(dbeta, cc, s1, accumulate);
  store_channel_sum(dgamma, cc, s2, accumulate);
}

// ---- fold + finish in ONE launch (round 6: the step ran ~75 fold_partials launches of 6.7 us each plus as many finish launches
// behind them).  One wavefront per (group, channel) folds BOTH quantities of its channel, lane 0 finishes them.
__global__ void __launch_bounds__(256)
fold_stats_finish_kernel(const double* __restrict__ part, int n_blocks, int c, int n_groups, long norm_rows, double* __restrict__ sums,
                         float* __restrict__ mean, float* __restrict__ var, float* __restrict__ rmean, float* __restrict__ rvar,
                         float momentum, long unbias_rows) {
  const int idx = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (idx >= n_groups * c) return;
  const int g = idx / c, cc = idx % c;
  double t[2];
  fold<2>(part + (size_t)g * n_blocks * 2 * c + cc, c, n_blocks, 2 * c, lane, t);
  if (lane == 0) {
    sums[(size_t)g * 2 * c + cc] = t[0];
    sums[(size_t)g * 2 * c + c + cc] = t[1];
    float mf, vf;
    bn_stats_finish(t[0], t[1], norm_rows, mf, vf);
    mean[idx] = mf;
    var[idx] = vf;
    if (rmean) {      // one group
      float rm = rmean[cc], rv = rvar[cc];
      bn_running_step(rm, rv, mf, vf, bn_unbias(unbias_rows), momentum);
      rmean[cc] = rm;
      rvar[cc] = rv;
    }
  }
}
__global__ void __launch_bounds__(256)
fold_param_grad_kernel(const double* __restrict__ part, int n_blocks, int c, double* __restrict__ sums, float* __restrict__ dgamma,
                       float* __restrict__ dbeta, int accumulate) {      // one group
  const int cc = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (cc >= c) return;
  double t[2];
  fold<2>(part + cc, c, n_blocks, 2 * c, lane, t);
  if (lane == 0) {
    sums[cc] = t[0];
    sums[c + cc] = t[1];
    store_channel_sum(dbeta, cc, t[0], accumulate);
    store_channel_sum(dgamma, cc, t[1], accumulate);
  }
}
__global__ void __launch_bounds__(256)
fold_channel_sum_kernel(const double* __restrict__ part, int n_blocks, int c, double* __restrict__ sums, float* __restrict__ out,
                        int accumulate) {
  const int cc = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (cc >= c) return;
  double t[1];
  fold<1>(part + cc, 0, n_blocks, c, lane, t);
  if (lane == 0) {
    sums[cc] = t[0];
    store_channel_sum(out, cc, t[0], accumulate);
  }
}

// ---- the channel-sum folds of a whole backward pass in ONE launch (dn_channel_sum_fold_multi).  The sums they finish -- bias
// gradients: leaves of the backward -- are not read before the optimizer step, so the launches that leave the partials
// (dn_bn_bwd_out.n_blocks, dn_channel_sum_partial) need not be followed by a fold each (26 launches of
// 5 us per step).  Jobs ride in the kernel arguments; one wavefront per (job, channel).
constexpr int kFoldJobs = 32;
struct FoldJobs {
  const double* part[kFoldJobs];
  double* sums[kFoldJobs];
  float* out[kFoldJobs];
  int n_blocks[kFoldJobs], c[kFoldJobs], accumulate[kFoldJobs];
  int first[kFoldJobs + 1];      // first wavefront of job j; first[n_jobs] = all wavefronts
};
__global__ void __launch_bounds__(256) fold_channel_sum_multi_kernel(const FoldJobs J, int n_jobs) {
  const int wv = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (wv >= J.first[n_jobs]) return;
  int j = 0;
  while (j + 1 < n_jobs && J.first[j + 1] <= wv) ++j;      // wave-uniform
  const int cc = wv - J.first[j], c = J.c[j];
  double t[1];
  fold<1>(J.part[j] + cc, 0, J.n_blocks[j], c, lane, t);
  if (lane == 0) {
    J.sums[j][cc] = t[0];
    store_channel_sum(J.out[j], cc, t[0], J.accumulate[j]);
  }
}

// ---- the BatchNorm elements: each expression once, for V = 1 or 4 channels (T: float or f32x4)
template <int V>
__device__ inline vec<V> bn_rstd(const float* var, float eps) {
  const vec<V> v = ldv<V>(var);
  vec<V> r;
#pragma unroll
  for (int e = 0; e < V; ++e) set_lane(r, e, 1.f / sqrtf(lane(v, e) + eps));
  return r;
}
template <class T> __device__ inline T bn_zhat(T z, T mean, T rstd) { return (z - mean) * rstd; }
// The fused multiply-adds are spelled out.  Left to contraction, hipcc paired zhat * m2 with gamma * rstd into one packed
// multiply in the scalar backward kernel and the subtraction stayed unfused: other bits than the float4 kernels'.
template <class T> __device__ inline T bn_fwd_element(T z, T mean, T rstd, T gamma, T beta) {
  return __builtin_elementwise_fma(bn_zhat(z, mean, rstd), gamma, beta);
}
// g: the incoming gradient; m1, m2: the group's means of g and g * zhat
template <class T> __device__ inline T bn_bwd_element(T z, T mean, T rstd, T gamma, T g, T m1, T m2) {
  return gamma * rstd * __builtin_elementwise_fma(-bn_zhat(z, mean, rstd), m2, g - m1);
}
// a mean of the backward: double sum / norm_rows, rounded to float
template <int V>
__device__ inline vec<V> bn_bwd_mean(const double* sums, long norm_rows) {
  vec<V> m;
#pragma unroll
  for (int e = 0; e < V; ++e) set_lane(m, e, (float)(sums[e] / norm_rows));
  return m;
}

// The flat index of an apply kernel over [rows][c / V] into (row, first channel, group).  General: two 64-bit divisions.
// FAST (one group, c / 4 = 1 << sh, fewer than 2^31 float4s -- every BatchNorm of the conv stack): a shift and a mask.
template <bool FAST> using bn_index = std::conditional_t<FAST, unsigned, long>;
template <int V, bool FAST>
__device__ inline void bn_decode(bn_index<FAST> idx, int c, int sh, long rows_per_group, bn_index<FAST>& row, int& cc, int& g) {
  if constexpr (FAST) {
    row = idx >> sh;
    cc = V * (int)(idx & ((1u << sh) - 1u));
    g = 0;
  } else {
    const int cvn = V == 4 ? c >> 2 : c;
    row = idx / cvn;
    cc = V * (int)(idx % cvn);
    g = (int)(row / rows_per_group);
  }
}

// The SP copy of a BatchNorm output (sp_layout.h: [image][c / 16][4 quarters][hw] x 16 bytes), vector form of sp_split.h ::
// split over the four channels 4 c4 .. 4 c4 + 3 of pixel `row` a thread holds.  A piece is 8 channels of one pixel = the values
// of TWO adjacent threads (c % 16 == 0: an even / odd pair never straddles a wavefront or the end of the loop, and there is no
// padded octet to zero): they swap halves, the even thread writes the hi piece, the odd one the lo piece.  amax: running max of
// the clamped magnitudes, for sp_note_range.  Called by every thread of the pair (the swap is a cross-lane read).
__device__ inline void sp_store_quad(const f32x4 v, float& amax, unsigned char* __restrict__ out, unsigned row, unsigned hw,
                                     int c4, int c) {
  typedef _Float16 h4 __attribute__((ext_vector_type(4)));
  typedef unsigned u2 __attribute__((ext_vector_type(2)));
  typedef unsigned u4 __attribute__((ext_vector_type(4)));
  f32x4 x;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    x[e] = fminf(fmaxf(v[e], -65504.f), 65504.f);
    amax = fmaxf(amax, fabsf(x[e]));
  }
  const h4 hi = __builtin_convertvector(x, h4);
  const h4 lo = __builtin_convertvector(x - __builtin_convertvector(hi, f32x4), h4);
  const u2 hu = __builtin_bit_cast(u2, hi), lu = __builtin_bit_cast(u2, lo);
  const bool odd = c4 & 1;
  // the even thread needs its partner's hi halves, the odd one its partner's lo halves
  const unsigned t0 = __shfl_xor(odd ? hu[0] : lu[0], 1), t1 = __shfl_xor(odd ? hu[1] : lu[1], 1);
  const u4 piece = odd ? u4{t0, t1, lu[0], lu[1]} : u4{hu[0], hu[1], t0, t1};
  const unsigned img = row / hw, px = row - img * hw;
  const int oct8 = c4 >> 1;
  *reinterpret_cast<u4*>(out + sp::act_piece(img, c >> 4, oct8 >> 1, sp::quarter_of(odd, oct8 & 1), hw, px) * 16) = piece;
}
// magnitudes of split values, into the conv engine's sticky range word (sp_device.h :: note_range's rule)
__device__ inline void sp_note_range(float amax, unsigned* __restrict__ flags) {
  if (amax > 16384.f && flags) atomicOr(flags, amax >= 65504.f ? 3u : 2u);
}

// ---- forward apply: y = (z - mean) * rstd * gamma + beta, optionally the ReLU and its byte mask, optionally (SP) the SP copy
// of y -- the next layer's forward operand on the split-f16 engine.
// Where the per-channel constants come from: the general kernels compute them per element from global memory -- ~300 VALU
// instructions per float4 on two 64-bit divisions and four 1 / sqrtf: instruction-bound at ~4.8 TB/s, not HBM-bound (round 5:
// rocprofv3 counters, profiles/r05_train_pmc.txt).  FAST computes them once per workgroup into LDS, by the same functions.
// DN_BN_LEGACY=1 routes every call to the general kernels (tests: bitwise A/B).
template <int V, bool FAST, bool SP>
__device__ inline void bn_apply_body(const float* __restrict__ z, const float* __restrict__ mean, const float* __restrict__ var,
                                     const float* __restrict__ gamma, const float* __restrict__ beta, float eps, int relu,
                                     long rows_per_group, int c, int sh, int ldz, bn_index<FAST> total, float* __restrict__ y,
                                     unsigned char* __restrict__ relu_mask, unsigned char* __restrict__ y_sp, unsigned hw,
                                     unsigned* __restrict__ flags) {
  typedef bn_index<FAST> I;
  __shared__ __attribute__((aligned(16))) float rstd_s[FAST ? kMaxC : 4];
  if constexpr (FAST) {
    for (int i = threadIdx.x; i < c; i += 256) rstd_s[i] = bn_rstd<1>(var + i, eps);
    __syncthreads();
  }
  float amax = 0.f;
  for (I idx = blockIdx.x * (I)256 + threadIdx.x; idx < total; idx += gridDim.x * (I)256) {
    I row;
    int cc, g;
    bn_decode<V, FAST>(idx, c, sh, rows_per_group, row, cc, g);
    vec<V> rs;
    if constexpr (FAST) rs = ldv<V>(&rstd_s[cc]);
    else rs = bn_rstd<V>(var + g * c + cc, eps);
    vec<V> v = bn_fwd_element(ldv<V>(z + (size_t)row * ldz + cc), ldv<V>(mean + g * c + cc), rs, ldv<V>(gamma + cc), ldv<V>(beta + cc));
    if constexpr (V == 4) {
      // one byte per four channels: bit e = (y[cc + e] > 0), what the backward's ReLU gate asks of y -- 1/16 of y's bytes
      if (relu_mask) relu_mask[idx] = (unsigned char)((v[0] > 0.f) | ((v[1] > 0.f) << 1) | ((v[2] > 0.f) << 2) | ((v[3] > 0.f) << 3));
    }
    if (relu) {
#pragma unroll
      for (int e = 0; e < V; ++e) set_lane(v, e, fmaxf(lane(v, e), 0.f));
    }
    stv<V>(y + (size_t)row * c + cc, v);
    if constexpr (SP) sp_store_quad(v, amax, y_sp, row, hw, cc >> 2, c);
  }
  if constexpr (SP) sp_note_range(amax, flags);
}

__global__ void __launch_bounds__(256)
bn_apply_kernel(const float* __restrict__ z, const float* __restrict__ mean,
                const float* __restrict__ var, const float* __restrict__ gamma,
                const float* __restrict__ beta, float eps, int relu, long rows_per_group, int c,
                int ldz, long total, float* __restrict__ y) {
  bn_apply_body<1, false, false>(z, mean, var, gamma, beta, eps, relu, rows_per_group, c, 0, ldz, total, y, nullptr, nullptr, 1u, nullptr);
}
__global__ void __launch_bounds__(256)
bn_apply_v4_kernel(const float* __restrict__ z, const float* __restrict__ mean,
                   const float* __restrict__ var, const float* __restrict__ gamma,
                   const float* __restrict__ beta, float eps, int relu, long rows_per_group, int c,
                   int ldz, long total4, float* __restrict__ y, unsigned char* __restrict__ relu_mask) {
  bn_apply_body<4, false, false>(z, mean, var, gamma, beta, eps, relu, rows_per_group, c, 0, ldz, total4, y, relu_mask, nullptr, 1u, nullptr);
}
template <bool SP>
__global__ void __launch_bounds__(256)
bn_apply_v4_fast_kernel(const float* __restrict__ z, const float* __restrict__ mean, const float* __restrict__ var,
                        const float* __restrict__ gamma, const float* __restrict__ beta, float eps, int relu, int c, int sh,
                        int ldz, unsigned total4, float* __restrict__ y, unsigned char* __restrict__ relu_mask,
                        unsigned char* __restrict__ y_sp, unsigned hw, unsigned* __restrict__ flags) {
  bn_apply_body<4, true, SP>(z, mean, var, gamma, beta, eps, relu, 0L, c, sh, ldz, total4, y, relu_mask, y_sp, hw, flags);
}

// incoming gradient of one element: dy_a (dense, the 2 x 2 block sum of a map at twice the resolution, or the space-to-depth
// image of the gradient) + dy_b, gated by the ReLU
struct GradSrc {
  const float* dy_a;
  const float* dy_b;
  const float* y;
  int ld_a, up_a, ld_b, relu, h, w, c;
  // channels cc .. cc + V - 1 of pixel `row`.  R: long, or unsigned for rows below 2^31 (the one-group fast kernels): the same
  // values, the pixel decode in 32-bit arithmetic
  template <int V, class R>
  __device__ inline vec<V> load(R row, int cc) const {
    vec<V> g;
    if (up_a) {
      const R hw = (R)h * (R)w, img = row / hw;
      const unsigned p = (unsigned)(row % hw), py = p / (unsigned)w, px = p - py * (unsigned)w;
      if (up_a == 2) {
        // dy_a is the space-to-depth image of the gradient: [img][h / 2][w / 2][4 c], pixel (y, x) channel cc at
        // (y / 2, x / 2), channel ((y & 1) * 2 + (x & 1)) * c + cc -- what ONE split-f16 launch over the four parity classes of a
        // stride-2 layer's data gradient writes (train.py :: _dgrad)
        g = ldv<V>(dy_a + (((size_t)img * (h >> 1) + (py >> 1)) * (size_t)(w >> 1) + (px >> 1)) * ld_a + ((py & 1) * 2 + (px & 1)) * c + cc);
      } else {
        const float* b = dy_a + (((size_t)img * 2 * h + 2 * py) * (2L * w) + 2 * px) * ld_a + cc;
        g = (ldv<V>(b) + ldv<V>(b + ld_a)) + (ldv<V>(b + 2L * w * ld_a) + ldv<V>(b + (2L * w + 1) * ld_a));
      }
    } else {
      g = ldv<V>(dy_a + (size_t)row * ld_a + cc);
    }
    if (dy_b) g += ldv<V>(dy_b + (size_t)row * ld_b + cc);
    if (relu == 2) {          // y is the byte mask of dn_bn_train_apply (c % 4 == 0): bit cc & 3 of byte (row * c + cc) / 4
      const unsigned m = reinterpret_cast<const unsigned char*>(y)[((size_t)row * c + cc) >> 2] >> (cc & 3);
#pragma unroll
      for (int e = 0; e < V; ++e)
        if (!((m >> e) & 1)) set_lane(g, e, 0.f);
    } else if (relu) {
      const vec<V> yv = ldv<V>(y + (size_t)row * c + cc);
#pragma unroll
      for (int e = 0; e < V; ++e)
        if (!(lane(yv, e) > 0.f)) set_lane(g, e, 0.f);
    }
    return g;
  }
};

// ---- the reductions: each quantity's addend once, for V = 1 or 4 channels per lane
template <int V, int U>
__device__ inline void bn_stats_body(const float* __restrict__ z, long rows_per_group, int c, int ldz, double* __restrict__ sums) {
  const int g = blockIdx.y;
  const float* zg = z + (size_t)g * rows_per_group * ldz;
  group_channel_sums<2, V, U, true>(c, rows_per_group, sums + (size_t)g * gridDim.x * 2 * c,
                                    [&](long r, int cc, vec<V>& q0, vec<V>& q1) {
                                      q0 = ldv<V>(zg + r * ldz + cc);
                                      (void)q1;
                                    });
}
template <int V, int U>
__device__ inline void bn_bwd_reduce_body(const GradSrc& src, const float* __restrict__ z, const float* __restrict__ mean,
                                          const float* __restrict__ var, float eps, long rows_per_group, double* __restrict__ sums) {
  const int g = blockIdx.y, c = src.c;
  const long base = (long)g * rows_per_group;
  group_channel_sums<2, V, U>(c, rows_per_group, sums + (size_t)g * gridDim.x * 2 * c,
                              [&](long r, int cc, vec<V>& q0, vec<V>& q1) {
                                q0 = src.load<V>(base + r, cc);
                                q1 = q0 * bn_zhat(ldv<V>(z + (base + r) * c + cc), ldv<V>(mean + g * c + cc), bn_rstd<V>(var + g * c + cc, eps));
                              });
}
template <int V, int U>
__device__ inline void channel_sum_body(const float* __restrict__ x, long rows, int c, int ld, double* __restrict__ sums) {
  group_channel_sums<1, V, U>(c, rows, sums, [&](long r, int cc, vec<V>& q0, vec<V>& q1) {
    q0 = ldv<V>(x + r * ld + cc);
    (void)q1;
  });
}

__global__ void __launch_bounds__(256)
bn_stats_kernel(const float* __restrict__ z, long rows_per_group, int c, int ldz, double* __restrict__ sums) {
  bn_stats_body<1, 1>(z, rows_per_group, c, ldz, sums);
}
template <int U>
__global__ void __launch_bounds__(256)
bn_stats_v4_kernel(const float* __restrict__ z, long rows_per_group, int c, int ldz, double* __restrict__ sums) {
  bn_stats_body<4, U>(z, rows_per_group, c, ldz, sums);
}
__global__ void __launch_bounds__(256)
bn_bwd_reduce_kernel(GradSrc src, const float* __restrict__ z, const float* __restrict__ mean,
                     const float* __restrict__ var, float eps, long rows_per_group, double* __restrict__ sums) {
  bn_bwd_reduce_body<1, 1>(src, z, mean, var, eps, rows_per_group, sums);
}
template <int U>
__global__ void __launch_bounds__(256)
bn_bwd_reduce_v4_kernel(GradSrc src, const float* __restrict__ z, const float* __restrict__ mean,
                        const float* __restrict__ var, float eps, long rows_per_group, double* __restrict__ sums) {
  bn_bwd_reduce_body<4, U>(src, z, mean, var, eps, rows_per_group, sums);
}
__global__ void __launch_bounds__(256)
channel_sum_kernel(const float* __restrict__ x, long rows, int c, int ld, double* __restrict__ sums) {
  channel_sum_body<1, 1>(x, rows, c, ld, sums);
}
template <int U>
__global__ void __launch_bounds__(256)
channel_sum_v4_kernel(const float* __restrict__ x, long rows, int c, int ld, double* __restrict__ sums) {
  channel_sum_body<4, U>(x, rows, c, ld, sums);
}

// ---- backward apply: dz = gamma * rstd * (g - m1 - zhat * m2).  The per-channel constants (1 / sqrtf(var + eps) and the two
// means: eight fp64 divisions per float4 in the general kernels) and the index decode: as in bn_apply_body; FAST also decodes
// the incoming gradient's pixel in 32 bits.
// SP: a second copy of dz, multiplied by the power of two `sp_lift`, as the split-planar f16 hi / lo tensor of the inference conv
// engine -- the operand of the split-f16 data gradient (dn_spconv2d_nhwc) -- written by sp_store_quad, magnitudes reported into
// the conv engine's sticky range word (`flags`).  FAST only (round 6): dz may be NULL, the SP copy is then the only consumer's.
// BIAS (FAST only, round 6): the per-channel sums of dz -- the gradient of the conv bias in front of this BatchNorm -- leave this
// launch as one double per (workgroup, channel) in `bias_part` (folded in a fixed order: deterministic), instead of
// a dn_channel_sum pass that reads dz again (0.5 ms of the det step).  A thread's channel quad never changes (the
// grid stride is a multiple of c / 4): it adds its own dz values in fp32 in loop order, the workgroup adds the threads of a
// quad in thread order in double.
template <int V, bool FAST, bool SP, bool BIAS>
__device__ inline void bn_bwd_apply_body(const GradSrc& src, const float* __restrict__ z, const float* __restrict__ mean,
                                         const float* __restrict__ var, const float* __restrict__ gamma, float eps,
                                         long rows_per_group, long norm_rows, const double* __restrict__ sums, int sh,
                                         bn_index<FAST> total, float* __restrict__ dz, unsigned char* __restrict__ dz_sp,
                                         float sp_lift, unsigned hw, unsigned* __restrict__ flags, double* __restrict__ bias_part) {
  static_assert(FAST || !BIAS, "the bias partials are the fast form's");
  typedef bn_index<FAST> I;
  __shared__ __attribute__((aligned(16))) float rstd_s[FAST ? kMaxC : 4], m1_s[FAST ? kMaxC : 4], m2_s[FAST ? kMaxC : 4];
  const int c = src.c;
  if constexpr (FAST) {
    for (int i = threadIdx.x; i < c; i += 256) {
      rstd_s[i] = bn_rstd<1>(var + i, eps);
      m1_s[i] = bn_bwd_mean<1>(sums + i, norm_rows);
      m2_s[i] = bn_bwd_mean<1>(sums + c + i, norm_rows);
    }
    __syncthreads();
  }
  float amax = 0.f;
  vec<V> bsum = vec<V>{};
  for (I idx = blockIdx.x * (I)256 + threadIdx.x; idx < total; idx += gridDim.x * (I)256) {
    I row;
    int cc, g;
    bn_decode<V, FAST>(idx, c, sh, rows_per_group, row, cc, g);
    vec<V> rs, m1, m2;
    if constexpr (FAST) {
      rs = ldv<V>(&rstd_s[cc]);
      m1 = ldv<V>(&m1_s[cc]);
      m2 = ldv<V>(&m2_s[cc]);
    } else {
      rs = bn_rstd<V>(var + g * c + cc, eps);
      m1 = bn_bwd_mean<V>(sums + (size_t)g * 2 * c + cc, norm_rows);
      m2 = bn_bwd_mean<V>(sums + (size_t)g * 2 * c + c + cc, norm_rows);
    }
    const vec<V> v = bn_bwd_element(ldv<V>(z + (size_t)row * c + cc), ldv<V>(mean + g * c + cc), rs, ldv<V>(gamma + cc), src.load<V>(row, cc), m1, m2);
    if (!SP || dz) stv<V>(dz + (size_t)row * c + cc, v);
    if constexpr (BIAS) bsum += v;
    if constexpr (SP) sp_store_quad(v * sp_lift, amax, dz_sp, (unsigned)row, hw, cc >> 2, c);
  }
  if constexpr (SP) sp_note_range(amax, flags);
  if constexpr (BIAS) {
    __shared__ __attribute__((aligned(16))) float bred[256][4];
    stv<4>(bred[threadIdx.x], bsum);
    __syncthreads();
    const int c4n = 1 << sh;
    for (int cc = threadIdx.x; cc < c; cc += 256) {
      double t = 0.0;
      for (int k = cc >> 2; k < 256; k += c4n) t += (double)bred[k][cc & 3];      // the quad's threads, in thread order
      bias_part[(size_t)blockIdx.x * c + cc] = t;
    }
  }
}

__global__ void __launch_bounds__(256)
bn_bwd_apply_kernel(GradSrc src, const float* __restrict__ z, const float* __restrict__ mean,
                    const float* __restrict__ var, const float* __restrict__ gamma, float eps,
                    long rows_per_group, long norm_rows, const double* __restrict__ sums, long total,
                    float* __restrict__ dz) {
  bn_bwd_apply_body<1, false, false, false>(src, z, mean, var, gamma, eps, rows_per_group, norm_rows, sums, 0, total, dz, nullptr, 1.f, 1u, nullptr, nullptr);
}
template <bool SP>
__global__ void __launch_bounds__(256)
bn_bwd_apply_v4_kernel(GradSrc src, const float* __restrict__ z, const float* __restrict__ mean,
                       const float* __restrict__ var, const float* __restrict__ gamma, float eps,
                       long rows_per_group, long norm_rows, const double* __restrict__ sums, long total4,
                       float* __restrict__ dz, unsigned char* __restrict__ dz_sp, float sp_lift, unsigned hw,
                       unsigned* __restrict__ flags) {
  bn_bwd_apply_body<4, false, SP, false>(src, z, mean, var, gamma, eps, rows_per_group, norm_rows, sums, 0, total4, dz, dz_sp, sp_lift, hw, flags, nullptr);
}
template <bool SP, bool BIAS = false>
__global__ void __launch_bounds__(256)
bn_bwd_apply_v4_fast_kernel(GradSrc src, const float* __restrict__ z, const float* __restrict__ mean,
                            const float* __restrict__ var, const float* __restrict__ gamma, float eps, long norm_rows,
                            const double* __restrict__ sums, int sh, unsigned total4, float* __restrict__ dz,
                            unsigned char* __restrict__ dz_sp, float sp_lift, unsigned hw, unsigned* __restrict__ flags,
                            double* __restrict__ bias_part = nullptr) {
  bn_bwd_apply_body<4, true, SP, BIAS>(src, z, mean, var, gamma, eps, 0L, norm_rows, sums, sh, total4, dz, dz_sp, sp_lift, hw, flags, bias_part);
}

__global__ void add_rows_kernel(float* __restrict__ a, int ld_a, const float* __restrict__ b, int ld_b,
                                int c, long total) {
  for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < total;
       idx += (long)gridDim.x * blockDim.x) {
    const long row = idx / c;
    const int cc = (int)(idx % c);
    a[row * ld_a + cc] += b[row * ld_b + cc];
  }
}

// backward of F.interpolate(scale_factor=2, nearest) on its own: out[n, y, x, c] = sum of the 2 x 2
// block of the double-resolution gradient (a channel slice with row stride ld)
__global__ void upsample2_sum_kernel(const float* __restrict__ g, int ld, int h, int w, int c,
                                     long total, float* __restrict__ out) {
  for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < total;
       idx += (long)gridDim.x * blockDim.x) {
    const int cc = (int)(idx % c);
    long r = idx / c;
    const int px = (int)(r % w);
    r /= w;
    const int py = (int)(r % h);
    const long img = r / h;
    const float* b = g + ((img * 2 * h + 2 * py) * (2L * w) + 2 * px) * ld + cc;
    out[idx] = (b[0] + b[ld]) + (b[2L * w * ld] + b[(2L * w + 1) * ld]);
  }
}

// ---------------------------------------------------------------------------------
// fusion, training form
// ---------------------------------------------------------------------------------
__global__ void pair_add_ego_kernel(float* __restrict__ z1, const float* __restrict__ e,
                                    const int* __restrict__ ego_image, long per_image, long total) {
  for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < total;
       idx += (long)gridDim.x * blockDim.x) {
    const int p = (int)(idx / per_image);
    z1[idx] += e[(size_t)ego_image[p] * per_image + idx % per_image];
  }
}

__global__ void pair_sum_ego_kernel(const float* __restrict__ dz1, const int* __restrict__ first,
                                    const int* __restrict__ pairs, long per_image, long total,
                                    float* __restrict__ de) {
  for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < total;
       idx += (long)gridDim.x * blockDim.x) {
    const int img = (int)(idx / per_image);
    const long off = idx % per_image;
    float s = 0.f;
    for (int k = first[img]; k < first[img + 1]; ++k) s += dz1[(size_t)pairs[k] * per_image + off];
    de[idx] = s;
  }
}

constexpr int kMaxNbr = 16;

__device__ inline float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// one wavefront per (ego, pixel); lanes carry float4s of channels
__global__ void __launch_bounds__(256)
fuse_combine_kernel(const float* __restrict__ z4, const float* __restrict__ maps,
                    const int* __restrict__ first, const int* __restrict__ pair_index,
                    const int* __restrict__ map_image, const int* __restrict__ ego_out, int n_egos,
                    int hw, int c, float* __restrict__ weights, float* __restrict__ fused) {
  const int lane = threadIdx.x & 63;
  const long item = blockIdx.x * 4L + (threadIdx.x >> 6);
  if (item >= (long)n_egos * hw) return;
  const int e = (int)(item / hw), px = (int)(item % hw);
  const int k0 = first[e];
  int kn = first[e + 1] - k0;
  kn = kn < 0 ? 0 : (kn > kMaxNbr ? kMaxNbr : kn);   // the per-lane arrays hold kMaxNbr entries (host side: train.py refuses more agents)
  float wk[kMaxNbr];
  float sum = 0.f;
  for (int k = 0; k < kn; ++k) {
    const int p = pair_index[k0 + k];
    const float s = p >= 0 ? fmaxf(z4[(size_t)p * hw + px], 0.f) : 0.f;
    wk[k] = expf(s);
    sum += wk[k];
  }
  for (int k = 0; k < kn; ++k) {
    wk[k] = wk[k] / sum;
    const int p = pair_index[k0 + k];
    if (lane == 0 && p >= 0) weights[(size_t)p * hw + px] = wk[k];
  }
  float* out = fused + ((size_t)ego_out[e] * hw + px) * c;
  for (int c4 = lane; c4 < (c >> 2); c4 += 64) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < kn; ++k)
      acc += *reinterpret_cast<const f32x4*>(maps + ((size_t)map_image[k0 + k] * hw + px) * c + 4 * c4) * wk[k];
    *reinterpret_cast<f32x4*>(out + 4 * c4) = acc;
  }
}

__global__ void __launch_bounds__(256)
fuse_combine_bwd_kernel(const float* __restrict__ dfused, int ld_df, const float* __restrict__ z4,
                        const float* __restrict__ weights, const float* __restrict__ maps,
                        const int* __restrict__ first, const int* __restrict__ pair_index,
                        const int* __restrict__ map_image, const int* __restrict__ ego_out, int n_egos,
                        int hw, int c, float* __restrict__ dmaps, float* __restrict__ dz4) {
  const int lane = threadIdx.x & 63;
  const long item = blockIdx.x * 4L + (threadIdx.x >> 6);
  if (item >= (long)n_egos * hw) return;
  const int e = (int)(item / hw), px = (int)(item % hw);
  const int k0 = first[e];
  int kn = first[e + 1] - k0;
  kn = kn < 0 ? 0 : (kn > kMaxNbr ? kMaxNbr : kn);   // the per-lane arrays hold kMaxNbr entries (host side: train.py refuses more agents)
  const float* df = dfused + ((size_t)ego_out[e] * hw + px) * ld_df;
  float wk[kMaxNbr], dot[kMaxNbr];
  for (int k = 0; k < kn; ++k) {
    const int p = pair_index[k0 + k];
    wk[k] = p >= 0 ? weights[(size_t)p * hw + px] : 1.f;
    dot[k] = 0.f;
  }
  for (int c4 = lane; c4 < (c >> 2); c4 += 64) {
    const f32x4 g = *reinterpret_cast<const f32x4*>(df + 4 * c4);
    for (int k = 0; k < kn; ++k) {
      const size_t off = ((size_t)map_image[k0 + k] * hw + px) * c + 4 * c4;
      const f32x4 m = *reinterpret_cast<const f32x4*>(maps + off);
      dot[k] += (g[0] * m[0] + g[1] * m[1]) + (g[2] * m[2] + g[3] * m[3]);
      *reinterpret_cast<f32x4*>(dmaps + off) = g * wk[k];
    }
  }
  float mean = 0.f;
  for (int k = 0; k < kn; ++k) {
    dot[k] = wave_sum(dot[k]);
    mean += wk[k] * dot[k];
  }
  if (lane == 0)
    for (int k = 0; k < kn; ++k) {
      const int p = pair_index[k0 + k];
      if (p >= 0) {
        const size_t i = (size_t)p * hw + px;
        dz4[i] = z4[i] > 0.f ? wk[k] * (dot[k] - mean) : 0.f;
      }
    }
}

// ---- `--com agent` (include/disconet_train.h :: dn_agent_combine_lists): one scalar weight per list entry, in the order of
// agent_device.h -- the inference path's (agent_fuse.hip), so the same scores give the same bits
// one workgroup per ego; wave v takes the list entries v, v + 4, ...; lane l and lane l + 32 carry pixel l of a tile
__global__ void __launch_bounds__(256)
agent_list_weights_kernel(const float* __restrict__ z4, const float* __restrict__ w5, const float* __restrict__ b5,
                          const int* __restrict__ first, const int* __restrict__ pair_index, int hw,
                          float* __restrict__ weights) {
  __shared__ float a_s[agentw::kMaxList];
  const int e = blockIdx.x;
  const int k0 = first[e];
  int kn = first[e + 1] - k0;
  kn = kn < 0 ? 0 : (kn > agentw::kMaxList ? agentw::kMaxList : kn);   // (host side: train.py refuses longer lists)
  if (kn == 0) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 31;
  const int tiles = (hw + 31) / 32;
  for (int k = wave; k < kn; k += 4) {
    const int p = pair_index[k0 + k];
    float folded = 0.f;
    if (p >= 0) {
      const float* z = z4 + (size_t)p * hw;
      for (int t = 0; t < tiles; ++t) {
        const int px = t * 32 + li;
        const bool valid = px < hw;
        const float s = valid ? fmaxf(z[px], 0.f) : 0.f;
        const float ts = agentw::tile_sum32(agentw::score_term(s, valid ? w5[px] : 0.f, valid));
        folded = agentw::fold_tile(folded, ts, t == 0);
      }
    }
    if (lane == 0) a_s[k] = p >= 0 ? agentw::agent_scalar(folded, b5[0]) : 0.f;   // (an ego that is not live: alone in its list)
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float w[agentw::kMaxList];
    agentw::list_softmax(a_s, kn, w);
    for (int k = 0; k < kn; ++k) weights[k0 + k] = w[k];
  }
}

__global__ void __launch_bounds__(256)
agent_combine_lists_kernel(const float* __restrict__ maps, const float* __restrict__ weights, const int* __restrict__ first,
                           const int* __restrict__ map_image, const int* __restrict__ ego_out, long quads,
                           float* __restrict__ fused) {
  const int e = blockIdx.y;
  const int s = first[e], t = first[e + 1];
  if (t <= s) return;
  for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < quads; q += (long)gridDim.x * 256) {
    f32x4 acc = agentw::weigh(*reinterpret_cast<const f32x4*>(maps + ((size_t)map_image[s] * quads + q) * 4), weights[s]);
    for (int k = s + 1; k < t; ++k)
      acc = agentw::weigh_add(acc, *reinterpret_cast<const f32x4*>(maps + ((size_t)map_image[k] * quads + q) * 4), weights[k]);
    *reinterpret_cast<f32x4*>(fused + ((size_t)ego_out[e] * quads + q) * 4) = acc;
  }
}

__global__ void __launch_bounds__(256)
agent_combine_lists_bwd_kernel(const float* __restrict__ dfused, int ld, const float* __restrict__ weights,
                               const int* __restrict__ first, const int* __restrict__ map_image,
                               const int* __restrict__ ego_out, int hw, int c4n, float* __restrict__ dmaps) {
  const int e = blockIdx.y;
  const int s = first[e], t = first[e + 1];
  if (t <= s) return;
  const long quads = (long)hw * c4n;
  for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < quads; q += (long)gridDim.x * 256) {
    const long p = q / c4n;
    const int c4 = (int)(q - p * c4n);
    const f32x4 g = *reinterpret_cast<const f32x4*>(dfused + ((size_t)ego_out[e] * hw + p) * ld + 4 * c4);
    for (int k = s; k < t; ++k)
      *reinterpret_cast<f32x4*>(dmaps + ((size_t)map_image[k] * quads + q) * 4) = agentw::weigh(g, weights[k]);
  }
}

// ---------------------------------------------------------------------------------
// loss and optimiser
// ---------------------------------------------------------------------------------
// Softmax focal loss of one anchor, L = -a (1 - q)^gamma log q with q the softmax probability of the labelled class, in the
// log-softmax form of oracle/train_ref.py :: focal_loss: with x = z_other - z_target, log q = -softplus(x), q = sigmoid(-x) and
// 1 - q = sigmoid(x) -- each from e = exp(-|x|) <= 1, so nothing is clamped, nothing is divided by q and 1 - q does not cancel.
// (Up to dn_version 139 log q was logf(max(q, 1e-30)) of a float quotient and the gradient divided by that clamp: past a
// wrong-side gap of ln 1e30 = 69 the loss stopped growing and the gradient of a confidently wrong anchor fell to zero.)
//   dL/dz_target = a [gamma (1 - q)^gamma q log q - (1 - q)^(gamma + 1)],  dL/dz_other = -dL/dz_target
// The one formula of both loss kernels: their dcls agree bit for bit.
__device__ inline void focal_one(float z0, float z1, float lb0, float lb1, float alpha, float gamma, float inv_norm,
                                 float& d0, float& d1, double& l_cls) {
  const bool fg = lb1 > 0.5f;
  const bool any = fg || lb0 > 0.5f;      // an all-zero row is "don't care"
  d0 = 0.f; d1 = 0.f;
  if (any) {
    const float x = fg ? z0 - z1 : z1 - z0;
    const float a = fg ? alpha : 1.f - alpha;
    const float e = expf(-fabsf(x));
    const float big = 1.f / (1.f + e), small = e / (1.f + e);
    const float q = x > 0.f ? small : big;
    const float om = x > 0.f ? big : small;
    const float lq = -(fmaxf(x, 0.f) + log1pf(e));
    const float mod = gamma == 0.f ? 1.f : powf(om, gamma);
    const float dmod = gamma == 0.f ? 0.f : gamma * mod;      // (1 - q) d(mod)/d(1 - q)
    l_cls += (double)(-a * mod * lq);
    const float dt = a * (dmod * q * lq - mod * om) * inv_norm;
    d0 = fg ? -dt : dt;
    d1 = fg ? dt : -dt;
  }
}

__global__ void __launch_bounds__(256)
det_loss_kernel(const float* __restrict__ cls, const float* __restrict__ labels,
                const float* __restrict__ loc, const float* __restrict__ targets,
                const float* __restrict__ mask, long n, int code, float alpha, float gamma,
                float sigma, float inv_norm, double* __restrict__ losses, float* __restrict__ dcls,
                float* __restrict__ dloc) {
  double l_cls = 0.0, l_loc = 0.0;
  const float s2 = sigma * sigma;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    float d0, d1;
    focal_one(cls[2 * i], cls[2 * i + 1], labels[2 * i], labels[2 * i + 1], alpha, gamma, inv_norm, d0, d1, l_cls);
    dcls[2 * i] = d0;
    dcls[2 * i + 1] = d1;
    const float mk = mask[i];
    for (int k = 0; k < code; ++k) {
      const float d = loc[i * code + k] - targets[i * code + k];
      const float ad = fabsf(d);
      float l, g;
      if (ad <= 1.f / s2) {
        l = 0.5f * s2 * d * d;
        g = s2 * d;
      } else {
        l = ad - 0.5f / s2;
        g = d > 0.f ? 1.f : -1.f;
      }
      l_loc += (double)(mk * l);
      dloc[i * code + k] = mk * g * inv_norm;
    }
  }
  // workgroup reduction, one atomic per workgroup and loss
  __shared__ double red[2][256];
  red[0][threadIdx.x] = l_cls;
  red[1][threadIdx.x] = l_loc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) {
      red[0][threadIdx.x] += red[0][threadIdx.x + s];
      red[1][threadIdx.x] += red[1][threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    atomic_add_f64(&losses[0], red[0][0] * inv_norm);
    atomic_add_f64(&losses[1], red[1][0] * inv_norm);
  }
}


// The same loss on FLAT float4 streams (round 6: the per-anchor form moved 786 MB per step at 54 % of the HBM rate -- every lane
// read its anchor's six box codes at a 24-byte stride).  Loop A: two anchors' class logits / labels per float4; loop B: four
// consecutive elements of loc / targets per float4, the anchor of element e is e / code (mask gather).  The per-element formulas
// are det_loss_kernel's (focal_one above, the same smooth-L1 lines), so dcls / dloc are bit for bit its values; the loss VALUES
// are summed in another order (they already leave through one f64 atomic per workgroup).  n even, code * n % 4 == 0, 16-byte
// aligned tensors.
__global__ void __launch_bounds__(256)
det_loss_v4_kernel(const float* __restrict__ cls, const float* __restrict__ labels, const float* __restrict__ loc,
                   const float* __restrict__ targets, const float* __restrict__ mask, long n, int code, float alpha, float gamma,
                   float sigma, float inv_norm, double* __restrict__ losses, float* __restrict__ dcls, float* __restrict__ dloc) {
  double l_cls = 0.0, l_loc = 0.0;
  const float s2 = sigma * sigma;
  const long stride = (long)gridDim.x * blockDim.x, t0 = blockIdx.x * (long)blockDim.x + threadIdx.x;
  for (long i = t0; i < n / 2; i += stride) {
    const f32x4 z = ldv4(cls + 4 * i), lb = ldv4(labels + 4 * i);
    float d0, d1, d2, d3;
    focal_one(z[0], z[1], lb[0], lb[1], alpha, gamma, inv_norm, d0, d1, l_cls);
    focal_one(z[2], z[3], lb[2], lb[3], alpha, gamma, inv_norm, d2, d3, l_cls);
    *reinterpret_cast<f32x4*>(dcls + 4 * i) = f32x4{d0, d1, d2, d3};
  }
  const long m4 = n * code / 4;
  for (long i = t0; i < m4; i += stride) {
    const f32x4 x = ldv4(loc + 4 * i), tg = ldv4(targets + 4 * i);
    f32x4 g4;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float mk = mask[(4 * i + e) / code];
      const float d = x[e] - tg[e];
      const float ad = fabsf(d);
      float l, g;
      if (ad <= 1.f / s2) {
        l = 0.5f * s2 * d * d;
        g = s2 * d;
      } else {
        l = ad - 0.5f / s2;
        g = d > 0.f ? 1.f : -1.f;
      }
      l_loc += (double)(mk * l);
      g4[e] = mk * g * inv_norm;
    }
    *reinterpret_cast<f32x4*>(dloc + 4 * i) = g4;
  }
  __shared__ double red[2][256];
  red[0][threadIdx.x] = l_cls;
  red[1][threadIdx.x] = l_loc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) {
      red[0][threadIdx.x] += red[0][threadIdx.x + s];
      red[1][threadIdx.x] += red[1][threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    atomic_add_f64(&losses[0], red[0][0] * inv_norm);
    atomic_add_f64(&losses[1], red[1][0] * inv_norm);
  }
}

// ---- corner localisation loss (include/disconet_train.h :: dn_det_loss_corner) ----
// One assigned anchor: the predicted codes p and the target codes t are decoded against the anchor row a (dn::decode_box,
// the library's one decode expression), each box gives its four corners in postprocess._corners' order with the RAW
// (sin, cos) pair, and the value is the sum of the four corner distances.  g[0..5] = scale * d(value)/d(p) by the chain rule
// through the corners (d/d centre, d/d size, d/d pair) and the decode.  A distance of exactly 0 contributes no gradient
// (torch's sub-gradient of norm); nothing is clamped, a NaN or inf goes through.  The one formula of both kernels below: their
// dloc agree bit for bit.
__device__ __forceinline__ float corner_one(const float* __restrict__ a, const float* __restrict__ p, const float* __restrict__ t,
                                            float scale, float* __restrict__ g) {
  // no fused multiply-adds in THIS body (decode_box keeps its own): with loc == targets bitwise the two boxes' corner
  // expressions must round alike so that their difference is exactly 0, and both kernels must see the same roundings
#pragma clang fp contract(off)
  float bp[6], bt[6];
  dn::decode_box(a, p, bp);
  dn::decode_box(a, t, bt);
  const float hw = 0.5f * bp[2], hh = 0.5f * bp[3], s = bp[4], c = bp[5];
  const float tw = 0.5f * bt[2], th = 0.5f * bt[3], ts = bt[4], tc = bt[5];
  float sum = 0.f, gx = 0.f, gy = 0.f, gw = 0.f, gh = 0.f, gs = 0.f, gc = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {      // (-,-), (+,-), (+,+), (-,+)
    const float sx = (k == 1 || k == 2) ? 1.f : -1.f, sy = k >= 2 ? 1.f : -1.f;
    const float dx = sx * hw, dy = sy * hh, tdx = sx * tw, tdy = sy * th;
    // corner - corner with the two centres (up to 32 m, half an ulp = 1.9e-6) subtracted from each other first and the rotated
    // offsets (a few metres) apart from them: the sum the contract states, without a second rounding at the centres' magnitude
    // -- d / |d| below loses accuracy like 1 / |d|
    const float ex = (bp[0] - bt[0]) + ((dx * c - dy * s) - (tdx * tc - tdy * ts));
    const float ey = (bp[1] - bt[1]) + ((dx * s + dy * c) - (tdx * ts + tdy * tc));
    const float d = sqrtf(ex * ex + ey * ey);
    sum += d;
    const float ux = d == 0.f ? 0.f : ex / d, uy = d == 0.f ? 0.f : ey / d;
    gx += ux;
    gy += uy;
    gw += sx * (c * ux + s * uy);      // d corner / d w = (sx / 2) (cos, sin)
    gh += sy * (c * uy - s * ux);      // d corner / d h = (sy / 2) (-sin, cos)
    gc += dx * ux + dy * uy;           // d corner / d cos = (dx, dy)
    gs += dx * uy - dy * ux;           // d corner / d sin = (-dy, dx)
  }
  g[0] = scale * (a[2] * gx);
  g[1] = scale * (a[3] * gy);
  g[2] = scale * (hw * gw);            // d w / d p2 = w
  g[3] = scale * (hh * gh);
  g[4] = scale * (a[5] * gs - a[4] * gc);
  g[5] = scale * (a[4] * gs + a[5] * gc);
  return sum;
}

// workgroup reduction of the two loss sums, one atomic per workgroup and loss (det_loss_kernel's)
__device__ inline void corner_loss_sums(double l_cls, double l_loc, float inv_norm, double* __restrict__ losses) {
  __shared__ double red[2][256];
  red[0][threadIdx.x] = l_cls;
  red[1][threadIdx.x] = l_loc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) {
      red[0][threadIdx.x] += red[0][threadIdx.x + s];
      red[1][threadIdx.x] += red[1][threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    atomic_add_f64(&losses[0], red[0][0] * inv_norm);
    atomic_add_f64(&losses[1], red[1][0] * inv_norm);
  }
}

// Per-anchor form (odd n or unaligned tensors): a lane per anchor.  loc / targets / anchors are read only under mask != 0 --
// positives are well under 1 % of the anchors, so the wave runs corner_one for the few lanes that have one (a lane-level
// branch: the other lanes idle for ~150 instructions in the waves that hold a positive) and the kernel streams cls, labels,
// mask in and dcls, dloc out.  An unmasked dloc row is written as zeros here: no memset in front.
__global__ void __launch_bounds__(256)
det_loss_corner_kernel(const float* __restrict__ cls, const float* __restrict__ labels, const float* __restrict__ loc,
                       const float* __restrict__ targets, const float* __restrict__ mask, const float* __restrict__ anchors,
                       long per_image, long n, float alpha, float gamma, float inv_norm, double* __restrict__ losses,
                       float* __restrict__ dcls, float* __restrict__ dloc) {
  double l_cls = 0.0, l_loc = 0.0;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    float d0, d1;
    focal_one(cls[2 * i], cls[2 * i + 1], labels[2 * i], labels[2 * i + 1], alpha, gamma, inv_norm, d0, d1, l_cls);
    dcls[2 * i] = d0;
    dcls[2 * i + 1] = d1;
    const float mk = mask[i];
    float g[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (mk != 0.f)
      l_loc += (double)(mk * corner_one(anchors + 6 * (i % per_image), loc + 6 * i, targets + 6 * i, mk * inv_norm, g));
#pragma unroll
    for (int k = 0; k < 6; ++k) dloc[6 * i + k] = g[k];
  }
  corner_loss_sums(l_cls, l_loc, inv_norm, losses);
}

// The same on FLAT float4 streams, det_loss_v4_kernel's discipline (n even, 16-byte aligned cls / labels / dcls / dloc).
// Loop A is det_loss_v4_kernel's: two anchors' logits / labels per float4.  Loop B writes dloc four consecutive elements
// per lane: element 4 i is code r = 4 i % 6 in {0, 2, 4} of anchor a0 = 4 i / 6, so the float4 holds codes r .. of a0 and,
// for r = 4 only, codes 0, 1 of a0 + 1.  A lane whose anchors are unmasked stores zeros; one that meets a masked anchor
// runs corner_one for it and keeps its own codes (an anchor's six codes lie in two float4s: two lanes compute it, the one
// that holds code 0 adds the value).
__global__ void __launch_bounds__(256)
det_loss_corner_v4_kernel(const float* __restrict__ cls, const float* __restrict__ labels, const float* __restrict__ loc,
                          const float* __restrict__ targets, const float* __restrict__ mask,
                          const float* __restrict__ anchors, long per_image, long n, float alpha, float gamma, float inv_norm,
                          double* __restrict__ losses, float* __restrict__ dcls, float* __restrict__ dloc) {
  double l_cls = 0.0, l_loc = 0.0;
  const long stride = (long)gridDim.x * blockDim.x, t0 = blockIdx.x * (long)blockDim.x + threadIdx.x;
  for (long i = t0; i < n / 2; i += stride) {
    const f32x4 z = ldv4(cls + 4 * i), lb = ldv4(labels + 4 * i);
    float d0, d1, d2, d3;
    focal_one(z[0], z[1], lb[0], lb[1], alpha, gamma, inv_norm, d0, d1, l_cls);
    focal_one(z[2], z[3], lb[2], lb[3], alpha, gamma, inv_norm, d2, d3, l_cls);
    *reinterpret_cast<f32x4*>(dcls + 4 * i) = f32x4{d0, d1, d2, d3};
  }
  const long m4 = n * 6 / 4;
  for (long i = t0; i < m4; i += stride) {
    const long a0 = (4 * i) / 6;
    const int r = (int)(4 * i - 6 * a0);
    f32x4 out = {0.f, 0.f, 0.f, 0.f};
    const float mk0 = mask[a0];
    if (mk0 != 0.f) {
      float g[6];
      const float v = corner_one(anchors + 6 * (a0 % per_image), loc + 6 * a0, targets + 6 * a0, mk0 * inv_norm, g);
      if (r == 0) {
        out = f32x4{g[0], g[1], g[2], g[3]};
        l_loc += (double)(mk0 * v);
      } else if (r == 2) {
        out = f32x4{g[2], g[3], g[4], g[5]};
      } else {
        out[0] = g[4];
        out[1] = g[5];
      }
    }
    if (r == 4) {      // (4 i + 3 < 6 n: anchor a0 + 1 exists)
      const float mk1 = mask[a0 + 1];
      if (mk1 != 0.f) {
        float g[6];
        const float v = corner_one(anchors + 6 * ((a0 + 1) % per_image), loc + 6 * (a0 + 1), targets + 6 * (a0 + 1),
                                   mk1 * inv_norm, g);
        out[2] = g[0];
        out[3] = g[1];
        l_loc += (double)(mk1 * v);
      }
    }
    *reinterpret_cast<f32x4*>(dloc + 4 * i) = out;
  }
  corner_loss_sums(l_cls, l_loc, inv_norm, losses);
}

// b1 / b2 and their complements c1 = 1 - b1, c2 = 1 - b2 arrive rounded from double each on its own (dn_adam_step): 1.f - b2 of a
// float-rounded 0.999 is off by 1.3e-5 of itself, which reached the update at ~3e-6 of its size.
__global__ void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                            float* __restrict__ v, long n, float step_size, float b1, float c1, float b2, float c2, float eps,
                            float wd, float bc2_sqrt) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    float gi = g[i];
    if (wd != 0.f) gi += wd * p[i];
    const float mi = b1 * m[i] + c1 * gi;
    const float vi = b2 * v[i] + c2 * gi * gi;
    m[i] = mi;
    v[i] = vi;
    // torch: denom = sqrt(v) / sqrt(bias_correction2) + eps; p -= (lr / bias_correction1) * m / denom
    p[i] -= step_size * mi / (sqrtf(vi) / bc2_sqrt + eps);
  }
}

int grid_for(long total, int cap = 4096) {
  const long b = (total + 255) / 256;
  return (int)(b < 1 ? 1 : (b > cap ? cap : b));
}

bool vec4_ok(int c, std::initializer_list<int> lds, std::initializer_list<const void*> ptrs) {
  if (c % 4) return false;
  for (int ld : lds)
    if (ld % 4) return false;
  for (const void* p : ptrs)
    if (p && (reinterpret_cast<uintptr_t>(p) & 15)) return false;
  return true;
}

// DN_BN_LEGACY=1: the general apply kernels and one row per iteration in the reductions (tests: the bitwise A/B; tools)
bool bn_legacy() {
  static const bool legacy = [] { const char* e = getenv("DN_BN_LEGACY"); return e && e[0] == '1'; }();
  return legacy;
}

// the one-group fast kernels (bn_apply_v4_fast_kernel, bn_bwd_apply_v4_fast_kernel): log2(c / 4) where they take the shape,
// else -1.  DN_BN_LEGACY=1 gives their shapes to the general kernels -- not the SP apply's (honour_legacy false): no general twin
int bn_fast_shift(int n_groups, long rows_per_group, int c, bool honour_legacy = true) {
  const int c4n = c >> 2;
  if ((honour_legacy && bn_legacy()) || n_groups != 1 || rows_per_group <= 0 || c % 4 != 0 || c > kMaxC || c4n <= 0 ||
      (c4n & (c4n - 1)) != 0 || rows_per_group * c / 4 >= (1L << 31))
    return -1;
  int sh = 0;
  while ((1 << sh) < c4n) ++sh;
  return sh;
}

// The kernels a BatchNorm pass runs: the general ones (any c, stride, alignment), the float4 ones (c % 4 == 0, 16-byte aligned
// strides and tensors) or, of those, the one-group fast ones (`shift`: bn_fast_shift).  A reduction runs float4 unless general.
enum class BnKernels { general = 0, vec4 = 1, fast = 2 };
struct BnForm { BnKernels k; int shift; };
BnForm bn_form(int n_groups, long rows_per_group, int c, std::initializer_list<int> lds, std::initializer_list<const void*> ptrs) {
  if (!vec4_ok(c, lds, ptrs)) return {BnKernels::general, -1};
  const int sh = bn_fast_shift(n_groups, rows_per_group, c);
  return {sh >= 0 ? BnKernels::fast : BnKernels::vec4, sh};
}

// tools and tests only (dn_bn_train_last_form): the record every BatchNorm entry point writes once nothing can refuse the call
// any more.  Host side; no kernel knows of it.
struct BnLastForm { int cls, u, flags, fold, grid, groups, c, rows; };
BnLastForm g_bn_last[DN_BN_PASSES] = {{-1, 0, 0, 0, 0, 0, 0, 0}, {-1, 0, 0, 0, 0, 0, 0, 0}, {-1, 0, 0, 0, 0, 0, 0, 0}, {-1, 0, 0, 0, 0, 0, 0, 0},
                                      {-1, 0, 0, 0, 0, 0, 0, 0}, {-1, 0, 0, 0, 0, 0, 0, 0}, {-1, 0, 0, 0, 0, 0, 0, 0}, {-1, 0, 0, 0, 0, 0, 0, 0}};
void bn_note(int pass, BnKernels k, int u, int flags, int fold, int grid, int groups, int c, long rows) {
  g_bn_last[pass] = BnLastForm{(int)k, u, flags, fold, grid, groups, c, (int)(rows > 0x7fffffffL ? 0x7fffffffL : rows)};
}

// Workgroups of a per-channel reduction over all groups.  1024 since round 5 (2048 before): measured in one lease
// (profiles/r05_reduce_blocks.txt) the folds of a training step cost 0.69 / 0.48 / 0.36 ms at 2048 / 1024 / 512 and the
// reductions themselves 2.13 / 2.02 / 2.64 ms -- four workgroups per CU still saturate the HBM, two do not.
constexpr int kReduceBlocks = 1024;
int blocks_per_group(long rows_per_group, int n_groups) {
  // ~1024 workgroups over all groups, at least 64 rows each
  long b = kReduceBlocks / n_groups;
  if (b > rows_per_group / 64) b = rows_per_group / 64;
  return (int)(b < 1 ? 1 : b);
}

// phase 1 of the statistics: every workgroup's partial sums, [n_groups][*nblk][2 c] doubles behind the [n_groups][2 c] folded
// sums at the start of `sums`
int bn_stats_reduce(const float* z, int n_groups, long rows_per_group, int c, int ldz, double* sums, size_t sums_bytes,
                    int* nblk, hipStream_t s) {
  DN_REQUIRE(z && sums, "bn stats: null pointer");
  DN_REQUIRE(n_groups > 0 && rows_per_group > 0 && c > 0 && c <= kMaxC && ldz >= c,
             "bn stats: bad shape (groups %d rows %ld c %d ld %d)", n_groups, rows_per_group, c, ldz);
  DN_REQUIRE(sums_bytes >= dn_reduce_workspace_bytes(n_groups, rows_per_group, c),
             "bn stats: workspace of %zu bytes, dn_reduce_workspace_bytes() asks for %zu", sums_bytes,
             dn_reduce_workspace_bytes(n_groups, rows_per_group, c));
  *nblk = blocks_per_group(rows_per_group, n_groups);
  double* part = sums + (size_t)2 * c * n_groups;
  const BnKernels k = bn_form(n_groups, rows_per_group, c, {ldz}, {z}).k;
  bn_note(DN_BN_PASS_STATS_REDUCE, k, k == BnKernels::general || bn_legacy() ? 1 : 4, 0, DN_BN_FOLD_NONE, *nblk, n_groups, c, rows_per_group);
  if (k != BnKernels::general)
    hipLaunchKernelGGL(bn_legacy() ? bn_stats_v4_kernel<1> : bn_stats_v4_kernel<4>, dim3(*nblk, n_groups), dim3(256), 0, s, z, rows_per_group, c, ldz, part);
  else
    hipLaunchKernelGGL(bn_stats_kernel, dim3(*nblk, n_groups), dim3(256), 0, s, z, rows_per_group, c, ldz, part);
  return 0;
}

// the description both phases of the backward take
int bn_backward_args(const dn_bn_bwd_desc* d) {
  DN_REQUIRE(d && d->dy_a && d->z && d->mean && d->var, "bn backward: null pointer");
  const int ld_a = d->ld_a, up_a = d->up_a, ld_b = d->ld_b, relu = d->relu, n_groups = d->n_groups, h = d->h, w = d->w,
            images_per_group = d->images_per_group, c = d->c;
  const float* dy_b = d->dy_b;
  DN_REQUIRE(!relu || d->y, "bn backward: relu needs y");
  DN_REQUIRE(relu >= 0 && relu <= 2 && (relu != 2 || c % 4 == 0), "bn backward: relu = 2 (y is the byte mask) needs c %% 4 == 0");
  DN_REQUIRE(up_a >= 0 && up_a <= 2 && (up_a != 2 || (h % 2 == 0 && w % 2 == 0 && ld_a >= 4 * c)),
             "bn backward: up_a = 2 (dy_a is the space-to-depth image [h / 2][w / 2][4 c]) needs even h, w and ld_a >= 4 c");
  DN_REQUIRE(n_groups > 0 && h > 0 && w > 0 && images_per_group > 0 && c > 0 && c <= kMaxC && ld_a >= c && (!dy_b || ld_b >= c),
             "bn backward: bad shape");
  return 0;
}

GradSrc bn_grad_src(const dn_bn_bwd_desc* d) {
  return GradSrc{d->dy_a, d->dy_b, (const float*)d->y, d->ld_a, d->up_a, d->ld_b, d->relu, d->h, d->w, d->c};
}

}  // namespace

// doubles of workspace a per-channel reduction needs: the folded sums + every workgroup's partial
extern "C" size_t dn_reduce_workspace_bytes(int n_groups, long rows_per_group, int c) {
  if (n_groups <= 0 || rows_per_group <= 0 || c <= 0) return 0;
  return sizeof(double) * 2 * c * n_groups * (size_t)(1 + blocks_per_group(rows_per_group, n_groups));
}

// workspace of the fused bias gradient (dn_bn_bwd_out.dbias): [c] folded sums + one double per (workgroup of
// the apply launch, channel)
// workgroups of the apply launch when it also leaves the bias partials: every workgroup is one row of partials for the fold
// (one wavefront per channel walks them), so fewer than the plain launch's 8192
constexpr int kBiasBlocks = 1024;
extern "C" size_t dn_bn_bias_workspace_bytes(long rows, int c) {
  if (rows <= 0 || c <= 0) return 0;
  return sizeof(double) * (size_t)c * (size_t)(1 + grid_for(rows * (long)c / 4, kBiasBlocks));
}

// The one rule of the fused forms: each entry point's DN_REQUIRE asks this, Python asks it through the C ABI.
extern "C" int dn_bn_train_form_supported(int form, int n_groups, long rows_per_group, int c) {
  switch (form) {
    case DN_BN_FORM_SP_APPLY: return c % 16 == 0 && bn_fast_shift(n_groups, rows_per_group, c, false) >= 0;
    case DN_BN_FORM_BIAS: return bn_fast_shift(n_groups, rows_per_group, c) >= 0;
    case DN_BN_FORM_DZ_NULL: return c % 16 == 0 && bn_fast_shift(n_groups, rows_per_group, c) >= 0;
  }
  return 0;
}

// Two-phase forms (round 5: agent-parallel training, sharded.py).  A rank that holds only SOME images of a BatchNorm batch
// reduces its own rows (`_partial`: the folded sums [n_groups][2 c] doubles land at the start of `sums`), the caller
// all-reduces those doubles over the ranks, and `_finish` normalises by the GLOBAL row count.  The one-call forms below are
// the two phases back to back with norm_rows = rows_per_group.
extern "C" int dn_bn_train_stats_partial(const float* z, int n_groups, long rows_per_group, int c, int ldz,
                                         double* sums, size_t sums_bytes, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  int nblk;
  if (int rc = bn_stats_reduce(z, n_groups, rows_per_group, c, ldz, sums, sums_bytes, &nblk, s)) return rc;
  bn_note(DN_BN_PASS_STATS_FINISH, BnKernels::general, 1, 0, DN_BN_FOLD_PARTIALS_FINALIZE, (n_groups * 2 * c + 3) / 4, n_groups, c, rows_per_group);
  hipLaunchKernelGGL(fold_partials_kernel, dim3((n_groups * 2 * c + 3) / 4), dim3(256), 0, s, sums + (size_t)2 * c * n_groups,
                     nblk, 2 * c, n_groups, sums);
  return dn::check_launch("bn_stats_kernel");
}

extern "C" int dn_bn_train_stats_finish(const double* sums, int n_groups, long norm_rows, int c, float* mean, float* var,
                                        void* stream) {
  DN_REQUIRE(sums && mean && var, "bn stats finish: null pointer");
  DN_REQUIRE(n_groups > 0 && norm_rows > 0 && c > 0 && c <= kMaxC, "bn stats finish: bad shape");
  const int n = n_groups * c;
  bn_note(DN_BN_PASS_STATS_FINISH, BnKernels::general, 1, 0, DN_BN_FOLD_PARTIALS_FINALIZE, (n + 255) / 256, n_groups, c, norm_rows);
  hipLaunchKernelGGL(bn_stats_finalize_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, sums, n, c,
                     norm_rows, mean, var);
  return dn::check_launch("bn_stats_finalize_kernel");
}

extern "C" int dn_bn_train_stats(const float* z, int n_groups, long rows_per_group, int c, int ldz, double* sums, size_t sums_bytes,
                                 float* mean, float* var, float* running_mean, float* running_var, float momentum, void* stream) {
  DN_REQUIRE(mean && var, "bn stats: null pointer");
  DN_REQUIRE(!running_mean == !running_var, "bn stats (+ running): running_mean and running_var go together: null pointer");
  DN_REQUIRE(!running_mean || n_groups == 1, "bn stats: the fused running-statistics update takes one group");
  hipStream_t s = (hipStream_t)stream;
  int nblk;
  if (int rc = bn_stats_reduce(z, n_groups, rows_per_group, c, ldz, sums, sums_bytes, &nblk, s)) return rc;
  // fold + finish (+ the running statistics) in one launch: the sums and statistics of the two-launch path, bit for bit
  bn_note(DN_BN_PASS_STATS_FINISH, BnKernels::general, 1, running_mean ? DN_BN_REC_RUNNING : 0, DN_BN_FOLD_STATS_FINISH, (n_groups * c + 3) / 4,
          n_groups, c, rows_per_group);
  hipLaunchKernelGGL(fold_stats_finish_kernel, dim3((n_groups * c + 3) / 4), dim3(256), 0, s, sums + (size_t)2 * c * n_groups, nblk, c,
                     n_groups, rows_per_group, sums, mean, var, running_mean, running_var, running_mean ? momentum : 0.f,
                     running_mean ? rows_per_group : 0L);
  return dn::check_launch("bn_stats_kernel");
}

extern "C" int dn_bn_train_apply(const float* z, const float* mean, const float* var, const float* gamma, const float* beta,
                                 float eps, int relu, int n_groups, long rows_per_group, int c, int ldz, float* y,
                                 unsigned char* relu_mask, void* y_sp, int hw, void* stream) {
  DN_REQUIRE(z && mean && var && gamma && beta && y, "bn apply: null pointer");
  DN_REQUIRE(n_groups > 0 && rows_per_group > 0 && c > 0 && ldz >= c, "bn apply: bad shape");
  DN_REQUIRE(!relu_mask || relu == 1, "bn apply (mask): the relu mask is written with relu = 1 only");
  const long total = (long)n_groups * rows_per_group * c;
  hipStream_t s = (hipStream_t)stream;
  if (!y_sp) {
    const BnForm f = bn_form(n_groups, rows_per_group, c, {ldz}, {z, y, mean, var, gamma, beta});
    DN_REQUIRE(!relu_mask || f.k != BnKernels::general, "bn apply (mask): needs c %% 4 == 0 and 16-byte aligned tensors");
    bn_note(DN_BN_PASS_APPLY, f.k, 1, relu_mask ? DN_BN_REC_MASK : 0, DN_BN_FOLD_NONE,
            grid_for(f.k == BnKernels::general ? total : total / 4, 8192), n_groups, c, rows_per_group);
    if (f.k == BnKernels::fast)
      hipLaunchKernelGGL(bn_apply_v4_fast_kernel<false>, dim3(grid_for(total / 4, 8192)), dim3(256), 0, s, z, mean, var,
                         gamma, beta, eps, relu, c, f.shift, ldz, (unsigned)(total / 4), y, relu_mask, (unsigned char*)nullptr, 1u,
                         (unsigned*)nullptr);
    else if (f.k == BnKernels::vec4)
      hipLaunchKernelGGL(bn_apply_v4_kernel, dim3(grid_for(total / 4, 8192)), dim3(256), 0, s, z, mean, var,
                         gamma, beta, eps, relu, rows_per_group, c, ldz, total / 4, y, relu_mask);
    else
      hipLaunchKernelGGL(bn_apply_kernel, dim3(grid_for(total, 8192)), dim3(256), 0, s, z,
                         mean, var, gamma, beta, eps, relu, rows_per_group, c, ldz, total, y);
    return dn::check_launch("bn_apply_kernel");
  }
  // y_sp: the one-group fast kernel that also writes the SP copy
  DN_REQUIRE(relu_mask, "bn apply (mask + SP): y_sp needs relu_mask: null pointer");
  DN_REQUIRE(hw > 0 && rows_per_group % hw == 0, "bn apply (mask + SP): bad shape");
  DN_REQUIRE(dn_bn_train_form_supported(DN_BN_FORM_SP_APPLY, n_groups, rows_per_group, c),
             "bn apply (mask + SP): needs one group, c %% 16 == 0, c / 4 a power of two, c <= %d and the map below 2^31 float4s (c = %d, groups = %d)",
             kMaxC, c, n_groups);
  DN_REQUIRE(vec4_ok(c, {ldz}, {z, y, mean, var, gamma, beta}) && (reinterpret_cast<uintptr_t>(y_sp) & 15) == 0,
             "bn apply (mask + SP): needs 16-byte aligned tensors");
  unsigned* flags = dn::sp_range_word();
  DN_REQUIRE(flags, "bn apply (mask + SP): the range word of the split-f16 engine is not addressable");
  const int fsh = bn_fast_shift(1, rows_per_group, c, false);      // (the SP form has no general-kernel twin for DN_BN_LEGACY to select)
  bn_note(DN_BN_PASS_APPLY, BnKernels::fast, 1, DN_BN_REC_MASK | DN_BN_REC_SP, DN_BN_FOLD_NONE, grid_for(total / 4, 8192), n_groups, c, rows_per_group);
  hipLaunchKernelGGL(bn_apply_v4_fast_kernel<true>, dim3(grid_for(total / 4, 8192)), dim3(256), 0, s, z, mean, var,
                     gamma, beta, eps, 1, c, fsh, ldz, (unsigned)(total / 4), y, relu_mask, (unsigned char*)y_sp, (unsigned)hw, flags);
  return dn::check_launch("bn_apply_kernel (mask + SP)");
}

extern "C" int dn_bn_update_running(const float* mean, const float* var, int n_groups,
                                    long rows_per_group, int c, const int* order, float momentum,
                                    float* running_mean, float* running_var, void* stream) {
  DN_REQUIRE(mean && var && running_mean && running_var, "bn running: null pointer");
  DN_REQUIRE(n_groups > 0 && rows_per_group > 0 && c > 0, "bn running: bad shape");
  bn_note(DN_BN_PASS_RUNNING, BnKernels::general, 8, order ? DN_BN_REC_ORDER : 0, DN_BN_FOLD_NONE, (c + 63) / 64, n_groups, c, rows_per_group);
  hipLaunchKernelGGL(bn_update_running_kernel, dim3((c + 63) / 64), dim3(64), 0, (hipStream_t)stream,
                     mean, var, n_groups, rows_per_group, c, order, momentum, running_mean, running_var);
  return dn::check_launch("bn_update_running_kernel");
}

static_assert(sizeof(dn_bn_bwd_desc) == 7 * sizeof(void*) + 10 * 4 && sizeof(dn_bn_bwd_out) == 5 * sizeof(void*) + 16,
              "dn_bn_bwd_desc / dn_bn_bwd_out: the layout include/disconet_train.h documents (and _lib.py restates)");

// phase 1 of the backward: this rank's sums of g and g * zhat (folded, at the start of `sums`) and the parameter gradients
// out of THESE rows (dgamma / dbeta are sums over rows: ranks add theirs with the gradient all-reduce)
extern "C" int dn_bn_train_backward_partial(const dn_bn_bwd_desc* d, double* sums, size_t sums_bytes, float* dgamma, float* dbeta,
                                            int accumulate, void* stream) {
  if (int rc = bn_backward_args(d)) return rc;
  DN_REQUIRE(sums && dgamma && dbeta, "bn backward: null pointer");
  hipStream_t s = (hipStream_t)stream;
  const int n_groups = d->n_groups, c = d->c;
  const long rows_per_group = (long)d->images_per_group * d->h * d->w;
  DN_REQUIRE(sums_bytes >= dn_reduce_workspace_bytes(n_groups, rows_per_group, c),
             "bn backward: workspace of %zu bytes, dn_reduce_workspace_bytes() asks for %zu", sums_bytes,
             dn_reduce_workspace_bytes(n_groups, rows_per_group, c));
  const GradSrc src = bn_grad_src(d);
  const int nblk = blocks_per_group(rows_per_group, n_groups);
  double* part = sums + (size_t)2 * c * n_groups;      // workspace layout: see dn_bn_train_stats_partial
  const BnKernels rk = bn_form(n_groups, rows_per_group, c, {d->ld_a, d->dy_b ? d->ld_b : 0}, {d->dy_a, d->dy_b, d->y, d->z, d->mean, d->var}).k;
  bn_note(DN_BN_PASS_BWD_REDUCE, rk, rk == BnKernels::general || bn_legacy() ? 1 : 2, d->relu == 2 ? DN_BN_REC_MASK : 0,
          n_groups == 1 && !bn_legacy() ? DN_BN_FOLD_PARAM_GRAD : DN_BN_FOLD_PARTIALS_PARAM_GRAD, nblk, n_groups, c, rows_per_group);
  if (rk != BnKernels::general)
    hipLaunchKernelGGL(bn_legacy() ? bn_bwd_reduce_v4_kernel<1> : bn_bwd_reduce_v4_kernel<2>, dim3(nblk, n_groups), dim3(256), 0, s, src, d->z, d->mean, d->var, d->eps,
                       rows_per_group, part);
  else
    hipLaunchKernelGGL(bn_bwd_reduce_kernel, dim3(nblk, n_groups), dim3(256), 0, s, src, d->z, d->mean, d->var, d->eps,
                       rows_per_group, part);
  if (n_groups == 1 && !bn_legacy()) {      // fold + parameter gradients in one launch (same sums, same bits)
    hipLaunchKernelGGL(fold_param_grad_kernel, dim3((c + 3) / 4), dim3(256), 0, s, part, nblk, c, sums, dgamma, dbeta, accumulate);
    return dn::check_launch("bn_backward reduce kernels");
  }
  hipLaunchKernelGGL(fold_partials_kernel, dim3((n_groups * 2 * c + 3) / 4), dim3(256), 0, s, part, nblk, 2 * c,
                     n_groups, sums);
  hipLaunchKernelGGL(bn_param_grad_kernel, dim3((c + 63) / 64), dim3(64), 0, s, sums, n_groups, c,
                     dgamma, dbeta, accumulate);
  return dn::check_launch("bn_backward reduce kernels");
}

// phase 2: what `out` asks for of this rank's rows from the (all-reduced) sums, means taken over norm_rows rows per group
extern "C" int dn_bn_train_backward_finish(const dn_bn_bwd_desc* d, const double* sums, long norm_rows, const dn_bn_bwd_out* out,
                                           void* stream) {
  if (int rc = bn_backward_args(d)) return rc;
  DN_REQUIRE(d->gamma && sums && out && (out->dz || out->dz_sp), "bn backward finish: null pointer");
  DN_REQUIRE(norm_rows > 0, "bn backward finish: bad shape");
  hipStream_t s = (hipStream_t)stream;
  const int n_groups = d->n_groups, c = d->c, h = d->h, w = d->w;
  const long rows_per_group = (long)d->images_per_group * h * w;
  float* dz = out->dz;
  // dz NULL (round 6): only the SP copy is written; the one-group fast kernels only
  DN_REQUIRE(dz || dn_bn_train_form_supported(DN_BN_FORM_DZ_NULL, n_groups, rows_per_group, c),
             "bn backward: dz may be NULL only where the one-group fast form runs (one group, c %% 16 == 0, c / 4 a power of two; DN_BN_LEGACY unset)");
  const BnForm f = bn_form(n_groups, rows_per_group, c, {d->ld_a, d->dy_b ? d->ld_b : 0},
                           {d->dy_a, d->dy_b, d->y, d->z, d->mean, d->var, d->gamma, dz});
  const bool bias = out->dbias || out->n_blocks;
  DN_REQUIRE(!(out->dbias && out->n_blocks), "bn backward: dbias is either folded here (dbias) or deferred (n_blocks), not both");
  DN_REQUIRE(!bias || (dn_bn_train_form_supported(DN_BN_FORM_BIAS, n_groups, rows_per_group, c) && f.k != BnKernels::general),
             "bn backward: the fused bias gradient needs the one-group fast form (one group, c / 4 a power of two, aligned tensors; DN_BN_LEGACY unset)");
  unsigned* flags = nullptr;
  if (out->dz_sp) {
    DN_REQUIRE(n_groups == 1 && c % 16 == 0 && f.k != BnKernels::general && (reinterpret_cast<uintptr_t>(out->dz_sp) & 15) == 0 &&
                   rows_per_group < (1L << 31),
               "bn backward: the SP copy of dz needs one group, c %% 16 == 0, 16-byte aligned tensors (c = %d, groups = %d)", c, n_groups);
    DN_REQUIRE(out->sp_lift > 0.f && std::isfinite(out->sp_lift), "bn backward: sp_lift must be a positive finite power of two");
    flags = dn::sp_range_word();
    DN_REQUIRE(flags, "bn backward: the range word of the split-f16 engine is not addressable");
  }
  const GradSrc src = bn_grad_src(d);
  const long total = (long)n_groups * rows_per_group * c;
  unsigned char* sp = (unsigned char*)out->dz_sp;
  const float lift = sp ? out->sp_lift : 1.f;
  const int rec = (sp ? DN_BN_REC_SP : 0) | (bias ? DN_BN_REC_BIAS : 0) | (d->relu == 2 ? DN_BN_REC_MASK : 0) | (dz ? 0 : DN_BN_REC_DZ_NULL);
  if (bias) {
    // the fused bias gradient (round 6): the apply launch leaves one double per (workgroup, channel), folded in a fixed order
    const int blocks = grid_for(total / 4, kBiasBlocks);
    DN_REQUIRE(out->bias_ws && out->bias_ws_bytes >= dn_bn_bias_workspace_bytes(rows_per_group, c),
               "bn backward: bias workspace of %zu bytes, dn_bn_bias_workspace_bytes() asks for %zu", (size_t)out->bias_ws_bytes,
               dn_bn_bias_workspace_bytes(rows_per_group, c));
    double* part = out->bias_ws + c;      // [c] folded sums, then [blocks][c] partials
    bn_note(DN_BN_PASS_BWD_APPLY, f.k, 1, rec, out->n_blocks ? DN_BN_FOLD_DEFERRED : DN_BN_FOLD_CHANNEL_SUM, blocks, n_groups, c, norm_rows);
    hipLaunchKernelGGL((sp ? bn_bwd_apply_v4_fast_kernel<true, true> : bn_bwd_apply_v4_fast_kernel<false, true>), dim3(blocks), dim3(256), 0,
                       s, src, d->z, d->mean, d->var, d->gamma, d->eps, norm_rows, sums, f.shift, (unsigned)(total / 4), dz, sp, lift, (unsigned)(h * w), flags, part);
    if (out->n_blocks)      // the fold is the caller's (dn_channel_sum_fold_multi): the partials stay in bias_ws
      *out->n_blocks = blocks;
    else
      hipLaunchKernelGGL(fold_channel_sum_kernel, dim3((c + 3) / 4), dim3(256), 0, s, part, blocks, c, out->bias_ws, out->dbias, 0);
    return dn::check_launch("bn backward apply kernel (+ bias gradient)");
  }
  const unsigned hw = sp ? (unsigned)(h * w) : 1u;
  bn_note(DN_BN_PASS_BWD_APPLY, f.k, 1, rec, DN_BN_FOLD_NONE, grid_for(f.k == BnKernels::general ? total : total / 4, 8192), n_groups, c, norm_rows);
  if (f.k == BnKernels::fast)
    hipLaunchKernelGGL(sp ? bn_bwd_apply_v4_fast_kernel<true> : bn_bwd_apply_v4_fast_kernel<false>, dim3(grid_for(total / 4, 8192)), dim3(256),
                       0, s, src, d->z, d->mean, d->var, d->gamma, d->eps, norm_rows, sums, f.shift, (unsigned)(total / 4), dz, sp, lift, hw, flags, (double*)nullptr);
  else if (f.k == BnKernels::vec4)
    hipLaunchKernelGGL(sp ? bn_bwd_apply_v4_kernel<true> : bn_bwd_apply_v4_kernel<false>, dim3(grid_for(total / 4, 8192)), dim3(256), 0, s,
                       src, d->z, d->mean, d->var, d->gamma, d->eps, rows_per_group, norm_rows, sums, total / 4, dz, sp, lift, hw, flags);
  else
    hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3(grid_for(total, 8192)), dim3(256), 0, s, src, d->z, d->mean,
                       d->var, d->gamma, d->eps, rows_per_group, norm_rows, sums, total, dz);
  return dn::check_launch("bn_backward apply kernels");
}

extern "C" int dn_bn_train_backward(const dn_bn_bwd_desc* d, double* sums, size_t sums_bytes, const dn_bn_bwd_out* out,
                                    float* dgamma, float* dbeta, int accumulate, void* stream) {
  DN_REQUIRE(d && d->gamma && out && (out->dz || out->dz_sp), "bn backward: null pointer");
  if (int rc = dn_bn_train_backward_partial(d, sums, sums_bytes, dgamma, dbeta, accumulate, stream)) return rc;
  return dn_bn_train_backward_finish(d, sums, (long)d->images_per_group * d->h * d->w, out, stream);
}

extern "C" int dn_channel_sum_fold_multi(const dn_fold_job* jobs, int n_jobs, void* stream) {
  DN_REQUIRE(jobs && n_jobs > 0, "channel sum fold multi: no jobs");
  for (int j = 0; j < n_jobs; ++j)      // every job is looked at before the first launch: a refused call has folded nothing
    DN_REQUIRE(jobs[j].partials && jobs[j].sums && jobs[j].out && jobs[j].n_blocks > 0 && jobs[j].c > 0 && jobs[j].c <= kMaxC,
               "channel sum fold multi: job %d", j);
  for (int j0 = 0; j0 < n_jobs; j0 += kFoldJobs) {
    const int n = n_jobs - j0 < kFoldJobs ? n_jobs - j0 : kFoldJobs;
    FoldJobs J;
    int waves = 0;
    for (int j = 0; j < n; ++j) {
      const dn_fold_job& q = jobs[j0 + j];
      J.part[j] = q.partials; J.sums[j] = q.sums; J.out[j] = q.out;
      J.n_blocks[j] = q.n_blocks; J.c[j] = q.c; J.accumulate[j] = q.accumulate;
      J.first[j] = waves;
      waves += q.c;
    }
    for (int j = n; j <= kFoldJobs; ++j) J.first[j] = waves;
    for (int j = n; j < kFoldJobs; ++j) { J.part[j] = nullptr; J.sums[j] = nullptr; J.out[j] = nullptr; J.n_blocks[j] = J.c[j] = J.accumulate[j] = 0; }
    bn_note(DN_BN_PASS_FOLD_MULTI, BnKernels::general, FOLD_BATCH, 0, DN_BN_FOLD_MULTI, n, j0 / kFoldJobs + 1, waves, 0);
    hipLaunchKernelGGL(fold_channel_sum_multi_kernel, dim3((waves + 3) / 4), dim3(256), 0, (hipStream_t)stream, J, n);
  }
  return dn::check_launch("fold_channel_sum_multi_kernel");
}

extern "C" int dn_channel_sum_partial(const float* x, long rows, int c, int ld, double* sums, size_t sums_bytes, int* n_blocks,
                                      void* stream) {
  DN_REQUIRE(x && sums && n_blocks, "channel sum: null pointer");
  DN_REQUIRE(rows > 0 && c > 0 && c <= kMaxC && ld >= c, "channel sum: bad shape");
  DN_REQUIRE(sums_bytes >= dn_reduce_workspace_bytes(1, rows, c),
             "channel sum: workspace of %zu bytes, dn_reduce_workspace_bytes() asks for %zu", sums_bytes,
             dn_reduce_workspace_bytes(1, rows, c));
  hipStream_t s = (hipStream_t)stream;
  const int nblk = blocks_per_group(rows, 1);
  double* part = sums + c;                              // [c] folded sums (the fold's), then the workgroups' partials [blocks][c]
  bn_note(DN_BN_PASS_CHANNEL_SUM, vec4_ok(c, {ld}, {x}) ? BnKernels::vec4 : BnKernels::general, vec4_ok(c, {ld}, {x}) && !bn_legacy() ? 4 : 1, 0,
          DN_BN_FOLD_DEFERRED, nblk, 1, c, rows);
  if (vec4_ok(c, {ld}, {x}))
    hipLaunchKernelGGL(bn_legacy() ? channel_sum_v4_kernel<1> : channel_sum_v4_kernel<4>, dim3(nblk), dim3(256), 0, s, x, rows, c, ld, part);
  else
    hipLaunchKernelGGL(channel_sum_kernel, dim3(nblk), dim3(256), 0, s, x, rows, c, ld, part);
  *n_blocks = nblk;
  return dn::check_launch("channel_sum_kernel");
}

extern "C" int dn_channel_sum(const float* x, long rows, int c, int ld, double* sums, size_t sums_bytes, float* out,
                              int accumulate, void* stream) {
  DN_REQUIRE(out, "channel sum: null pointer");
  int nblk;
  if (int rc = dn_channel_sum_partial(x, rows, c, ld, sums, sums_bytes, &nblk, stream)) return rc;
  g_bn_last[DN_BN_PASS_CHANNEL_SUM].fold = DN_BN_FOLD_CHANNEL_SUM;
  hipLaunchKernelGGL(fold_channel_sum_kernel, dim3((c + 3) / 4), dim3(256), 0, (hipStream_t)stream, sums + c, nblk, c, sums, out,
                     accumulate);
  return dn::check_launch("fold_channel_sum_kernel");
}

extern "C" int dn_bn_train_last_form(int pass, int* out, int n) {
  constexpr int kInts = (int)(sizeof(BnLastForm) / sizeof(int));
  static_assert(sizeof(BnLastForm) == 8 * sizeof(int), "dn_bn_train_last_form: the record is 8 ints");
  DN_REQUIRE(out && n > 0 && pass >= 0 && pass < DN_BN_PASSES, "bn last form: null pointer / no room / unknown pass %d", pass);
  const int* f = reinterpret_cast<const int*>(&g_bn_last[pass]);
  for (int i = 0; i < n && i < kInts; ++i) out[i] = f[i];
  return kInts;
}

extern "C" int dn_add_rows(float* a, int ld_a, const float* b, int ld_b, long rows, int c,
                           void* stream) {
  DN_REQUIRE(a && b && rows > 0 && c > 0 && ld_a >= c && ld_b >= c, "add rows: bad arguments");
  const long total = rows * c;
  hipLaunchKernelGGL(add_rows_kernel, dim3(grid_for(total, 8192)), dim3(256), 0, (hipStream_t)stream, a,
                     ld_a, b, ld_b, c, total);
  return dn::check_launch("add_rows_kernel");
}

extern "C" int dn_upsample2_sum(const float* g, int ld, int n_images, int h, int w, int c, float* out,
                                void* stream) {
  DN_REQUIRE(g && out && n_images > 0 && h > 0 && w > 0 && c > 0 && ld >= c, "upsample sum: bad arguments");
  const long total = (long)n_images * h * w * c;
  hipLaunchKernelGGL(upsample2_sum_kernel, dim3(grid_for(total, 8192)), dim3(256), 0, (hipStream_t)stream,
                     g, ld, h, w, c, total, out);
  return dn::check_launch("upsample2_sum_kernel");
}

extern "C" int dn_pair_add_ego(float* z1, const float* e, const int* ego_image, int n_pairs,
                               int rows_per_image, int c, void* stream) {
  DN_REQUIRE(z1 && e && ego_image && n_pairs > 0 && rows_per_image > 0 && c > 0,
             "pair add: bad arguments");
  const long per_image = (long)rows_per_image * c, total = per_image * n_pairs;
  hipLaunchKernelGGL(pair_add_ego_kernel, dim3(grid_for(total, 8192)), dim3(256), 0,
                     (hipStream_t)stream, z1, e, ego_image, per_image, total);
  return dn::check_launch("pair_add_ego_kernel");
}

extern "C" int dn_pair_sum_ego(const float* dz1, const int* first, const int* pairs, int n_images,
                               int rows_per_image, int c, float* de, void* stream) {
  DN_REQUIRE(dz1 && first && pairs && de && n_images > 0 && rows_per_image > 0 && c > 0,
             "pair sum: bad arguments");
  const long per_image = (long)rows_per_image * c, total = per_image * n_images;
  hipLaunchKernelGGL(pair_sum_ego_kernel, dim3(grid_for(total, 8192)), dim3(256), 0,
                     (hipStream_t)stream, dz1, first, pairs, per_image, total, de);
  return dn::check_launch("pair_sum_ego_kernel");
}

extern "C" int dn_fuse_combine(const float* z4, const float* maps, const int* first,
                               const int* pair_index, const int* map_image, const int* ego_out,
                               int n_egos, int hw, int c, float* weights, float* fused, void* stream) {
  DN_REQUIRE(z4 && maps && first && pair_index && map_image && ego_out && weights && fused,
             "fuse combine: null pointer");
  DN_REQUIRE(n_egos > 0 && hw > 0 && c > 0 && c % 4 == 0, "fuse combine: bad shape");
  const long items = (long)n_egos * hw;
  hipLaunchKernelGGL(fuse_combine_kernel, dim3((unsigned)((items + 3) / 4)), dim3(256), 0,
                     (hipStream_t)stream, z4, maps, first, pair_index, map_image, ego_out, n_egos, hw, c,
                     weights, fused);
  return dn::check_launch("fuse_combine_kernel");
}

extern "C" int dn_fuse_combine_backward(const float* dfused, int ld_df, const float* z4,
                                        const float* weights, const float* maps, const int* first,
                                        const int* pair_index, const int* map_image,
                                        const int* ego_out, int n_egos, int hw, int c, float* dmaps,
                                        float* dz4, void* stream) {
  DN_REQUIRE(dfused && z4 && weights && maps && first && pair_index && map_image && ego_out && dmaps &&
                 dz4,
             "fuse combine backward: null pointer");
  DN_REQUIRE(n_egos > 0 && hw > 0 && c > 0 && c % 4 == 0 && ld_df >= c && ld_df % 4 == 0,
             "fuse combine backward: bad shape");
  const long items = (long)n_egos * hw;
  hipLaunchKernelGGL(fuse_combine_bwd_kernel, dim3((unsigned)((items + 3) / 4)), dim3(256), 0,
                     (hipStream_t)stream, dfused, ld_df, z4, weights, maps, first, pair_index, map_image,
                     ego_out, n_egos, hw, c, dmaps, dz4);
  return dn::check_launch("fuse_combine_bwd_kernel");
}

extern "C" int dn_agent_combine_lists(const float* z4, const float* w5, const float* b5, const float* maps,
                                      const int32_t* first, const int32_t* pair_index, const int32_t* map_image,
                                      const int32_t* ego_out, int n_egos, int hw, int c, float* weights, float* fused,
                                      void* stream) {
  DN_REQUIRE(z4 && w5 && b5 && maps && first && pair_index && map_image && ego_out && weights && fused,
             "agent combine lists: null pointer");
  DN_REQUIRE(n_egos > 0 && n_egos <= 65535 && hw > 0 && c > 0 && c % 4 == 0, "agent combine lists: bad shape");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(agent_list_weights_kernel, dim3(n_egos), dim3(256), 0, s, z4, w5, b5, first, pair_index, hw, weights);
  const long quads = (long)hw * (c >> 2);
  hipLaunchKernelGGL(agent_combine_lists_kernel, dim3(grid_for(quads), n_egos), dim3(256), 0, s, maps, weights, first,
                     map_image, ego_out, quads, fused);
  return dn::check_launch("agent_combine_lists_kernel");
}

extern "C" int dn_agent_combine_lists_backward(const float* dfused, int ld, const float* weights, const int32_t* first,
                                               const int32_t* map_image, const int32_t* ego_out, int n_egos, int hw, int c,
                                               float* dmaps, void* stream) {
  DN_REQUIRE(dfused && weights && first && map_image && ego_out && dmaps, "agent combine lists backward: null pointer");
  DN_REQUIRE(n_egos > 0 && n_egos <= 65535 && hw > 0 && c > 0 && c % 4 == 0, "agent combine lists backward: bad shape");
  DN_REQUIRE(ld >= c && ld % 4 == 0 && ((size_t)dfused & 15) == 0,
             "agent combine lists backward: dfused rows must be 16-byte aligned (ld = %d, c = %d)", ld, c);
  hipLaunchKernelGGL(agent_combine_lists_bwd_kernel, dim3(grid_for((long)hw * (c >> 2)), n_egos), dim3(256), 0,
                     (hipStream_t)stream, dfused, ld, weights, first, map_image, ego_out, hw, c >> 2, dmaps);
  return dn::check_launch("agent_combine_lists_bwd_kernel");
}

extern "C" int dn_det_loss(const float* cls, const float* labels, const float* loc,
                           const float* targets, const float* mask, long n, int code, float alpha,
                           float gamma, float sigma, float norm, double* losses, float* dcls,
                           float* dloc, void* stream) {
  DN_REQUIRE(cls && labels && loc && targets && mask && losses && dcls && dloc, "det loss: null pointer");
  DN_REQUIRE(n > 0 && code > 0 && norm > 0.f && sigma > 0.f, "det loss: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  if (dn::zero_fill(losses, 2 * sizeof(double), s) != hipSuccess)
    return dn::fail(DN_ERR_LAUNCH, "det loss: memset failed");
  auto al16 = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; };
  if (n % 2 == 0 && (n * code) % 4 == 0 && al16(cls) && al16(labels) && al16(loc) && al16(targets) && al16(dcls) && al16(dloc))
    hipLaunchKernelGGL(det_loss_v4_kernel, dim3(grid_for(n * code / 4, 4096)), dim3(256), 0, s, cls, labels, loc, targets,
                       mask, n, code, alpha, gamma, sigma, 1.f / norm, losses, dcls, dloc);
  else
    hipLaunchKernelGGL(det_loss_kernel, dim3(grid_for(n, 2048)), dim3(256), 0, s, cls, labels, loc, targets,
                       mask, n, code, alpha, gamma, sigma, 1.f / norm, losses, dcls, dloc);
  return dn::check_launch("det_loss_kernel");
}

extern "C" int dn_det_loss_corner(const float* cls, const float* labels, const float* loc, const float* targets,
                                  const float* mask, const float* anchors, long per_image, long n, float alpha, float gamma,
                                  float norm, double* losses, float* dcls, float* dloc, void* stream) {
  DN_REQUIRE(cls && labels && loc && targets && mask && anchors && losses && dcls && dloc, "corner loss: null pointer");
  DN_REQUIRE(n > 0 && per_image > 0 && n % per_image == 0 && norm > 0.f,
             "corner loss: bad arguments (n = %ld anchors, %ld per image)", n, per_image);
  hipStream_t s = (hipStream_t)stream;
  if (dn::zero_fill(losses, 2 * sizeof(double), s) != hipSuccess)
    return dn::fail(DN_ERR_LAUNCH, "corner loss: memset failed");
  auto al16 = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; };
  // dn_det_loss' rule (code = 6: n even makes 6 n a multiple of 4)
  if (n % 2 == 0 && al16(cls) && al16(labels) && al16(loc) && al16(targets) && al16(dcls) && al16(dloc))
    hipLaunchKernelGGL(det_loss_corner_v4_kernel, dim3(grid_for(n * 6 / 4, 4096)), dim3(256), 0, s, cls, labels, loc, targets,
                       mask, anchors, per_image, n, alpha, gamma, 1.f / norm, losses, dcls, dloc);
  else
    hipLaunchKernelGGL(det_loss_corner_kernel, dim3(grid_for(n, 2048)), dim3(256), 0, s, cls, labels, loc, targets, mask,
                       anchors, per_image, n, alpha, gamma, 1.f / norm, losses, dcls, dloc);
  return dn::check_launch("det_loss_corner_kernel");
}

extern "C" int dn_adam_step(float* p, const float* g, float* m, float* v, long n, double lr,
                            double beta1, double beta2, double eps, double weight_decay, int step,
                            void* stream) {
  DN_REQUIRE(p && g && m && v && n > 0 && step >= 1, "adam: bad arguments");
  // the scalars of the update in double, as torch.optim.Adam keeps them, each rounded to float once
  const double bc1 = 1.0 - pow(beta1, (double)step);
  const double bc2 = 1.0 - pow(beta2, (double)step);
  hipLaunchKernelGGL(adam_kernel, dim3(grid_for(n, 4096)), dim3(256), 0, (hipStream_t)stream, p, g, m, v,
                     n, (float)(lr / bc1), (float)beta1, (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)eps,
                     (float)weight_decay, (float)sqrt(bc2));
  return dn::check_launch("adam_kernel");
}

// ---------------------------------------------------------------------------------
// knowledge distillation: KLDivLoss(log_softmax(student), softmax(teacher)) over channels
// ---------------------------------------------------------------------------------
namespace {

// one wavefront per row (= pixel of an NHWC map); mean over ALL elements (the reference's
// nn.KLDivLoss(size_average=True, reduce=True)), times `scale` = kd_weight / (rows * c)
__global__ void __launch_bounds__(256)
kd_kl_kernel(const float* __restrict__ student, const float* __restrict__ teacher, long rows, int c,
             float scale, double* __restrict__ loss, float* __restrict__ dstudent) {
  const int lane = threadIdx.x & 63;
  double acc = 0.0;
  for (long row = blockIdx.x * 4L + (threadIdx.x >> 6); row < rows; row += gridDim.x * 4L) {
    const float* s = student + row * c;
    const float* t = teacher + row * c;
    float ms = -INFINITY, mt = -INFINITY;
    for (int k = lane; k < c; k += 64) {
      ms = fmaxf(ms, s[k]);
      mt = fmaxf(mt, t[k]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      ms = fmaxf(ms, __shfl_xor(ms, o, 64));
      mt = fmaxf(mt, __shfl_xor(mt, o, 64));
    }
    float es = 0.f, et = 0.f;
    for (int k = lane; k < c; k += 64) {
      es += expf(s[k] - ms);
      et += expf(t[k] - mt);
    }
    es = wave_sum(es);
    et = wave_sum(et);
    const float lse_s = ms + logf(es), lse_t = mt + logf(et);
    float part = 0.f;
    for (int k = lane; k < c; k += 64) {
      const float ls = s[k] - lse_s;              // log_softmax(student)
      const float lt = t[k] - lse_t;              // log softmax(teacher)
      const float pt = expf(lt);
      if (pt > 0.f) part += pt * (lt - ls);
      dstudent[row * c + k] = (expf(ls) - pt) * scale;
    }
    acc += (double)wave_sum(part);
  }
  __shared__ double red[4];
  if (lane == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) atomic_add_f64(loss, (red[0] + red[1] + red[2] + red[3]) * (double)scale);
}

}  // namespace

extern "C" int dn_kd_kl_loss(const float* student, const float* teacher, long rows, int c, float scale,
                             double* loss, float* dstudent, int zero_loss, void* stream) {
  DN_REQUIRE(student && teacher && loss && dstudent, "kd loss: null pointer");
  DN_REQUIRE(rows > 0 && c > 0, "kd loss: bad shape");
  hipStream_t s = (hipStream_t)stream;
  if (zero_loss && dn::zero_fill(loss, sizeof(double), s) != hipSuccess)
    return dn::fail(DN_ERR_LAUNCH, "kd loss: memset failed");
  const long blocks = (rows + 3) / 4;
  hipLaunchKernelGGL(kd_kl_kernel, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(256), 0, s,
                     student, teacher, rows, c, scale, loss, dstudent);
  return dn::check_launch("kd_kl_kernel");
}
