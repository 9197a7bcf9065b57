// Quantised feature exchange (include/disconet_hip.h :: "Feature exchange wire format"): the level-3 map an agent sends,
// encoded as f16 / MXFP8 (E4M3 + E8M0) / MXFP4 (E2M1 + E8M0) and decoded back to fp32 NHWC.  Two streaming kernels, one
// launch each, no atomics, no workspace, no host read: graph-capturable, and the same bytes on every run.
//
// An image is a flat run of h * w * c floats (pixel-major, channel order) and c % 32 == 0, so MX block k of the image is
// floats [32 k, 32 k + 32) and its scale byte is scale[k]: the kernels never look at pixels.  A lane owns one OCTET -- 8
// consecutive floats, two 16-byte loads -- and the 4 lanes of a block fold max |v| with two cross-lane steps.  A wave
// owns 64 octets = 16 blocks of ONE image (waves never straddle images): its payload leaves as one 16 / 8 / 4-byte store
// per lane, and its 16 scale bytes are gathered into lane 0 and leave as ONE 16-byte store.  The scale run of an image is
// padded with zeros to a multiple of 16 bytes, which is exactly the image's waves x 16: the last wave's store writes the
// padding, blocks past the image's end contribute a zero byte.
//
// The conversion is integer arithmetic on the fp32 bits -- the scaled element v * 2^-e is never formed as a float, so no
// rounding mode, denormal mode or contraction can touch it -- and states the contract's rule directly; gfx950's scaled
// converts (v_cvt_scalef32_pk_fp8_f32 / _fp4_f32) are not used: DESIGN.md, "Feature exchange".
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>

#include "dn_internal.h"

namespace {

using u32x4 = __attribute__((ext_vector_type(4))) unsigned;
using u32x2 = __attribute__((ext_vector_type(2))) unsigned;

// element formats: mantissa bits, exponent of the smallest normal binade, largest magnitude code, emax of the scale rule
template <int FMT> struct Elem;
template <> struct Elem<DN_EXCHANGE_MXFP8> { static constexpr int MB = 3, KMIN = -6, MAX_CODE = 0x7E, EMAX = 8, SIGN = 0x80; };
template <> struct Elem<DN_EXCHANGE_MXFP4> { static constexpr int MB = 1, KMIN = 0, MAX_CODE = 0x7, EMAX = 2, SIGN = 0x8; };

// The code of fp32 bits `u` under scale exponent e (the contract's element rule).  |v| = M * 2^(x - 150) with the
// integer significand M < 2^24 (x = max(biased exponent, 1): subnormals have no hidden bit).  With p = msb(M), the scaled
// element lies in binade k = p + x - 150 - e, the format's quantum there is 2^(max(k, KMIN) - MB), and
//     |v| 2^-e / quantum = M >> sh,   sh = max(p - MB, 150 + KMIN - MB + e - x)   (>= 13 for every input: no left shift)
// rounded to nearest even as an integer R.  code = R + (max(k - KMIN, 0) << MB): R carries the hidden bit of a normal
// result, so a mantissa that rounds up to 2^(MB+1) moves into the next exponent by the same addition.  k <= EMAX for every
// element of the block, so the unclamped code is at most MAX_CODE + 2 and min() is the contract's clamp.
template <int FMT>
__device__ inline unsigned elem_code(unsigned u, int e) {
  using F = Elem<FMT>;
  const unsigned a = u & 0x7fffffffu;
  const int ev = (int)(a >> 23);
  const int x = ev > 0 ? ev : 1;
  const unsigned M = (a & 0x7fffffu) | (ev > 0 ? 0x800000u : 0u);
  const int p = 31 - __clz((int)(M | 1u));               // (M == 0: p = 0, R = 0 below)
  const int kk = p + x - 150 - e - F::KMIN;              // k - KMIN
  int sh = p - F::MB - (kk < 0 ? kk : 0);                // = max(p - MB, 150 + KMIN - MB + e - x)
  sh = sh > 31 ? 31 : sh;                                // sh >= 25 rounds every M < 2^24 to 0
  const unsigned R = (M + ((1u << (sh - 1)) - 1u) + ((M >> sh) & 1u)) >> sh;
  unsigned code = R + ((unsigned)(kk > 0 ? kk : 0) << F::MB);
  code = code > (unsigned)F::MAX_CODE ? (unsigned)F::MAX_CODE : code;
  return code | ((u >> 31) ? (unsigned)F::SIGN : 0u);
}

// 2^t as a float, t in [-149, 127]
__device__ inline float pow2f(int t) {
  return __uint_as_float(t >= -126 ? (unsigned)(t + 127) << 23 : 1u << (t + 149));
}

// value(code) * 2^e.  value = I * 2^(max(Eb, 1) - bias - MB) with the integer I < 2^(MB+1); I * 2^t is exact in fp32 for
// every reachable (code, e): t >= -9 - 127 = -136 > -149, and the largest products are 448 * 2^119 and 6 * 2^125 < 2^128.
template <int FMT>
__device__ inline float elem_value(unsigned code, int e) {
  using F = Elem<FMT>;
  const unsigned mag = code & (unsigned)(F::SIGN - 1);
  const int eb = (int)(mag >> F::MB);
  const unsigned mant = mag & ((1u << F::MB) - 1u);
  const unsigned I = eb ? (mant | (1u << F::MB)) : mant;
  float v = (float)I * pow2f((eb ? eb : 1) - 1 + F::KMIN - F::MB + e);
  if (FMT == DN_EXCHANGE_MXFP8 && mag == 0x7Fu) v = __uint_as_float(0x7fc00000u);      // E4M3's NaN code (never encoded)
  return (code & (unsigned)F::SIGN) ? -v : v;
}

struct Geometry {
  long octets;            // 8-float groups of one image: h * w * c / 8
  long waves_per_image;   // ceil(octets / 64)
  long total_waves;       // n_images * waves_per_image
  long message_bytes, payload_bytes;
};

template <int FMT>
__global__ void __launch_bounds__(256)
exchange_encode_kernel(const float* __restrict__ feat, Geometry g, uint8_t* __restrict__ wire) {
  const long gw = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (gw >= g.total_waves) return;                        // the guarded tail of the grid (no barrier in this kernel)
  const int lane = threadIdx.x & 63;
  const long image = gw / g.waves_per_image, wi = gw - image * g.waves_per_image;
  const long q = wi * 64 + lane;
  const bool on = q < g.octets;                           // the image's last wave may be partial, in whole blocks
  u32x4 lo = {0u, 0u, 0u, 0u}, hi = {0u, 0u, 0u, 0u};
  if (on) {
    const u32x4* src = reinterpret_cast<const u32x4*>(feat + (image * g.octets + q) * 8);
    lo = src[0];
    hi = src[1];
  }
  const unsigned u[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  uint8_t* msg = wire + image * g.message_bytes;
  if constexpr (FMT == DN_EXCHANGE_F16) {
    if (!on) return;
    unsigned w[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const unsigned a = __half_as_ushort(__float2half_rn(__uint_as_float(u[2 * k])));
      const unsigned b = __half_as_ushort(__float2half_rn(__uint_as_float(u[2 * k + 1])));
      w[k] = a | (b << 16);
    }
    *reinterpret_cast<u32x4*>(msg + q * 16) = u32x4{w[0], w[1], w[2], w[3]};
  } else {
    using F = Elem<FMT>;
    // max |v| of the block as an integer: fp32 magnitudes order as their bit patterns, and Inf / NaN sort at the top
    unsigned m = 0u;
#pragma unroll
    for (int k = 0; k < 8; ++k) m = max(m, u[k] & 0x7fffffffu);
    m = max(m, (unsigned)__shfl_xor((int)m, 1, 64));
    m = max(m, (unsigned)__shfl_xor((int)m, 2, 64));
    const bool bad = m >= 0x7f800000u;
    int e = (int)(m >> 23) - 127 - F::EMAX;               // a subnormal or zero maximum has exponent field 0: below -127
    e = e < -127 ? -127 : e;
    const unsigned scale = !on ? 0u : (bad ? 0xFFu : (unsigned)(e + 127));
    unsigned code[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) code[k] = bad ? 0u : elem_code<FMT>(u[k], e);
    if (on) {
      if (FMT == DN_EXCHANGE_MXFP8) {
        *reinterpret_cast<u32x2*>(msg + q * 8) =
            u32x2{code[0] | (code[1] << 8) | (code[2] << 16) | (code[3] << 24),
                  code[4] | (code[5] << 8) | (code[6] << 16) | (code[7] << 24)};
      } else {
        *reinterpret_cast<unsigned*>(msg + q * 4) = code[0] | (code[1] << 4) | (code[2] << 8) | (code[3] << 12) |
                                                    (code[4] << 16) | (code[5] << 20) | (code[6] << 24) | (code[7] << 28);
      }
    }
    // the wave's 16 scale bytes: byte (lane / 4) % 4 of word lane / 16, OR-folded over each 16-lane group, then the four
    // words to lane 0 -- one 16-byte store per wave
    unsigned word = (lane & 3) == 0 ? scale << (8 * ((lane >> 2) & 3)) : 0u;
    word |= (unsigned)__shfl_xor((int)word, 4, 64);
    word |= (unsigned)__shfl_xor((int)word, 8, 64);
    const unsigned w1 = (unsigned)__shfl((int)word, 16, 64), w2 = (unsigned)__shfl((int)word, 32, 64),
                   w3 = (unsigned)__shfl((int)word, 48, 64);
    if (lane == 0) *reinterpret_cast<u32x4*>(msg + g.payload_bytes + wi * 16) = u32x4{word, w1, w2, w3};
  }
}

template <int FMT>
__global__ void __launch_bounds__(256)
exchange_decode_kernel(const uint8_t* __restrict__ wire, Geometry g, float* __restrict__ feat) {
  const long gw = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (gw >= g.total_waves) return;
  const int lane = threadIdx.x & 63;
  const long image = gw / g.waves_per_image, wi = gw - image * g.waves_per_image;
  const long q = wi * 64 + lane;
  if (q >= g.octets) return;
  const uint8_t* msg = wire + image * g.message_bytes;
  float v[8];
  if constexpr (FMT == DN_EXCHANGE_F16) {
    const u32x4 w = *reinterpret_cast<const u32x4*>(msg + q * 16);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      v[2 * k] = __half2float(__ushort_as_half((unsigned short)(w[k] & 0xffffu)));
      v[2 * k + 1] = __half2float(__ushort_as_half((unsigned short)(w[k] >> 16)));
    }
  } else {
    const unsigned scale = msg[g.payload_bytes + (q >> 2)];
    const int e = (int)scale - 127;
    unsigned code[8];
    if (FMT == DN_EXCHANGE_MXFP8) {
      const u32x2 w = *reinterpret_cast<const u32x2*>(msg + q * 8);
#pragma unroll
      for (int k = 0; k < 8; ++k) code[k] = (w[k >> 2] >> (8 * (k & 3))) & 0xffu;
    } else {
      const unsigned w = *reinterpret_cast<const unsigned*>(msg + q * 4);
#pragma unroll
      for (int k = 0; k < 8; ++k) code[k] = (w >> (4 * k)) & 0xfu;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k)
      v[k] = scale == 0xFFu ? __uint_as_float(0x7fc00000u) : elem_value<FMT>(code[k], e);
  }
  float* dst = feat + (image * g.octets + q) * 8;
  using f32x4v = __attribute__((ext_vector_type(4))) float;
  *reinterpret_cast<f32x4v*>(dst) = f32x4v{v[0], v[1], v[2], v[3]};
  *reinterpret_cast<f32x4v*>(dst + 4) = f32x4v{v[4], v[5], v[6], v[7]};
}

// bytes of one image's message, or -1 (the shape / format is refused)
long message_bytes_of(int format, int h, int w, int c, long* payload) {
  if (h <= 0 || w <= 0 || c <= 0 || c % 32 != 0) return -1;
  const long values = (long)h * w * c;
  if (values >= ((long)1 << 31)) return -1;
  const long scales = (values / 32 + 15) / 16 * 16;
  long p, s = 0;
  switch (format) {
    case DN_EXCHANGE_F32: p = values * 4; break;
    case DN_EXCHANGE_F16: p = values * 2; break;
    case DN_EXCHANGE_MXFP8: p = values; s = scales; break;
    case DN_EXCHANGE_MXFP4: p = values / 2; s = scales; break;
    default: return -1;
  }
  if (payload) *payload = p;
  return p + s;
}

int geometry_of(const char* who, const void* a, const void* b, int n_images, int h, int w, int c, int format, Geometry* g) {
  DN_REQUIRE(a && b, "%s: null pointer", who);
  DN_REQUIRE(format == DN_EXCHANGE_F16 || format == DN_EXCHANGE_MXFP8 || format == DN_EXCHANGE_MXFP4,
             "%s: format %d is none of DN_EXCHANGE_F16 1, DN_EXCHANGE_MXFP8 2, DN_EXCHANGE_MXFP4 3 (DN_EXCHANGE_F32 0 is the "
             "identity: there is nothing to launch)", who, format);
  DN_REQUIRE(n_images > 0 && h > 0 && w > 0, "%s: empty problem", who);
  DN_REQUIRE(c > 0 && c % 32 == 0, "%s: channel count %d must be a multiple of 32 (one scale per 32 channels of a pixel)",
             who, c);
  g->message_bytes = message_bytes_of(format, h, w, c, &g->payload_bytes);
  DN_REQUIRE(g->message_bytes > 0, "%s: a %d x %d x %d map is past 2^31 values", who, h, w, c);
  DN_REQUIRE((((size_t)a | (size_t)b) & 15) == 0, "%s: feat and wire must be 16-byte aligned", who);
  g->octets = (long)h * w * c / 8;
  g->waves_per_image = (g->octets + 63) / 64;
  g->total_waves = g->waves_per_image * n_images;
  DN_REQUIRE((g->total_waves + 3) / 4 <= 0x7fffffffL, "%s: %d images of %d x %d x %d are past the grid limit", who, n_images,
             h, w, c);
  return DN_OK;
}

}  // namespace

extern "C" long dn_exchange_message_bytes(int format, int h, int w, int c) {
  const long bytes = message_bytes_of(format, h, w, c, nullptr);
  if (bytes < 0)
    return dn::fail(DN_ERR_ARG, "exchange message bytes: format %d, map %d x %d x %d (formats 0..3, c a multiple of 32, "
                    "fewer than 2^31 values)", format, h, w, c);
  return bytes;
}

#define DN_EXCHANGE_BY_FORMAT(format, LAUNCH)                         \
  do {                                                                \
    if ((format) == DN_EXCHANGE_F16) { LAUNCH(DN_EXCHANGE_F16); }     \
    else if ((format) == DN_EXCHANGE_MXFP8) { LAUNCH(DN_EXCHANGE_MXFP8); } \
    else { LAUNCH(DN_EXCHANGE_MXFP4); }                               \
  } while (0)

extern "C" int dn_exchange_encode(const float* feat, int n_images, int h, int w, int c, int format, uint8_t* wire,
                                  void* stream) {
  Geometry g;
  if (int rc = geometry_of("exchange encode", feat, wire, n_images, h, w, c, format, &g)) return rc;
  const dim3 grid((unsigned)((g.total_waves + 3) / 4));
#define DN_LAUNCH(F) hipLaunchKernelGGL(exchange_encode_kernel<F>, grid, dim3(256), 0, (hipStream_t)stream, feat, g, wire)
  DN_EXCHANGE_BY_FORMAT(format, DN_LAUNCH);
#undef DN_LAUNCH
  return dn::check_launch("exchange_encode_kernel");
}

extern "C" int dn_exchange_decode(const uint8_t* wire, int n_images, int h, int w, int c, int format, float* feat,
                                  void* stream) {
  Geometry g;
  if (int rc = geometry_of("exchange decode", wire, feat, n_images, h, w, c, format, &g)) return rc;
  const dim3 grid((unsigned)((g.total_waves + 3) / 4));
#define DN_LAUNCH(F) hipLaunchKernelGGL(exchange_decode_kernel<F>, grid, dim3(256), 0, (hipStream_t)stream, wire, g, feat)
  DN_EXCHANGE_BY_FORMAT(format, DN_LAUNCH);
#undef DN_LAUNCH
  return dn::check_launch("exchange_decode_kernel");
}
