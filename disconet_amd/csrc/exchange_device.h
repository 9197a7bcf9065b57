// Device helpers of the feature-exchange wire format (include/disconet_hip.h :: "Feature exchange wire format"), shared by
// the dense kernels of exchange.hip and the selective ones of exchange_cells.hip: the element formats, the integer
// conversions, and the encode / decode body of one OCTET -- 8 consecutive floats of a message, one lane's work.
//
// The conversion is integer arithmetic on the fp32 bits -- the scaled element v * 2^-e is never formed as a float, so no
// rounding mode, denormal mode or contraction can touch it -- and states the contract's rule directly; gfx950's scaled
// converts (v_cvt_scalef32_pk_fp8_f32 / _fp4_f32) are not used: DESIGN.md, "Feature exchange".
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>

#include "disconet_hip.h"

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

// Encode octet q of an image's message: `u` are its 8 fp32 bit patterns (zeros when !on), wi the wave's index inside the
// image (q = wi * 64 + lane), msg the message's first byte.  Every lane of the wave must call this -- the block maximum
// and the scale bytes fold across lanes -- and `on` may be false only in the image's last wave, in whole blocks.  The
// payload leaves as one 16 / 8 / 4-byte store per lane, and the wave's 16 scale bytes as ONE 16-byte store of lane 0 at
// payload_bytes + wi * 16: blocks past the image's end contribute the zero padding.
template <int FMT>
__device__ inline void encode_octet(const unsigned (&u)[8], bool on, long q, long wi, int lane, uint8_t* msg,
                                    long payload_bytes) {
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
    if (lane == 0) *reinterpret_cast<u32x4*>(msg + payload_bytes + wi * 16) = u32x4{word, w1, w2, w3};
  }
}

// Decode octet q of an image's message to 8 floats: no cross-lane step, any lane may call it alone.
template <int FMT>
__device__ inline void decode_octet(const uint8_t* msg, long payload_bytes, long q, float (&v)[8]) {
  if constexpr (FMT == DN_EXCHANGE_F16) {
    const u32x4 w = *reinterpret_cast<const u32x4*>(msg + q * 16);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      v[2 * k] = __half2float(__ushort_as_half((unsigned short)(w[k] & 0xffffu)));
      v[2 * k + 1] = __half2float(__ushort_as_half((unsigned short)(w[k] >> 16)));
    }
  } else {
    const unsigned scale = msg[payload_bytes + (q >> 2)];
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
}

// bytes of the dense message of one [h][w][c] image, or -1 (the shape / format is refused); *payload: the bytes before
// the scale run
inline long exchange_message_bytes_of(int format, int h, int w, int c, long* payload) {
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

}  // namespace
