// The values of the split-planar ("SP") f16 format: one float as two halves, x ~= hi + lo, and the pack bodies
// that are shared between translation units.  Where the halves are stored is sp_layout.h's.  No DMA or wait-count
// assembly here (that is sp_device.h): a host program can include this header (tests/c_abi/check_sp_layout.cpp
// prints the split of a fixed list) as well as every unit that packs, converts or resamples the format.
//
// sp_device.h :: split4 is the epilogues' instruction sequence (packed convert, v_fma_mix); it equals split() on
// every finite value and differs on NaN.
#pragma once
#include <math.h>
#include "sp_layout.h"

typedef _Float16 half8 __attribute__((ext_vector_type(8)));

namespace sp {

// Clamp to the finite f16 range, hi = half(x), lo = half(x - hi) (the difference is exact in fp32).
// fminf(fmaxf()): a NaN becomes -65504 (fmaxf returns its other operand), hi = 0xfbff, lo = 0.
SP_HD void split(float x, _Float16& hi, _Float16& lo) {
  x = fminf(fmaxf(x, -65504.f), 65504.f);
  hi = (_Float16)x;
  lo = (_Float16)(x - (float)hi);
}
SP_HD void split(const float (&x)[8], half8& hi, half8& lo) {   // one piece: 8 channels of a pixel / of an output channel
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    _Float16 h, l;
    split(x[e], h, l);
    hi[e] = h;
    lo[e] = l;
  }
}
SP_HD float value(_Float16 hi, _Float16 lo) { return (float)hi + (float)lo; }

#if defined(__HIPCC__)
// The hi and lo piece of the same 8 values: `hi_piece` is the piece index of the hi quarter (sp_layout.h), the lo
// quarter lies `lo_step` pieces behind it (two quarters: 2 * hw in a tensor, 2 * cout_pad in a weight image).
__device__ inline void load_pair(const unsigned char* base, size_t hi_piece, size_t lo_step, half8& hi, half8& lo) {
  hi = *reinterpret_cast<const half8*>(base + hi_piece * 16);
  lo = *reinterpret_cast<const half8*>(base + (hi_piece + lo_step) * 16);
}
__device__ inline void store_pair(unsigned char* base, size_t hi_piece, size_t lo_step, const half8 hi, const half8 lo) {
  *reinterpret_cast<half8*>(base + hi_piece * 16) = hi;
  *reinterpret_cast<half8*>(base + (hi_piece + lo_step) * 16) = lo;
}
__device__ inline void split_store(unsigned char* base, size_t hi_piece, size_t lo_step, const float (&x)[8]) {
  half8 hi, lo;
  split(x, hi, lo);
  store_pair(base, hi_piece, lo_step, hi, lo);
}

// The A-operand fragment image (sp_layout.h :: frag_piece) of w [rows][cols] * wmul, rows / cols past the matrix
// zero; `col0` = first column inside the source matrix (row stride ld).  One thread per (nt, ks, h, row).
__device__ inline void pack_frags(const float* __restrict__ w, int ld, int col0, int rows, int cols, int n_tiles,
                                  int ksteps, float wmul, unsigned char* __restrict__ out) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n_tiles * ksteps * 2 * 32) return;
  const int row = idx % 32, h = (idx / 32) % 2, ks = (idx / 64) % ksteps, nt = idx / (64 * ksteps);
  float v[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int r = nt * 32 + row, c = ks * 16 + h * 8 + e;
    v[e] = (r < rows && c < cols) ? w[(size_t)r * ld + col0 + c] * wmul : 0.f;
  }
  split_store(out, frag_piece(nt, ks, ksteps, 0, h, row), frag_piece(0, 0, ksteps, 1, 0, 0), v);
}
#endif

}  // namespace sp
