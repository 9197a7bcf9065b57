// Index maps of the split-planar ("SP") f16 format: where a 16-byte piece of an activation tensor, of a
// packed weight image and of an A-operand fragment image lies, and the LDS images the SP conv engine
// (conv_sp.hip) stages with LDS-DMA.  Pure integer functions, usable from host code
// (tests/c_abi/check_sp_layout.cpp checks bijection, quarter order and ds_read_b128 bank-conflict freedom on
// the CPU) and from the kernels.  The values inside a piece -- hi = half(x), lo = half(x - hi) -- are
// sp_split.h's.  Every unit that reads or writes the format goes through these functions; a hot kernel that
// keeps an index written out (its ISA would change) names the function it restates.
#pragma once
#include <stddef.h>

#if defined(__HIPCC__)
#define SP_HD __host__ __device__ inline
#else
#define SP_HD inline
#endif

namespace sp {

// A piece is 16 bytes = 8 halves = 8 consecutive channels: channels 16 * chunk + 8 * oct + 0..7.
SP_HD constexpr int chunks_of(int c) { return (c + 15) / 16; }
// The four pieces of a chunk: part 0 = hi, part 1 = lo, each for octet 0 and 1 -> hi-oct0, hi-oct1, lo-oct0, lo-oct1.
SP_HD constexpr int quarter_of(int part, int oct) { return 2 * part + oct; }

// SP activation tensor [image][C/16 chunk][4 quarter][H][W] x 16 bytes: piece of pixel px (of hw) of one image.
// A value is x ~= hi + lo (22-bit significand); bytes per element = 4, as fp32.  The piece is the B-operand
// fragment order of v_mfma_f32_32x32x16_f16 (lane (j, h) holds k = 8h..8h+7), so a plane row is at once an HBM
// burst, an LDS-DMA burst and a conflict-free ds_read_b128 source.  `quarters` = 2: the hi-only tensor
// (dn_scatter_dense_sp_hi), whose chunks hold the two hi pieces alone.
SP_HD constexpr size_t act_piece(size_t img, int chunks, size_t chunk, int quarter, size_t hw, size_t px, int quarters = 4) {
  return ((img * chunks + chunk) * quarters + quarter) * hw + px;
}
SP_HD constexpr size_t act_bytes(size_t n_images, int channels, size_t hw, int quarters = 4) {
  return act_piece(n_images, chunks_of(channels), 0, 0, hw, 0, quarters) * 16;
}

// SP packed weights [block][4 quarter][cout_pad] x 16 bytes: piece = input channels 16 * chunk + 8 * oct + 0..7 of
// output channel n.  A plain image has one block per (chunk, tap); the tap-merged images (conv_sp.hip row-merged,
// conv_spq.hip quad-merged) count their own blocks per chunk.
SP_HD constexpr size_t weight_piece(size_t block, int quarter, int cout_pad, int n) {
  return (block * 4 + quarter) * cout_pad + n;
}
SP_HD constexpr size_t weight_bytes(size_t blocks, int cout_pad) { return weight_piece(blocks, 0, cout_pad, 0) * 16; }
SP_HD constexpr int plain_block(int chunk, int taps, int tap) { return chunk * taps + tap; }

// A-operand fragment image [nt][ks][part][h][32 rows] x 16 bytes of a matrix W[rows][cols]: piece = columns
// 16 * ks + 8 * h + 0..7 of row 32 * nt + row (fuse_mlp.hip's MLP weights, conv_sp.hip's post-1x1 weights).
SP_HD constexpr int frag_piece(int nt, int ks, int ksteps, int part, int h, int row) {
  return (((nt * ksteps + ks) * 2 + part) * 2 + h) * 32 + row;
}
SP_HD constexpr size_t frag_bytes(int n_tiles, int ksteps) { return (size_t)frag_piece(n_tiles, 0, ksteps, 0, 0, 0) * 16; }

// ---- LDS images of the SP conv engine ----

// ds_read_b128 is serviced in four 16-lane groups; within the low 32 lanes they are
// g1 = {0-3, 12-15, 20-27} and g2 = {4-11, 16-19, 28-31} (MI355X_MICROARCH.md, LDS).
SP_HD constexpr bool in_g2(int j) { return (j >= 4 && j < 12) || (j >= 16 && j < 20) || j >= 28; }
SP_HD constexpr int rank16(int j) {   // position of lane j inside its 16-lane group
  return j < 4 ? j : j < 12 ? j - 4 : j < 16 ? j - 8 : j < 20 ? j - 8 : j < 28 ? j - 12 : j - 16;
}

// Pixel (row, col) inside the workgroup's TH x TW output tile that MFMA column j of the
// pixel group `gm` (32 pixels) owns.  Chosen so that every 16-lane read group touches 16
// distinct 16-byte LDS slots (mod 16) for every tap:
//   TW = 32: a group is one tile row, column = j (any 16 of 32 consecutive pieces differ mod 16);
//   TW = 16: a group is two rows; each 16-lane read group takes one whole row;
//   TW =  8: four rows {g, g + 4} x {g1, g2}: rows r and r + 4 are 4 * STRIDE * PITCH pieces
//            apart, = 8 (mod 16) for the natural pitches 10 (3x3 s1) and 17 (3x3 s2).
template <int TW>
SP_HD constexpr int tile_row(int gm, int j) {
  if (TW == 32) return gm;
  if (TW == 16) return gm * 2 + (in_g2(j) ? 1 : 0);
  return gm * 2 + (in_g2(j) ? 1 : 0) + 4 * (rank16(j) / 8);   // TW == 8
}
template <int TW>
SP_HD constexpr int tile_col(int j) {
  if (TW == 32) return j;
  if (TW == 16) return rank16(j);
  return rank16(j) % 8;
}

// patch geometry of one workgroup: input rows/cols an output tile reads
template <int KS, int STRIDE, int TH, int TW>
struct Patch {
  static constexpr int PH = (TH - 1) * STRIDE + KS;
  static constexpr int PW = (TW - 1) * STRIDE + KS;
  // stride 2: columns are stored de-interleaved, EVENW even columns then the odd ones, so a
  // tap reads consecutive pieces for consecutive output columns
  static constexpr int EVENW = STRIDE == 2 ? TW + 1 : 0;
  // pieces per patch row; 1x1 with TW = 8 pads 8 -> 10 to keep rows r, r + 4 apart by 8 (mod 16)
  static constexpr int PITCH = (KS == 1 && TW == 8) ? 10 : PW;
  static constexpr int NPIX = PH * PITCH;   // pieces of one (chunk, quarter) plane of the patch
};

// LDS position (piece index inside a quarter plane) of patch pixel (r, cc)
template <int KS, int STRIDE, int TH, int TW>
SP_HD constexpr int patch_pos(int r, int cc) {
  using P = Patch<KS, STRIDE, TH, TW>;
  return r * P::PITCH + (STRIDE == 2 ? ((cc & 1) ? P::EVENW + (cc >> 1) : (cc >> 1)) : cc);
}
// inverse: patch column of position `pos` within a row, or -1 for padding
template <int KS, int STRIDE, int TH, int TW>
SP_HD constexpr int patch_col_of(int pos) {
  using P = Patch<KS, STRIDE, TH, TW>;
  if (STRIDE == 2) {
    if (pos < P::EVENW) return 2 * pos;
    const int cc = 2 * (pos - P::EVENW) + 1;
    return cc < P::PW ? cc : -1;
  }
  return pos < P::PW ? pos : -1;
}
// piece offset a tap adds to an output pixel's base position
template <int KS, int STRIDE, int TH, int TW>
SP_HD constexpr int tap_offset(int ty, int tx) {
  using P = Patch<KS, STRIDE, TH, TW>;
  return ty * P::PITCH + (STRIDE == 2 ? ((tx & 1) ? P::EVENW + (tx >> 1) : (tx >> 1)) : tx);
}
// base position (tap (0, 0)) of output pixel (row, col) of the tile
template <int KS, int STRIDE, int TH, int TW>
SP_HD constexpr int out_base_pos(int row, int col) {
  using P = Patch<KS, STRIDE, TH, TW>;
  return row * STRIDE * P::PITCH + col;   // stride 2: col indexes the even plane (cc = 2 col)
}

}  // namespace sp
