// Device phases shared by the split-planar conv kernels -- conv_sp_kernel (conv_sp.hip), conv_spq_kernel (conv_spq.hip)
// and conv_pre_pair_kernel (conv_pre_pair.inl): the work-item order, the K-slice bookkeeping, the three-product MFMA
// group and the register epilogue's two stores.  Each is written once, as a template over what differs between the
// kernels (accumulator tiles per wave, waves per workgroup); what a kernel multiplies the item by (BN / TH / TW), where
// its affine comes from and how its K loop is scheduled stay in the kernel.  Everything is force-inlined: the
// accumulator arrays are passed by reference and must stay registers.  Scalars too are taken by const reference, as a
// lambda's captures are: a phase then reads the kernel's own variable where it uses it, and the instantiations that sit
// on a register step keep their allocation (by-value copies moved conv_spq_kernel<64> from 1 spilled VGPR to 6).
// gfx950 only.
#pragma once
#include "sp_device.h"

namespace {

#define SP_PHASE __device__ __attribute__((always_inline)) inline

// ---------------------------------------------------------------------------------------------------------------------
// Work items.  A launch's items are (channel block, image, tile y, tile x); workgroup b runs on XCD b % 8 (observed,
// not a contract -- a wrong guess only costs speed) and each XCD has its own L2.  The XCD-aware order: all channel
// blocks of a pixel tile take ids b, b + 8, b + 16, ... (same XCD, dispatched back to back: the patch comes out of that
// L2 once per tile, not once per channel block), and each XCD walks its own contiguous run of pixel tiles, so tiles
// that share halo rows / columns meet in one L2 as well.  The last spatial_items % 8 pixel tiles come in plain order.
// conv_mfma.hip's decode is the same formula with integer divisions.
// Part of the kernels' argument structs, filled by item_order_of().  The kernel multiplies n_images x tiles_y x tiles_x
// itself: with that product passed in, conv_sp_kernel's 256-VGPR tiles spill (tools/kernel_resources.py).
struct ItemOrder {
  int tiles_x, tiles_y;
  int items;                       // work items the launch walks: pixel tiles x n_cb (a K-sliced launch sets its own count)
  int n_images, n_cb;              // images; channel blocks
  float rcp_ncb, rcp_tx, rcp_ty;   // reciprocals of the decode's divisors (sp_device.h :: fdivmod)
};
// (host side; the launcher has checked n_images x tiles_y x tiles_x x n_cb < 2^22, fdivmod's range)
inline ItemOrder item_order_of(int n_images, int tiles_y, int tiles_x, int n_cb = 1) {
  const int spatial = n_images * tiles_y * tiles_x;
  return ItemOrder{tiles_x, tiles_y, spatial * n_cb, n_images, n_cb, 1.0f / (float)n_cb, 1.0f / (float)tiles_x,
                   1.0f / (float)tiles_y};
}
struct Item {
  int cb, img, ty, tx;
};
// CB = false: a launch without channel blocks (the stem pair): n_cb and rcp_ncb are not read
template <bool CB = true>
SP_PHASE Item decode_item(const ItemOrder& o, const int& item) {
  const int spatial_items = o.n_images * o.tiles_y * o.tiles_x;
  const int sp_full = spatial_items & ~7;
  Item t;
  int spi;
  if constexpr (!CB) {
    t.cb = 0;
    spi = item < sp_full ? (item & 7) * (sp_full >> 3) + (item >> 3) : item;
  } else if (item < sp_full * o.n_cb) {
    const int j = item >> 3;
    const int jq = fdivmod(j, o.n_cb, o.rcp_ncb, t.cb);
    spi = (item & 7) * (sp_full >> 3) + jq;
  } else {
    const int r = item - sp_full * o.n_cb, rem = spatial_items - sp_full;   // the last < 8 spatial items: rare
    t.cb = r / rem;
    spi = sp_full + r % rem;
  }
  spi = fdivmod(spi, o.tiles_x, o.rcp_tx, t.tx);
  t.img = fdivmod(spi, o.tiles_y, o.rcp_ty, t.ty);
  return t;
}

// ---------------------------------------------------------------------------------------------------------------------
// K slices (sp_device.h :: KSlices).  Work item v < n_whole is a whole tile (all K slices, folded in registers); the
// others are single slices of the tiles behind them, `count` consecutive work items per tile.
// sl0 .. sl1: the slices the item computes (all of them: a whole tile; one: a split tile's slice `sl0`, partial index
// j = v - n_whole = tile * count + slice; a whole tile has j = -1).
template <class Tile>
struct KWork {
  Tile tc;
  int sl0, sl1, j;
};
template <int KSL, class Decode>
SP_PHASE auto ks_decode_work(const KSlices& ks, const int& v, Decode&& decode) {
  KWork<decltype(decode(0))> w;
  if (KSL == 0 || v < ks.n_whole) {
    w.tc = decode(v);
    w.sl0 = 0; w.sl1 = KSL ? ks.count : 1; w.j = -1;
  } else {
    w.j = v - ks.n_whole;
    w.sl0 = w.j & ((1 << ks.log2) - 1);
    w.sl1 = w.sl0 + 1;
    w.tc = decode(ks.n_whole + (w.j >> ks.log2));
  }
  return w;
}
template <int KSL, class Work>
SP_PHASE int ks_first_group(const KSlices& ks, const Work& w) { return KSL ? ks.bound(w.sl0) : 0; }

// The sum, in slice order and starting from zero, of the slices' accumulation chains lives in a second accumulator set
// `tot`.  A whole tile and the fix-up pass add with the SAME function: that is what makes a result independent of how
// its slices were distributed (tests/test_gpu_conv.py :: test_k_sliced_conv_is_batch_invariant).
template <int M, int N>
SP_PHASE void ks_fold(f32x16 (&tot)[M][N], f32x16 (&acc)[M][N]) {   // tot += acc (fp32 adds), acc = 0
#pragma unroll
  for (int wm = 0; wm < M; ++wm)
#pragma unroll
    for (int wn = 0; wn < N; ++wn)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        tot[wm][wn][r] += acc[wm][wn][r];
        acc[wm][wn][r] = 0.f;
      }
}
template <int M, int N>
SP_PHASE void acc_zero(f32x16 (&acc)[M][N]) {
#pragma unroll
  for (int wm = 0; wm < M; ++wm)
#pragma unroll
    for (int wn = 0; wn < N; ++wn)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[wm][wn][r] = 0.f;
}
template <int M, int N>
SP_PHASE void acc_move(f32x16 (&dst)[M][N], const f32x16 (&src)[M][N]) {
#pragma unroll
  for (int wm = 0; wm < M; ++wm)
#pragma unroll
    for (int wn = 0; wn < N; ++wn) dst[wm][wn] = src[wm][wn];
}
// Partial sums of a split tile <-> global memory: one f32x4 per lane and register quad (1 KB runs).  j = tile * count +
// slice; NW waves per workgroup, NACC accumulator tiles per wave.
template <int NW, int NACC>
SP_PHASE float* ks_partial_of(const KSlices& ks, const int& j, const int& wave, const int& lane) {
  return ks.partial + ((size_t)j * NW + wave) * (NACC * 16 * 64) + lane * 4;
}
template <int M, int N>
SP_PHASE void ks_store_partial(float* pb, const f32x16 (&acc)[M][N]) {   // raw accumulators, no affine
#pragma unroll
  for (int wm = 0; wm < M; ++wm)
#pragma unroll
    for (int wn = 0; wn < N; ++wn)
#pragma unroll
      for (int q = 0; q < 4; ++q)
        *reinterpret_cast<f32x4*>(pb + ((wm * N + wn) * 4 + q) * 256) =
            f32x4{acc[wm][wn][4 * q], acc[wm][wn][4 * q + 1], acc[wm][wn][4 * q + 2], acc[wm][wn][4 * q + 3]};
}
template <int M, int N>
SP_PHASE void ks_load_partial(const float* pb, f32x16 (&acc)[M][N]) {
#pragma unroll
  for (int wm = 0; wm < M; ++wm)
#pragma unroll
    for (int wn = 0; wn < N; ++wn)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(pb + ((wm * N + wn) * 4 + q) * 256);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[wm][wn][4 * q + e] = v[e];
      }
}
// The fix-up pass of a K-sliced launch (ks.fixup): the split tiles' slices, added in slice order from zero -- the
// arithmetic of a whole tile's ks_fold -- then the kernel's ordinary epilogue.  No operand DMA, no LDS.
// decode(item) -> the kernel's tile (with a channel origin n0), load_affine(n0), epilogue(tile).
template <int NW, int M, int N, class Decode, class LoadAffine, class Epilogue>
SP_PHASE void ks_fixup(const KSlices& ks, const int& wave, const int& lane, f32x16 (&acc)[M][N], f32x16 (&tot)[M][N], Decode&& decode,
                       LoadAffine&& load_affine, Epilogue&& epilogue) {
  for (int p = blockIdx.x; p < ks.n_split; p += gridDim.x) {
    const auto tc = decode(ks.n_whole + p);
    load_affine(tc.n0);
    acc_zero(tot);
    for (int sl = 0; sl < ks.count; ++sl) {
      ks_load_partial(ks_partial_of<NW, M * N>(ks, (p << ks.log2) + sl, wave, lane), acc);
      ks_fold(tot, acc);
    }
    acc_move(acc, tot);
    epilogue(tc);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// One product group of the split-f16 x3 arithmetic on the M x N accumulator tiles of a wave: x = hi + lo on both sides,
// products lo.hi, hi.lo, hi.hi (small terms first), D[i = channel][j = pixel].  HI_ONLY: the activations are exact in
// binary16 (no lo fragments; `al` is not read): two products.
// The accumulator tiles of a product are walked in Gray order -- consecutive MFMAs then differ in ONE operand register
// set, not two; independent accumulators are interleaved.  Every accumulator still receives its products in the same
// order: same bits as any other walk.
template <bool HI_ONLY = false, int M, int N>
SP_PHASE void mma_x3(f32x16 (&acc)[M][N], const half8 (&ah)[M], const half8 (&al)[M], const half8 (&bh)[N],
                     const half8 (&bl)[N]) {
#pragma unroll
  for (int wm = 0; wm < M; ++wm)
#pragma unroll
    for (int k = 0; k < N; ++k) {
      const int wn = (wm & 1) ? N - 1 - k : k;
      acc[wm][wn] = __builtin_amdgcn_mfma_f32_32x32x16_f16(bl[wn], ah[wm], acc[wm][wn], 0, 0, 0);
    }
  if constexpr (!HI_ONLY) {
#pragma unroll
    for (int wm = 0; wm < M; ++wm)
#pragma unroll
      for (int k = 0; k < N; ++k) {
        const int wn = (wm & 1) ? N - 1 - k : k;
        acc[wm][wn] = __builtin_amdgcn_mfma_f32_32x32x16_f16(bh[wn], al[wm], acc[wm][wn], 0, 0, 0);
      }
  }
#pragma unroll
  for (int wm = 0; wm < M; ++wm)
#pragma unroll
    for (int k = 0; k < N; ++k) {
      const int wn = (wm & 1) ? N - 1 - k : k;
      acc[wm][wn] = __builtin_amdgcn_mfma_f32_32x32x16_f16(bh[wn], ah[wm], acc[wm][wn], 0, 0, 0);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Register epilogue of one 32-pixel x 32-channel accumulator tile, AFTER the kernel's affine: quad(g) is the affine'd
// register quad g (this lane's channels 8 g + 4 lh .. + 3 of the tile, no ReLU applied).  No LDS.
//
// SP output.  Stores are buffer stores against a descriptor of the output IMAGE (32-bit lane offset computed once per
// pixel + the quarter-plane offset; a lane outside the map carries an out-of-range offset and the bounds check drops its
// store): no 64-bit address arithmetic and no exec-mask juggling per store.
struct SpOut {
  __amdgpu_buffer_rsrc_t rsrc;
  int plane;   // bytes of one quarter plane (the launchers check the image < 2 GiB)
  int cog;     // 16-channel chunks of the output tensor
};
SP_PHASE SpOut sp_out_of(unsigned char* const& out, const int& img, const int& cog, const int& h, const int& w) {
  const int plane = h * w * 16, img_bytes = cog * 4 * plane;
  return SpOut{__builtin_amdgcn_make_buffer_rsrc(out + (size_t)img * img_bytes, 0, img_bytes, 0x00020000), plane, cog};
}
SP_PHASE int sp_out_voff(const SpOut& o, const bool& inside, const int& pixel, const int& lh) {   // pixel = oy * w + ox
  return inside ? pixel * 16 + lh * o.plane : (int)0x80000000;
}
// quads -> split4 -> gather_octet -> two 16-byte stores per chunk: chunks cg0, cg0 + 1 of the output tensor.  The ReLU
// rides in the split's lower clamp bound `lo_clamp` (0 or -65504; sp_device.h :: split4).
// NO_STORE (the tools' timing ablations only): the stores stay in the code behind a test that never holds.
template <bool NO_STORE = false, class Quad>
SP_PHASE void store_sp_quads(Quad&& quad, const SpOut& o, const int& voff, const int& cg0, const float& lo_clamp,
                             float& amax) {
  u32x2 hi[4], lo[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) split4(quad(g), hi[g], lo[g], amax, lo_clamp);
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    // chunk cg0 + m: lane half 0 ends up with octet 0, lane half 1 with octet 1
    const u32x4 ph = gather_octet(hi[2 * m], hi[2 * m + 1]);
    const u32x4 pl = gather_octet(lo[2 * m], lo[2 * m + 1]);
    const int cg = cg0 + m;
    if (cg < o.cog && (!NO_STORE || ph[0] == 0x12345678u)) {
      // The plane offset rides in the VECTOR offset, the scalar offset operand stays 0.  With it in the scalar
      // operand hipcc leaves out the wait states between a dwordx4 store and a VALU write of its data registers
      // (its hazard recognizer exempts SGPR offsets; gfx950 needs them): the round-3 form wrote ~1e-4 of the lo
      // pieces wrong, lanes 12-15 / 28-31 of both halves.  DESIGN.md 3.6 (C); tools/soff; tests/test_isa_hazard_cpu.py.
      __builtin_amdgcn_raw_buffer_store_b128(ph, o.rsrc, voff + cg * 4 * o.plane, 0, 0);
      __builtin_amdgcn_raw_buffer_store_b128(pl, o.rsrc, voff + (cg * 4 + 2) * o.plane, 0, 0);
    }
  }
}
// fp32 NHWC output: the same values as one pixel's row `orow`, channels ch0 + 8 g + 4 lh .. + 3 below c_lim.  ReLU is a
// max against a uniform floor (0 or -inf).  The fp32 copy leaves the engine (fusion kernels, the agent all-gather, the
// training step): the one place where a NaN / Inf test of the conv stack is free -- behind the caller's uniform branch.
// Before the ReLU, which would hide a NaN.
template <class Quad>
SP_PHASE void store_f32_quads(Quad&& quad, float* const& orow, const int& ch0, const int& lh, const int& c_lim,
                              const bool& inside, const float& floor_v, bool& nan_seen) {
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const int co = ch0 + 8 * g + 4 * lh;
    f32x4 v = quad(g);
    nan_seen |= !(fabsf(v[0]) <= 3.4028235e38f) | !(fabsf(v[1]) <= 3.4028235e38f) | !(fabsf(v[2]) <= 3.4028235e38f) |
                !(fabsf(v[3]) <= 3.4028235e38f);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], floor_v);
    if (inside && co < c_lim) *reinterpret_cast<f32x4*>(orow + co) = v;
  }
}

#undef SP_PHASE

}  // namespace
