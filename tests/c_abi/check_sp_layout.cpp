// Host-side check of disconet_amd/csrc/sp_layout.h and sp_split.h (no GPU):
//   * the piece indices of an activation tensor, a packed weight image and a fragment image are bijections onto
//     [0, pieces) in the documented order, quarters hi-oct0, hi-oct1, lo-oct0, lo-oct1;
//   * the split of a fixed list of values, printed as (hi, lo) bit patterns (tests/test_c_abi.py holds the expected pairs);
// and for every tile shape of conv_sp.hip's menu
//   * the LDS image map patch_pos / patch_col_of is a bijection between patch pixels and
//     non-padding positions;
//   * an output pixel's tap read (out_base_pos + tap_offset) lands on the position of the
//     input pixel the convolution needs;
//   * the lane -> pixel map covers the tile exactly once;
//   * every 16-lane ds_read_b128 service group touches 16 distinct 16-byte slots (mod 16).
// Build: /opt/rocm/llvm/bin/clang++ -std=c++17 -I disconet_amd/csrc tests/c_abi/check_sp_layout.cpp -o check_sp_layout
// (ROCm's clang as a host compiler: _Float16 on x86 needs clang >= 15 or gcc >= 12)
#include <cstdio>
#include <set>
#include <vector>
#include "sp_layout.h"
#include "sp_split.h"

static int g_bad = 0;
#define EXPECT(c, ...) do { if (!(c)) { ++g_bad; printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

template <int KS, int STRIDE, int TH, int TW>
void check(const char* name, int groups) {
  using P = sp::Patch<KS, STRIDE, TH, TW>;
  // bijection
  std::set<int> seen;
  for (int r = 0; r < P::PH; ++r)
    for (int cc = 0; cc < P::PW; ++cc) {
      const int pos = sp::patch_pos<KS, STRIDE, TH, TW>(r, cc);
      EXPECT(pos >= 0 && pos < P::NPIX, "%s: pos %d out of plane", name, pos);
      EXPECT(seen.insert(pos).second, "%s: position %d used twice", name, pos);
      EXPECT(pos / P::PITCH == r, "%s: row of pos", name);
      EXPECT((sp::patch_col_of<KS, STRIDE, TH, TW>(pos % P::PITCH)) == cc, "%s: inverse col (%d,%d)", name, r, cc);
    }
  for (int pos = 0; pos < P::PITCH; ++pos) {
    const int cc = sp::patch_col_of<KS, STRIDE, TH, TW>(pos);
    EXPECT(cc < P::PW, "%s: inverse beyond patch", name);
    if (cc >= 0) EXPECT((sp::patch_pos<KS, STRIDE, TH, TW>(0, cc)) == pos, "%s: inverse mismatch at %d", name, pos);
  }
  // lane -> pixel coverage and tap reads
  std::set<int> pix;
  for (int gm = 0; gm < groups; ++gm)
    for (int j = 0; j < 32; ++j) {
      const int row = sp::tile_row<TW>(gm, j), col = sp::tile_col<TW>(j);
      EXPECT(row >= 0 && row < TH && col >= 0 && col < TW, "%s: lane pixel (%d,%d) outside tile", name, row, col);
      EXPECT(pix.insert(row * TW + col).second, "%s: pixel (%d,%d) owned twice", name, row, col);
      for (int ty = 0; ty < KS; ++ty)
        for (int tx = 0; tx < KS; ++tx) {
          const int want = sp::patch_pos<KS, STRIDE, TH, TW>(row * STRIDE + ty, col * STRIDE + tx);
          const int got = sp::out_base_pos<KS, STRIDE, TH, TW>(row, col) + sp::tap_offset<KS, STRIDE, TH, TW>(ty, tx);
          EXPECT(want == got, "%s: tap (%d,%d) of pixel (%d,%d): %d != %d", name, ty, tx, row, col, got, want);
        }
    }
  EXPECT((int)pix.size() == TH * TW, "%s: %zu of %d pixels covered", name, pix.size(), TH * TW);
  // bank conflicts: service groups of ds_read_b128 within 32 lanes
  for (int gm = 0; gm < groups; ++gm)
    for (int ty = 0; ty < KS; ++ty)
      for (int tx = 0; tx < KS; ++tx)
        for (int g2 = 0; g2 < 2; ++g2) {
          std::set<int> slots;
          for (int j = 0; j < 32; ++j)
            if (sp::in_g2(j) == (g2 == 1))
              slots.insert((sp::out_base_pos<KS, STRIDE, TH, TW>(sp::tile_row<TW>(gm, j), sp::tile_col<TW>(j)) +
                            sp::tap_offset<KS, STRIDE, TH, TW>(ty, tx)) % 16);
          EXPECT(slots.size() == 16, "%s: group %d tap (%d,%d) half %d: %zu distinct slots", name, gm, ty, tx, g2,
                 slots.size());
        }
  printf("%-22s PH %2d PW %2d pitch %2d plane %4d pieces\n", name, P::PH, P::PW, P::PITCH, P::NPIX);
}

// a piece index visits every value of [0, pieces) exactly once
struct Once {
  std::vector<int> hits;
  const char* name;
  Once(const char* n, size_t pieces) : hits(pieces, 0), name(n) {}
  void add(size_t p) {
    EXPECT(p < hits.size(), "%s: piece %zu outside [0, %zu)", name, p, hits.size());
    if (p < hits.size()) ++hits[p];
  }
  ~Once() {
    for (size_t p = 0; p < hits.size(); ++p) EXPECT(hits[p] == 1, "%s: piece %zu written %d times", name, p, hits[p]);
  }
};

void check_pieces() {
  // quarter order: hi-oct0, hi-oct1, lo-oct0, lo-oct1
  EXPECT(sp::quarter_of(0, 0) == 0 && sp::quarter_of(0, 1) == 1 && sp::quarter_of(1, 0) == 2 && sp::quarter_of(1, 1) == 3,
         "quarter order");
  EXPECT(sp::chunks_of(1) == 1 && sp::chunks_of(16) == 1 && sp::chunks_of(17) == 2 && sp::chunks_of(32) == 2, "chunks_of");
  const int images = 2, hw = 15;
  for (int c : {8, 24, 32}) {
    const int chunks = sp::chunks_of(c);
    EXPECT(sp::act_bytes(images, c, hw) == (size_t)images * chunks * 4 * hw * 16, "act_bytes of %d channels", c);
    Once once("activation piece", sp::act_bytes(images, c, hw) / 16);
    for (int img = 0; img < images; ++img)
      for (int cg = 0; cg < chunks; ++cg)
        for (int part = 0; part < 2; ++part)
          for (int oct = 0; oct < 2; ++oct)
            for (int px = 0; px < hw; ++px) {
              const size_t p = sp::act_piece(img, chunks, cg, sp::quarter_of(part, oct), hw, px);
              once.add(p);
              // [image][chunk][quarter][pixel], pixel fastest; lo lies two quarter planes behind hi
              EXPECT(p == (((size_t)img * chunks + cg) * 4 + 2 * part + oct) * hw + px, "activation piece order");
              EXPECT(sp::act_piece(img, chunks, cg, sp::quarter_of(1, oct), hw, px) ==
                         sp::act_piece(img, chunks, cg, sp::quarter_of(0, oct), hw, px) + 2 * hw, "lo plane offset");
            }
    // the hi-only tensor: two quarters per chunk
    Once hi_only("hi-only activation piece", sp::act_bytes(images, c, hw, 2) / 16);
    for (int img = 0; img < images; ++img)
      for (int cg = 0; cg < chunks; ++cg)
        for (int oct = 0; oct < 2; ++oct)
          for (int px = 0; px < hw; ++px) hi_only.add(sp::act_piece(img, chunks, cg, sp::quarter_of(0, oct), hw, px, 2));
  }
  // weight images: 9 blocks = one chunk of a plain 3x3 layer, 12 + 9 = a row-merged chunk and a plain one
  for (int blocks : {9, 12 + 9})
    for (int cout_pad : {64, 128}) {
      EXPECT(sp::weight_bytes(blocks, cout_pad) == (size_t)blocks * 4 * cout_pad * 16, "weight_bytes");
      Once once("weight piece", sp::weight_bytes(blocks, cout_pad) / 16);
      for (int b = 0; b < blocks; ++b)
        for (int q = 0; q < 4; ++q)
          for (int n = 0; n < cout_pad; ++n) {
            once.add(sp::weight_piece(b, q, cout_pad, n));
            EXPECT(sp::weight_piece(b, q, cout_pad, n) == ((size_t)b * 4 + q) * cout_pad + n, "weight piece order");
          }
    }
  for (int taps : {1, 9}) {
    std::set<int> seen;
    for (int cg = 0; cg < 4; ++cg)
      for (int t = 0; t < taps; ++t) seen.insert(sp::plain_block(cg, taps, t));
    EXPECT((int)seen.size() == 4 * taps && *seen.begin() == 0 && *seen.rbegin() == 4 * taps - 1, "plain_block with %d taps", taps);
  }
  for (int ksteps : {4, 8}) {
    const int n_tiles = 2;
    EXPECT(sp::frag_bytes(n_tiles, ksteps) == (size_t)n_tiles * ksteps * 2 * 2 * 32 * 16, "frag_bytes");
    Once once("fragment piece", sp::frag_bytes(n_tiles, ksteps) / 16);
    for (int nt = 0; nt < n_tiles; ++nt)
      for (int ks = 0; ks < ksteps; ++ks)
        for (int part = 0; part < 2; ++part)
          for (int h = 0; h < 2; ++h)
            for (int row = 0; row < 32; ++row) {
              once.add(sp::frag_piece(nt, ks, ksteps, part, h, row));
              EXPECT(sp::frag_piece(nt, ks, ksteps, part, h, row) == (((nt * ksteps + ks) * 2 + part) * 2 + h) * 32 + row,
                     "fragment piece order");
            }
  }
}

// the split of a fixed list as (hi, lo) bit patterns: tests/test_c_abi.py compares the printed pairs
void print_splits() {
  const float values[] = {1.0009765f, 3.14159265f, -70000.f, 1e-5f, 65519.9f, __builtin_nanf("")};
  float x8[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int i = 0; i < 6; ++i) x8[i] = values[i];
  half8 h8, l8;
  sp::split(x8, h8, l8);
  for (int i = 0; i < 6; ++i) {
    _Float16 hi, lo;
    sp::split(values[i], hi, lo);
    unsigned short hb, lb, hb8, lb8;
    const _Float16 he = h8[i], le = l8[i];
    __builtin_memcpy(&hb, &hi, 2); __builtin_memcpy(&lb, &lo, 2);
    __builtin_memcpy(&hb8, &he, 2); __builtin_memcpy(&lb8, &le, 2);
    EXPECT(hb == hb8 && lb == lb8, "split of 8 differs from split of one at value %d", i);
    if (values[i] == values[i]) {
      const float clamped = values[i] > 65504.f ? 65504.f : values[i] < -65504.f ? -65504.f : values[i];
      const float err = sp::value(hi, lo) - clamped;
      EXPECT((err < 0 ? -err : err) <= (clamped < 0 ? -clamped : clamped) * 0x1p-21f + 0x1p-25f, "value(split(x)) != x at value %d", i);
    }
    printf("split %d: %04x %04x\n", i, hb, lb);
  }
}

int main() {
  check_pieces();
  print_splits();
  int ranks = 0;
  for (int j = 0; j < 32; ++j) ranks += sp::rank16(j);
  EXPECT(ranks == 2 * 120, "rank16 is not a permutation of 0..15 per group");
  check<3, 1, 8, 32>("3x3 s1 8x32", 8);
  check<3, 1, 8, 16>("3x3 s1 8x16", 4);
  check<3, 1, 8, 8>("3x3 s1 8x8", 2);
  check<3, 2, 8, 16>("3x3 s2 8x16", 4);
  check<3, 2, 8, 8>("3x3 s2 8x8", 2);
  check<1, 1, 8, 32>("1x1 8x32", 8);
  check<1, 1, 8, 8>("1x1 8x8", 2);
  check<3, 1, 16, 32>("3x3 s1 16x32", 16);
  printf(g_bad ? "SP LAYOUT CHECK FAILED (%d)\n" : "SP LAYOUT CHECK PASSED\n", g_bad);
  return g_bad ? 1 : 0;
}
