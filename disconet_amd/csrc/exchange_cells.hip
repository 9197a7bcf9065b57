// Selective feature exchange (include/disconet_hip.h :: "Selective exchange"): an agent sends the K strongest cells of
// its map -- a 16-byte header, the ascending list of their indices, and the dense message (exchange.hip's formats) of the
// gathered [1][K][c] image.  Encode is three launches, decode one; integer LDS atomics only, no global atomics, no host
// read: graph-capturable, and the same bytes on every run.
//
//   score   grid-wide and streaming, the only pass over the whole map.  A cell's c floats are contiguous: a group of G
//           lanes (G = the largest power of two <= min(64, c / 8)) owns a cell, each lane folds the integer max of its
//           octets (two 16-byte loads each), log2 G cross-lane max steps finish the cell.  score [n][P] uint32.
//   select  one 1024-lane workgroup per image, the scores in LDS.  Radix select of the K-th largest score T: four 8-bit
//           digits from the top, a 256-bin LDS histogram each, the bin found by wave 0 with one wave scan.  Then one pass
//           per 1024 cells: wave ballots of "score > T" and "score == T" give every wave's counts, wave 0 scans the <= 256
//           counts, and a cell's slot is (cells above T before it) + min(cells equal to T before it, cells equal to T
//           still needed) -- ascending cell index, ties to the lower index.  T == 0 sends no tie: an all-zero cell never
//           leaves.  Writes the header, the index list with its 0xFFFF tail and zero padding, and sent_cells.
//   pack    the dense encoder's octet body (exchange_device.h) with one indirection: row r of the body reads cell
//           index[r], rows >= count read zeros; f32 is a copy.
//   decode  over all P cells of every image: each octet's lane binary-searches the ascending index list (<= 14 steps,
//           served from L2) and writes its decoded row or zeros.  No memset, no atomics, no races; the search never
//           leaves [0, min(count, K)), so a malformed list cannot fault.
#include <hip/hip_runtime.h>

#include "dn_internal.h"
#include "exchange_device.h"

namespace {

using f32x4v = __attribute__((ext_vector_type(4))) float;

constexpr int kSelectThreads = 1024;                      // 16 waves: 16 rounds of 1024 cells cover DN_EXCHANGE_CELLS_MAX
constexpr int kSelectRounds = DN_EXCHANGE_CELLS_MAX / kSelectThreads;
static_assert(kSelectRounds * (kSelectThreads / 64) == 256, "the wave counts of one image are one 256-entry scan");

struct CellGeometry {
  int cells, capacity;    // P = h * w, K
  int row_octets;         // c / 8
  int group;              // lanes of the score launch that share a cell
  long total_cells;       // n_images * P
  long message_bytes;     // one image's whole message
  long body_offset;       // 16 + pad16(2 K)
  long payload_bytes;     // of the body (the scale run follows)
  long body_octets;       // K * c / 8
  long body_waves;        // ceil(body_octets / 64)
  long map_octets;        // P * c / 8
  long map_waves;         // ceil(map_octets / 64)
  long n_images;
};

__global__ void __launch_bounds__(256)
exchange_cells_score_kernel(const float* __restrict__ feat, CellGeometry g, unsigned* __restrict__ score) {
  const long gw = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int G = g.group;
  const long cell = gw * (64 / G) + lane / G;             // no early return: every lane takes the cross-lane steps
  const int sub = lane & (G - 1);
  const bool on = cell < g.total_cells;
  unsigned m = 0u;
  if (on) {
    const u32x4* src = reinterpret_cast<const u32x4*>(feat + cell * g.row_octets * 8);
    for (int o = sub; o < g.row_octets; o += G) {
      const u32x4 lo = src[2 * o], hi = src[2 * o + 1];
#pragma unroll
      for (int k = 0; k < 4; ++k) m = max(m, max(lo[k] & 0x7fffffffu, hi[k] & 0x7fffffffu));
    }
  }
  for (int s = 1; s < G; s <<= 1) m = max(m, (unsigned)__shfl_xor((int)m, s, 64));
  if (on && sub == 0) score[cell] = m;
}

// exclusive scan of 256 LDS words by one wave, in place: lane l owns words 4 l .. 4 l + 3
__device__ inline void wave_scan_256(unsigned* a, int lane) {
  unsigned v[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) v[i] = a[4 * lane + i];
  const unsigned s = v[0] + v[1] + v[2] + v[3];
  unsigned incl = s;
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned t = (unsigned)__shfl_up((int)incl, o, 64);
    if (lane >= o) incl += t;
  }
  unsigned acc = incl - s;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    a[4 * lane + i] = acc;
    acc += v[i];
  }
}

__global__ void __launch_bounds__(kSelectThreads)
exchange_cells_select_kernel(const unsigned* __restrict__ score, CellGeometry g, uint8_t* __restrict__ wire,
                             int64_t* __restrict__ sent_cells) {
  extern __shared__ unsigned s_score[];                   // P words
  __shared__ unsigned s_hist[256], s_above[256], s_equal[256], s_prefix, s_remaining;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int P = g.cells, K = g.capacity;
  const long image = blockIdx.x;
  const unsigned* sc = score + image * P;
  for (int i = tid; i < P; i += kSelectThreads) s_score[i] = sc[i];
  if (tid < 256) {
    s_above[tid] = 0u;
    s_equal[tid] = 0u;
  }

  // T = the K-th largest score: digit by digit from the top, among the scores that share the digits found so far
  unsigned prefix = 0u, remaining = (unsigned)K;          // `remaining`-th largest of the scores matching `prefix`
  for (int d = 3; d >= 0; --d) {
    const int shift = 8 * d;
    const unsigned himask = d == 3 ? 0u : 0xffffffffu << (shift + 8);
    if (tid < 256) s_hist[tid] = 0u;
    __syncthreads();
    for (int i = tid; i < P; i += kSelectThreads) {
      const unsigned v = s_score[i];
      if ((v & himask) == prefix) atomicAdd(&s_hist[(v >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (wave == 0) {                                      // bins in descending order: lane l owns 255 - 4 l .. 252 - 4 l
      unsigned hb[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) hb[i] = s_hist[255 - (4 * lane + i)];
      const unsigned s = hb[0] + hb[1] + hb[2] + hb[3];
      unsigned incl = s;
      for (int o = 1; o < 64; o <<= 1) {
        const unsigned t = (unsigned)__shfl_up((int)incl, o, 64);
        if (lane >= o) incl += t;
      }
      unsigned acc = incl - s;
      if (acc < remaining && remaining <= incl) {         // exactly one lane: 1 <= remaining <= the matching scores
        bool found = false;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          if (!found && acc + hb[i] >= remaining) {
            s_prefix = prefix | ((unsigned)(255 - (4 * lane + i)) << shift);
            s_remaining = remaining - acc;
            found = true;
          }
          acc += hb[i];
        }
      }
    }
    __syncthreads();
    prefix = s_prefix;
    remaining = s_remaining;
  }
  const unsigned T = prefix;
  const unsigned need_equal = T == 0u ? 0u : remaining;   // score 0 is never sent: then only the cells above it go
  const unsigned count = (unsigned)K - remaining + need_equal;

  // every wave's counts of cells above and equal to T, round by round (entry = round * 16 + wave: ascending cell index)
  const int rounds = (P + kSelectThreads - 1) / kSelectThreads;
  for (int r = 0; r < rounds; ++r) {
    const int i = r * kSelectThreads + tid;
    const unsigned v = i < P ? s_score[i] : 0u;
    const unsigned long long ba = __ballot(v > T), be = __ballot(T != 0u && v == T);
    if (lane == 0) {
      s_above[r * 16 + wave] = (unsigned)__popcll(ba);
      s_equal[r * 16 + wave] = (unsigned)__popcll(be);
    }
  }
  __syncthreads();
  if (wave == 0) {
    wave_scan_256(s_above, lane);
    wave_scan_256(s_equal, lane);
  }
  __syncthreads();

  uint8_t* msg = wire + image * g.message_bytes;
  uint16_t* index = reinterpret_cast<uint16_t*>(msg + 16);
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int r = 0; r < rounds; ++r) {
    const int i = r * kSelectThreads + tid;
    const unsigned v = i < P ? s_score[i] : 0u;
    const bool above = v > T, equal = T != 0u && v == T;
    const unsigned long long ba = __ballot(above), be = __ballot(equal);
    const unsigned a_before = s_above[r * 16 + wave] + (unsigned)__popcll(ba & below);
    const unsigned e_before = s_equal[r * 16 + wave] + (unsigned)__popcll(be & below);
    if (above || (equal && e_before < need_equal)) index[a_before + min(e_before, need_equal)] = (uint16_t)i;
  }
  const int padded = (K + 7) / 8 * 8;                     // uint16 entries up to a multiple of 16 bytes
  for (int i = (int)count + tid; i < padded; i += kSelectThreads) index[i] = i < K ? (uint16_t)0xFFFFu : (uint16_t)0u;
  if (tid == 0) {
    *reinterpret_cast<u32x4*>(msg) = u32x4{count, 0u, 0u, 0u};
    if (sent_cells) sent_cells[image] += (int64_t)count;  // this lane alone owns the image's word
  }
}

template <int FMT>
__global__ void __launch_bounds__(256)
exchange_cells_pack_kernel(const float* __restrict__ feat, CellGeometry g, uint8_t* wire) {
  const long gw = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (gw >= g.body_waves * g.n_images) return;            // whole waves leave: the cross-lane steps below stay complete
  const int lane = threadIdx.x & 63;
  const long image = gw / g.body_waves, wi = gw - image * g.body_waves;
  const long q = wi * 64 + lane;
  const bool on = q < g.body_octets;
  uint8_t* msg = wire + image * g.message_bytes;
  u32x4 lo = {0u, 0u, 0u, 0u}, hi = {0u, 0u, 0u, 0u};
  if (on) {
    const long row = q / g.row_octets, oct = q - row * g.row_octets;
    const unsigned count = *reinterpret_cast<const unsigned*>(msg);
    if (row < (long)count) {                              // rows at and beyond count are +0.0
      const long p = reinterpret_cast<const uint16_t*>(msg + 16)[row];
      const u32x4* src = reinterpret_cast<const u32x4*>(feat + ((image * g.cells + p) * g.row_octets + oct) * 8);
      lo = src[0];
      hi = src[1];
    }
  }
  uint8_t* body = msg + g.body_offset;
  if constexpr (FMT == DN_EXCHANGE_F32) {
    if (!on) return;
    *reinterpret_cast<u32x4*>(body + q * 32) = lo;
    *reinterpret_cast<u32x4*>(body + q * 32 + 16) = hi;
  } else {
    const unsigned u[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    encode_octet<FMT>(u, on, q, wi, lane, body, g.payload_bytes);
  }
}

template <int FMT>
__global__ void __launch_bounds__(256)
exchange_cells_decode_kernel(const uint8_t* __restrict__ wire, CellGeometry g, float* __restrict__ feat) {
  const long gw = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (gw >= g.map_waves * g.n_images) return;
  const int lane = threadIdx.x & 63;
  const long image = gw / g.map_waves, wi = gw - image * g.map_waves;
  const long q = wi * 64 + lane;
  if (q >= g.map_octets) return;
  const unsigned cell = (unsigned)(q / g.row_octets);
  const long oct = q - (long)cell * g.row_octets;
  const uint8_t* msg = wire + image * g.message_bytes;
  const uint16_t* index = reinterpret_cast<const uint16_t*>(msg + 16);
  const unsigned count = min(*reinterpret_cast<const unsigned*>(msg), (unsigned)g.capacity);
  unsigned first = 0u, last = count;                      // the first row whose index is >= cell, inside [0, count]
  while (first < last) {
    const unsigned mid = (first + last) >> 1;
    if (index[mid] < cell) first = mid + 1; else last = mid;
  }
  float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (first < count && index[first] == cell) {            // (an index >= P matches no cell: skipped)
    const uint8_t* body = msg + g.body_offset;
    const long bq = (long)first * g.row_octets + oct;
    if constexpr (FMT == DN_EXCHANGE_F32) {
      const f32x4v a = *reinterpret_cast<const f32x4v*>(body + bq * 32), b = *reinterpret_cast<const f32x4v*>(body + bq * 32 + 16);
      v[0] = a[0]; v[1] = a[1]; v[2] = a[2]; v[3] = a[3];
      v[4] = b[0]; v[5] = b[1]; v[6] = b[2]; v[7] = b[3];
    } else {
      decode_octet<FMT>(body, g.payload_bytes, bq, v);
    }
  }
  float* dst = feat + (image * g.map_octets + q) * 8;
  *reinterpret_cast<f32x4v*>(dst) = f32x4v{v[0], v[1], v[2], v[3]};
  *reinterpret_cast<f32x4v*>(dst + 4) = f32x4v{v[4], v[5], v[6], v[7]};
}

// one image's message bytes, or -1 (refused); *body_offset, *payload: where the body begins, its bytes before the scales
long cells_message_bytes_of(int format, int h, int w, int c, int cells, long* body_offset, long* payload) {
  if (h <= 0 || w <= 0 || (long)h * w > DN_EXCHANGE_CELLS_MAX || cells < 1 || cells > h * w) return -1;
  const long body = exchange_message_bytes_of(format, 1, cells, c, payload);
  if (body < 0) return -1;
  const long offset = 16 + (2L * cells + 15) / 16 * 16;
  if (body_offset) *body_offset = offset;
  return offset + body;
}

int cell_geometry_of(const char* who, const void* a, const void* b, int n_images, int h, int w, int c, int format, int cells,
                     CellGeometry* g) {
  DN_REQUIRE(a && b, "%s: null pointer", who);
  DN_REQUIRE(format == DN_EXCHANGE_F32 || format == DN_EXCHANGE_F16 || format == DN_EXCHANGE_MXFP8 ||
             format == DN_EXCHANGE_MXFP4, "%s: format %d is none of DN_EXCHANGE_F32 0, DN_EXCHANGE_F16 1, DN_EXCHANGE_MXFP8 2, "
             "DN_EXCHANGE_MXFP4 3", who, format);
  DN_REQUIRE(n_images > 0 && h > 0 && w > 0, "%s: empty problem", who);
  DN_REQUIRE(c > 0 && c % 32 == 0, "%s: channel count %d must be a multiple of 32 (one scale per 32 channels of a pixel)",
             who, c);
  DN_REQUIRE((long)h * w <= DN_EXCHANGE_CELLS_MAX, "%s: a %d x %d map has %ld cells, at most %d fit (one image's scores "
             "live in LDS)", who, h, w, (long)h * w, DN_EXCHANGE_CELLS_MAX);
  DN_REQUIRE(cells >= 1 && cells <= h * w, "%s: cells = %d must be in [1, %d] (the cells of a %d x %d map)", who, cells,
             h * w, h, w);
  DN_REQUIRE((long)h * w * c < ((long)1 << 31), "%s: a %d x %d x %d map is past 2^31 values", who, h, w, c);
  g->message_bytes = cells_message_bytes_of(format, h, w, c, cells, &g->body_offset, &g->payload_bytes);
  DN_REQUIRE(g->message_bytes > 0, "%s: %d cells of %d channels are past 2^31 values", who, cells, c);
  DN_REQUIRE((((size_t)a | (size_t)b) & 15) == 0, "%s: feat and wire must be 16-byte aligned", who);
  g->cells = h * w;
  g->capacity = cells;
  g->row_octets = c / 8;
  int group = 4;                                          // c % 32 == 0: at least 4 octets per cell
  while (group * 2 <= 64 && group * 2 <= g->row_octets) group *= 2;
  g->group = group;
  g->n_images = n_images;
  g->total_cells = (long)n_images * g->cells;
  g->body_octets = (long)cells * g->row_octets;
  g->body_waves = (g->body_octets + 63) / 64;
  g->map_octets = (long)g->cells * g->row_octets;
  g->map_waves = (g->map_octets + 63) / 64;
  DN_REQUIRE((g->map_waves * n_images + 3) / 4 <= 0x7fffffffL && g->total_cells <= 0x7fffffffL,
             "%s: %d images of %d x %d x %d are past the grid limit", who, n_images, h, w, c);
  return DN_OK;
}

long cells_workspace_bytes_of(int n_images, int h, int w) {
  if (n_images <= 0 || h <= 0 || w <= 0 || (long)h * w > DN_EXCHANGE_CELLS_MAX) return -1;
  return (long)dn::align256((size_t)n_images * h * w * sizeof(unsigned));
}

}  // namespace

extern "C" long dn_exchange_cells_message_bytes(int format, int h, int w, int c, int cells) {
  const long bytes = cells_message_bytes_of(format, h, w, c, cells, nullptr, nullptr);
  if (bytes < 0)
    return dn::fail(DN_ERR_ARG, "exchange cells message bytes: format %d, map %d x %d x %d, cells %d (formats 0..3, c a "
                    "multiple of 32, at most %d cells in the map, cells in [1, h * w])", format, h, w, c, cells,
                    DN_EXCHANGE_CELLS_MAX);
  return bytes;
}

extern "C" long dn_exchange_cells_workspace_bytes(int n_images, int h, int w) {
  const long bytes = cells_workspace_bytes_of(n_images, h, w);
  if (bytes < 0)
    return dn::fail(DN_ERR_ARG, "exchange cells workspace bytes: %d images of %d x %d (at least one image, at most %d cells "
                    "in the map)", n_images, h, w, DN_EXCHANGE_CELLS_MAX);
  return bytes;
}

#define DN_EXCHANGE_CELLS_BY_FORMAT(format, LAUNCH)                        \
  do {                                                                     \
    if ((format) == DN_EXCHANGE_F32) { LAUNCH(DN_EXCHANGE_F32); }          \
    else if ((format) == DN_EXCHANGE_F16) { LAUNCH(DN_EXCHANGE_F16); }     \
    else if ((format) == DN_EXCHANGE_MXFP8) { LAUNCH(DN_EXCHANGE_MXFP8); } \
    else { LAUNCH(DN_EXCHANGE_MXFP4); }                                    \
  } while (0)

extern "C" int dn_exchange_encode_cells(const float* feat, int n_images, int h, int w, int c, int format, int cells,
                                        void* workspace, size_t workspace_bytes, uint8_t* wire, int64_t* sent_cells,
                                        void* stream) {
  const char* who = "exchange encode cells";
  CellGeometry g;
  if (int rc = cell_geometry_of(who, feat, wire, n_images, h, w, c, format, cells, &g)) return rc;
  DN_REQUIRE(workspace, "%s: null workspace", who);
  DN_REQUIRE(((size_t)workspace & 15) == 0, "%s: the workspace must be 16-byte aligned", who);
  DN_REQUIRE(((size_t)sent_cells & 7) == 0, "%s: sent_cells must be 8-byte aligned", who);
  const long need = cells_workspace_bytes_of(n_images, h, w);
  DN_REQUIRE(workspace_bytes >= (size_t)need, "%s: the workspace holds %zu bytes, %ld are needed "
             "(dn_exchange_cells_workspace_bytes)", who, workspace_bytes, need);
  static dn::PerDeviceFlag lds_flag;
  if (int rc = dn::reserve_dynamic_lds((const void*)exchange_cells_select_kernel, lds_flag,
                                       DN_EXCHANGE_CELLS_MAX * sizeof(unsigned), who))
    return rc;
  hipStream_t s = (hipStream_t)stream;
  unsigned* score = static_cast<unsigned*>(workspace);
  const long cells_per_group = 4 * (64 / g.group);        // cells of one score workgroup
  hipLaunchKernelGGL(exchange_cells_score_kernel, dim3((unsigned)((g.total_cells + cells_per_group - 1) / cells_per_group)),
                     dim3(256), 0, s, feat, g, score);
  if (int rc = dn::check_launch("exchange_cells_score_kernel")) return rc;
  hipLaunchKernelGGL(exchange_cells_select_kernel, dim3((unsigned)n_images), dim3(kSelectThreads),
                     (size_t)g.cells * sizeof(unsigned), s, score, g, wire, sent_cells);
  if (int rc = dn::check_launch("exchange_cells_select_kernel")) return rc;
  const dim3 grid((unsigned)((g.body_waves * n_images + 3) / 4));
#define DN_LAUNCH(F) hipLaunchKernelGGL(exchange_cells_pack_kernel<F>, grid, dim3(256), 0, s, feat, g, wire)
  DN_EXCHANGE_CELLS_BY_FORMAT(format, DN_LAUNCH);
#undef DN_LAUNCH
  return dn::check_launch("exchange_cells_pack_kernel");
}

extern "C" int dn_exchange_decode_cells(const uint8_t* wire, int n_images, int h, int w, int c, int format, int cells,
                                        float* feat, void* stream) {
  CellGeometry g;
  if (int rc = cell_geometry_of("exchange decode cells", wire, feat, n_images, h, w, c, format, cells, &g)) return rc;
  const dim3 grid((unsigned)((g.map_waves * n_images + 3) / 4));
#define DN_LAUNCH(F) hipLaunchKernelGGL(exchange_cells_decode_kernel<F>, grid, dim3(256), 0, (hipStream_t)stream, wire, g, feat)
  DN_EXCHANGE_CELLS_BY_FORMAT(format, DN_LAUNCH);
#undef DN_LAUNCH
  return dn::check_launch("exchange_cells_decode_kernel");
}
