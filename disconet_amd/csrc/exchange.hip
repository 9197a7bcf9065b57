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
// The element formats, the integer conversions and the per-octet encode / decode bodies are exchange_device.h, shared
// with the selective exchange of exchange_cells.hip.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>

#include "dn_internal.h"
#include "exchange_device.h"

namespace {

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
  encode_octet<FMT>(u, on, q, wi, lane, wire + image * g.message_bytes, g.payload_bytes);
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
  float v[8];
  decode_octet<FMT>(wire + image * g.message_bytes, g.payload_bytes, q, v);
  float* dst = feat + (image * g.octets + q) * 8;
  using f32x4v = __attribute__((ext_vector_type(4))) float;
  *reinterpret_cast<f32x4v*>(dst) = f32x4v{v[0], v[1], v[2], v[3]};
  *reinterpret_cast<f32x4v*>(dst + 4) = f32x4v{v[4], v[5], v[6], v[7]};
}

int geometry_of(const char* who, const void* a, const void* b, int n_images, int h, int w, int c, int format, Geometry* g) {
  DN_REQUIRE(a && b, "%s: null pointer", who);
  DN_REQUIRE(format == DN_EXCHANGE_F16 || format == DN_EXCHANGE_MXFP8 || format == DN_EXCHANGE_MXFP4,
             "%s: format %d is none of DN_EXCHANGE_F16 1, DN_EXCHANGE_MXFP8 2, DN_EXCHANGE_MXFP4 3 (DN_EXCHANGE_F32 0 is the "
             "identity: there is nothing to launch)", who, format);
  DN_REQUIRE(n_images > 0 && h > 0 && w > 0, "%s: empty problem", who);
  DN_REQUIRE(c > 0 && c % 32 == 0, "%s: channel count %d must be a multiple of 32 (one scale per 32 channels of a pixel)",
             who, c);
  g->message_bytes = exchange_message_bytes_of(format, h, w, c, &g->payload_bytes);
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
  const long bytes = exchange_message_bytes_of(format, h, w, c, nullptr);
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
