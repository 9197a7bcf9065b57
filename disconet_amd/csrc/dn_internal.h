// Shared helpers of libdisconet_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdio>

#include "disconet_hip.h"

namespace dn {

char* err_buf();   // thread-local, 512 bytes

constexpr int kCUs = 256;   // MI355X: what the conv launchers size their persistent grids by

inline int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(err_buf(), 512, fmt, ap);
  va_end(ap);
  return code;
}

// Zero `bytes` bytes at `ptr` on `stream` with a kernel launch.  NOT hipMemsetAsync: a memset captured into a
// hipGraph was measured to write a garbage 16-byte pattern from the second replay on (tools/hazard/ptr_audit.py,
// DESIGN.md 3.6) -- a kernel node carries its arguments by value and replays exactly.
hipError_t zero_fill(void* ptr, size_t bytes, hipStream_t stream);

// Launch-time caches (kernel attributes) are per DEVICE: a process that drives several GPUs must set the
// dynamic-LDS attribute on each.  `flags` is a function-local static of the caller.
struct PerDeviceFlag {
  bool done[64] = {};
  bool& here() {
    int dev = 0;
    (void)hipGetDevice(&dev);
    return done[dev & 63];
  }
};

// The kernel's static LDS in bytes, read once per device; with dynamic_most > 0 the same first call reserves that much
// dynamic LDS for it.  `flag` and `cache` (64 words) are function-local statics of the caller.  -1: the attributes cannot
// be read, -2: the dynamic LDS cannot be reserved.
inline int static_lds_of(const void* kernel, PerDeviceFlag& flag, int* cache, int dynamic_most) {
  int dev = 0;
  (void)hipGetDevice(&dev);
  bool& ready = flag.done[dev & 63];
  if (!ready) {
    hipFuncAttributes attr;
    if (hipFuncGetAttributes(&attr, kernel) != hipSuccess) return -1;
    if (dynamic_most > 0 &&
        hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, dynamic_most) != hipSuccess)
      return -2;
    cache[dev & 63] = (int)attr.sharedSizeBytes;
    ready = true;
  }
  return cache[dev & 63];
}

// Reserve `bytes` of dynamic LDS for `kernel`, once per device.  `flag` is a function-local static of the caller.
inline int reserve_dynamic_lds(const void* kernel, PerDeviceFlag& flag, size_t bytes, const char* who) {
  bool& ready = flag.here();
  if (!ready) {
    hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess)
      return fail(DN_ERR_LAUNCH, "%s: hipFuncSetAttribute(%zu B LDS): %s", who, bytes, hipGetErrorString(e));
    ready = true;
  }
  return DN_OK;
}

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// Carves a caller-owned workspace into arrays: take(bytes) returns the current offset and advances to the next 256-byte
// boundary; `at` is then the bytes needed so far.
struct Carver {
  size_t at = 0;
  size_t take(size_t bytes) {
    const size_t o = at;
    at = align256(at + bytes);
    return o;
  }
};

inline int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(DN_ERR_LAUNCH, "%s: %s", what, hipGetErrorString(e));
  return DN_OK;
}

// quad-merged up-conv (conv_spq.hip), reached through dn_spconv2d / dn_spconv_pack_weights (conv_sp.hip)
size_t spq_packed_blocks(int c0g, int nchunks);
int spq_pack_weights(const float* weight_oihw, void* packed, int c_out, int c_in, int c0g, int cout_pad, int nchunks,
                     float wmul, hipStream_t stream);
int spq_conv(const dn_conv_desc* d, const void* src0, const void* src1, const void* packed, size_t packed_bytes,
             const float* scale, const float* shift, void* out, int cout_pad, int bn, hipStream_t stream,
             int kslices = 1, float* workspace = nullptr, size_t workspace_bytes = 0, float* out_nhwc = nullptr,
             int ld_nhwc = 0);

// the score launch of dn_agent_fuse (agent_fuse.hip), an epilogue of the attention MLP's kernel (fuse_mlp.hip)
int fuse_mlp_agent_scores(const float* feat, const float* warped, int warped_fm, const int32_t* num_agent,
                          const dn_fuse_mlp_params* p, const float* w5, int batch, int agents, int hw, int c, int only_v2i,
                          int ego_first, int ego_count, float* partials, hipStream_t stream);

// per-translation-unit words of the split-f16 range flags (sp_device.h); dn_sp_range_flags() ORs them
void range_collect_conv_sp(unsigned* dst, bool reset, hipStream_t stream);
void range_collect_conv_spq(unsigned* dst, bool reset, hipStream_t stream);
void range_collect_fuse_mlp(unsigned* dst, bool reset, hipStream_t stream);
void range_collect_conv_wgrad(unsigned* dst, bool reset, hipStream_t stream);
unsigned* sp_range_word();   // conv_sp.hip's word on the current device (nullptr on error)

// The form of the last SP conv launch of the process (dn_spconv_last_form: tools and tests), written by the three
// launchers themselves -- launch<>() of conv_sp.hip, launch_spq<>() of conv_spq.hip, dn_spconv2d_pre_pair -- so that
// it names the kernel that ran and not a copy of the dispatch.  Host side only; process-wide, not thread-safe.
struct SpLastForm {
  int family;                     // 0 = conv_sp_kernel, 1 = conv_spq_kernel, 2 = conv_pre_pair_kernel, -1 = none yet
  int ks, stride, th, tw, bn, tg, ca, post, bstat, upm, ahi, ksl, nb, deep;
  int grid, total_items;          // workgroups and work items of the (main) launch
  int n_whole, n_split;           // K-sliced launches: tiles run whole / split into slices (else total_items, 0)
  int fixup_grid;                 // workgroups of the K-sliced fix-up launch (0: none)
};
extern SpLastForm g_sp_last_form;
extern int g_spq_last_resident;   // family 1 only: the launch ran conv_spq.hip's resident-weights form (dn_spconv_last_resident)

}  // namespace dn

#define DN_REQUIRE(cond, ...) \
  do { if (!(cond)) return dn::fail(DN_ERR_ARG, __VA_ARGS__); } while (0)

// The arguments that the evaluation steps behind the tracker share (dn_mot_step, dn_idf_step, dn_hota_step): the reported
// tracks, the ground truth, the state, M, G and scale, under the names of include/disconet_hip.h.
#define DN_REQUIRE_EVAL_STEP(who, max_m, max_g)                                                                \
  DN_REQUIRE(rect, who ": null rect");                                                                         \
  DN_REQUIRE(id, who ": null id");                                                                             \
  DN_REQUIRE(count, who ": null count");                                                                       \
  DN_REQUIRE(gt_boxes, who ": null gt_boxes");                                                                 \
  DN_REQUIRE(gt_ids, who ": null gt_ids");                                                                     \
  DN_REQUIRE(gt_count, who ": null gt_count");                                                                 \
  DN_REQUIRE(state, who ": null state");                                                                       \
  DN_REQUIRE(m >= 1 && m <= (max_m), who ": M = %d track rows, must be in [1, %d]", m, (max_m));              \
  DN_REQUIRE(g >= 1 && g <= (max_g), who ": G = %d ground-truth rows, must be in [1, %d]", g, (max_g));       \
  DN_REQUIRE(std::isfinite(scale) && scale > 0, who ": scale = %g, must be finite and > 0", scale)
