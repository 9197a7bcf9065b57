#include "dn_internal.h"

namespace dn {
char* err_buf() {
  static thread_local char buf[512] = {0};
  return buf;
}
namespace {
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
// head/tail bytes one at a time, the 16-byte aligned middle as 128-bit stores (grid-stride)
__global__ void __launch_bounds__(256) zero_fill_kernel(unsigned char* p, size_t head, size_t vecs, size_t tail) {
  const size_t tid = blockIdx.x * (size_t)blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
  if (tid < head) p[tid] = 0;
  u32x4* v = reinterpret_cast<u32x4*>(p + head);
  for (size_t i = tid; i < vecs; i += stride) v[i] = u32x4{0u, 0u, 0u, 0u};
  if (tid < tail) p[head + 16 * vecs + tid] = 0;
}
}  // namespace

hipError_t zero_fill(void* ptr, size_t bytes, hipStream_t stream) {
  if (bytes == 0) return hipSuccess;
  unsigned char* p = static_cast<unsigned char*>(ptr);
  size_t head = (16 - (reinterpret_cast<size_t>(p) & 15)) & 15;
  if (head > bytes) head = bytes;
  const size_t vecs = (bytes - head) / 16, tail = bytes - head - 16 * vecs;
  const size_t want = (vecs + 255) / 256;
  const int blocks = (int)(want < 1 ? 1 : (want > 8192 ? 8192 : want));
  hipLaunchKernelGGL(zero_fill_kernel, dim3(blocks), dim3(256), 0, stream, p, head, vecs, tail);
  return hipGetLastError();
}
}  // namespace dn

extern "C" int dn_version(void) { return 158; }  // 0.1.3: round-5 kernels (profiles carry this number; 131: dn_conv_wgrad_sp; 132: round 6 -- Gray MFMA order, fp32 rows from the tap-merged kernel, fused bias gradients; 133: dn_spconv_pack_weights_multi, lane-parallel warp gathers; 134: dn_conv_wgrad_sp_z, dz = NULL in the BatchNorm backward; 135: dn_detect; 136: dn_ap_match, dn_ap_reset; 137: the BatchNorm training passes take dn_bn_bwd_desc / dn_bn_bwd_out and optional outputs -- 8 entry points for 14; 138: dn_assign_targets; 139: dn_voxelize_views; 140: the focal loss takes log q from the logit difference (log-softmax form) -- loss and class gradient of anchors with a wrong-side logit gap above 69 change; dn_adam_step takes its hyper-parameters as doubles; the x2 bilinear upsample kernels take the source coordinate as an exact rational; 141: dn_spconv_last_form (host side only: every kernel as in 140); 142: dn_conv_force_config, dn_conv_last_form (host side only: every kernel as in 140); 143: dn_mot_state_bytes, dn_mot_reset, dn_mot_step (a new kernel; every other kernel as in 140); 144: dn_idf_state_bytes, dn_idf_reset, dn_idf_step, dn_idf_finish (two new kernels; every other kernel as in 140); 145: dn_hota_state_bytes, dn_hota_work_bytes, dn_hota_reset, dn_hota_step, dn_hota_finish (three new kernels; every other kernel as in 140); 146: dn_seg_confusion (one new kernel; every other kernel as in 140); 147: dn_fuse_reduce, dn_fuse_reduce_lists, dn_fuse_reduce_lists_backward (fuse_reduce.hip: four new kernels; every other kernel as in 140); 148: dn_late_fuse_workspace_bytes, dn_late_fuse (detect.hip: one new kernel in front of dn_detect's pair-mask and wave-walk kernels; every other kernel as in 140); 149: dn_agent_fuse, dn_agent_fuse_workspace_bytes, dn_agent_combine_lists / _backward (agent_fuse.hip, a score epilogue of fuse_mlp.hip's kernel as new instantiations; every shipped instantiation as in 148); 150: dn_det_loss_corner (train_ops.hip: two new kernels; the six decode lines of decode_device.h in a helper that dn_decode_boxes, dn_detect and the new kernels inline; every shipped kernel as in 149); 151: dn_render_bev (render.hip: one new kernel; every other kernel as in 150); 152: dn_lidar_scan (lidar.hip: two new kernels; every other kernel as in 150); 153: dn_gt_strata, dn_ap_match_strata_workspace_bytes, dn_ap_match_strata, dn_ap_strata_reset (ap_match.hip: four new kernels; ap_tp_kernel takes its tp bits and its record offset from two device functions that the stratified kernel shares -- the same words; every other kernel as in 150); 154: dn_lidar_world_step (lidar_seq.hip: one new kernel), dn_lidar_scan_ids (lidar.hip: lidar_visible_kernel takes a nullable gt_ids, null from dn_lidar_scan -- the same bytes; every other kernel as in 153); 155: dn_exchange_message_bytes, dn_exchange_encode, dn_exchange_decode (exchange.hip: two new kernels; every other kernel as in 154); 156: dn_exchange_cells_message_bytes, dn_exchange_cells_workspace_bytes, dn_exchange_encode_cells, dn_exchange_decode_cells (exchange_cells.hip: four new kernels; exchange.hip's two take their octet bodies from exchange_device.h -- the same bytes; every other kernel as in 155); 157: dn_bn_train_last_form (host side only); the batch statistics square z in double (bn_stats_kernel, bn_stats_v4_kernel: var may differ from 156's, mean is the same bits; every other kernel as in 156); 158: the four dn_scatter_dense forms skip rows outside [offsets[0], offsets[n_images]) (157 wrote them into the first / the last image; the same bytes for a list that its offsets cover); the voxel entry points name the argument they refuse (every other kernel as in 157))

// The hash of every source / header / flag this library was built from (csrc/build.py :: tree_hash), behind a marker
// that build.py also finds in the file without loading it.  _lib.load() refuses a library whose id is not the tree's.
#ifndef DN_BUILD_ID
#error "build through disconet_amd/csrc/build.py (it passes -DDN_BUILD_ID)"
#endif
static const char dn_build_id_marker[] = "dn-build-id:" DN_BUILD_ID;
extern "C" const char* dn_build_id(void) { return dn_build_id_marker + 12; }

// Stream-ordered form: every split-f16 translation unit ORs its sticky word into *dst_device (which the caller
// zeroed) behind whatever the stream holds; kernel launches only, so it is legal inside a capture.
extern "C" int dn_sp_range_flags_async(unsigned* dst_device, int reset, void* stream) {
  DN_REQUIRE(dst_device != nullptr, "sp_range_flags_async: null destination");
  hipStream_t s = (hipStream_t)stream;
  // bit 1 of `reset`: zero *dst first, with a kernel -- a captured step cannot rely on a memset node
  if ((reset & 2) && dn::zero_fill(dst_device, sizeof(unsigned), s) != hipSuccess)
    return dn::fail(DN_ERR_LAUNCH, "sp_range_flags_async: zero fill of the destination failed");
  const bool clear = (reset & 1) != 0;
  dn::range_collect_conv_sp(dst_device, clear, s);
  dn::range_collect_conv_spq(dst_device, clear, s);
  dn::range_collect_fuse_mlp(dst_device, clear, s);
  dn::range_collect_conv_wgrad(dst_device, clear, s);
  return dn::check_launch("sp_range_collect_kernel");
}

// Blocking form: waits for the device (every stream, blocking or not), then reads through the same collectors.
extern "C" unsigned dn_sp_range_flags(int reset) {
  unsigned* d = nullptr;
  unsigned v = 0;
  if (hipDeviceSynchronize() != hipSuccess || hipMalloc((void**)&d, sizeof v) != hipSuccess) return 0x80000000u;
  bool ok = hipMemcpy(d, &v, sizeof v, hipMemcpyHostToDevice) == hipSuccess &&
            dn_sp_range_flags_async(d, reset ? 1 : 0, nullptr) == DN_OK &&
            hipMemcpy(&v, d, sizeof v, hipMemcpyDeviceToHost) == hipSuccess;
  (void)hipFree(d);
  return ok ? v : 0x80000000u;
}

extern "C" const char* dn_last_error(void) { return dn::err_buf(); }
