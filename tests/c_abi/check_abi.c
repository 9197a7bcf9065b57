/* A C host of libdisconet_hip.so with no Python and no torch: the drop-in boundary
 * is the C ABI of include/disconet_hip.h.
 *   gcc -std=c11 -D__HIP_PLATFORM_AMD__ -I include -I /opt/rocm/include tests/c_abi/check_abi.c \
 *       -L disconet_amd -ldisconet_hip -L /opt/rocm/lib -lamdhip64 -lm -Wl,-rpath,... -o check_abi
 *   ./check_abi          error behaviour only (no GPU needed)
 *   ./check_abi --gpu    + a 3x3 conv (both math modes), the voxelizer, the split-planar engine (plain and over an
 *                        upsampled + concatenated source), the hi-only occupancy form, the range flags, the pose warp
 *                        and both forms of the fusion launch against C loops
 */
#include <hip/hip_runtime_api.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "disconet_hip.h"
#include "disconet_train.h"

#define CHECK(cond, ...) do { if (!(cond)) { printf("FAIL line %d: ", __LINE__); printf(__VA_ARGS__); printf("\n"); return 1; } } while (0)
#define HIP(x) CHECK((x) == hipSuccess, "%s", #x)

static float frand(unsigned* s) { *s = *s * 1664525u + 1013904223u; return ((*s >> 8) / 8388608.0f) - 1.0f; }

static int errors_only(void) {
  CHECK(dn_version() >= 137, "version");
  CHECK(dn_build_id() != NULL && strlen(dn_build_id()) == 16, "build id: %s", dn_build_id() ? dn_build_id() : "(null)");
  dn_conv_desc d;
  memset(&d, 0, sizeof d);
  d.n_images = 1; d.h_in = 8; d.w_in = 8; d.c0 = 32; d.c_out = 32; d.ksize = 7; d.stride = 1;
  d.ld0 = 32; d.ldo = 32;
  CHECK(dn_conv_packed_weight_floats(&d) == 0, "bad ksize must give 0 floats");
  CHECK(strstr(dn_last_error(), "ksize") != NULL, "message: %s", dn_last_error());
  CHECK(dn_conv2d(&d, NULL, NULL, NULL, NULL, NULL, NULL, NULL) == DN_ERR_ARG, "conv arg error");
  d.ksize = 3; d.math = 5;
  CHECK(dn_conv2d(&d, NULL, NULL, NULL, NULL, NULL, NULL, NULL) == DN_ERR_ARG, "bad math mode");
  CHECK(dn_decode_boxes(NULL, NULL, NULL, 1, 10, NULL, NULL, NULL) == DN_ERR_ARG, "decode null");
  int dims[3] = {256, 256, 13};
  CHECK(dn_voxel_compact_workspace(dims) == ((256 * 256 * 13 + 1023) / 1024) * sizeof(int), "workspace");
  CHECK(dn_post1x1_packed_floats() == 64 * 64, "post1x1 size");
  /* the fp32-NHWC engine's tools hooks: ids -1 .. 8, an 11-int record */
  {
    int form[11];
    CHECK(dn_conv_force_config(9) == DN_ERR_ARG && dn_conv_force_config(-2) == DN_ERR_ARG, "force config: bad id accepted");
    CHECK(dn_conv_force_config(3) == DN_OK && dn_conv_force_config(-1) == DN_OK, "force config: %s", dn_last_error());
    CHECK(dn_conv_last_form(NULL, 11) == DN_ERR_ARG, "last form: null accepted");
    CHECK(dn_conv_last_form(form, 11) == 11, "last form: 11 fields");
  }
  /* training header: plain C as well, same error convention */
  d.math = 0;
  CHECK(dn_conv_wgrad_workspace(&d) > 0, "wgrad workspace");
  CHECK(dn_conv_wgrad(&d, NULL, NULL, NULL, NULL, NULL, 0, 0, NULL) == DN_ERR_ARG, "wgrad null");
  /* the weight gradient's tools hooks: a 12-int plan (8 x 8 map, 32 -> 32: one 8 x 16 tile, one slice), a 10-int record */
  {
    int plan[12], form[10];
    CHECK(dn_conv_wgrad_plan(&d, 0, NULL, 12) == DN_ERR_ARG, "wgrad plan: null accepted");
    CHECK(dn_conv_wgrad_plan(&d, 0, plan, 12) == 12 && plan[0] == 32 && plan[1] == 8 && plan[2] == 16 && plan[7] == 1 &&
          plan[10] == 1 && plan[11] == 9, "wgrad plan: %d %d %d %d %d %d", plan[0], plan[1], plan[2], plan[7], plan[10], plan[11]);
    CHECK(dn_conv_wgrad_plan(&d, 1, plan, 12) == 12 && plan[0] == 32 && plan[1] == 8, "wgrad plan, split-f16");
    CHECK(dn_conv_wgrad_last_form(NULL, 10) == DN_ERR_ARG, "wgrad last form: null accepted");
    CHECK(dn_conv_wgrad_last_form(form, 10) == 10, "wgrad last form: 10 fields");
    CHECK(dn_bn_train_last_form(DN_BN_PASS_APPLY, NULL, 8) == DN_ERR_ARG && dn_bn_train_last_form(DN_BN_PASSES, form, 8) == DN_ERR_ARG, "bn last form: null / unknown pass accepted");
    CHECK(dn_bn_train_last_form(DN_BN_PASS_APPLY, form, 8) == 8 && form[0] == -1, "bn last form: 8 fields, no call yet");
  }
  /* the split-f16 weight gradient: 32 -> 32 channels takes the 32-channel block form; a 13-channel source has none */
  CHECK(dn_conv_wgrad_sp_supported(&d) == 32 && dn_conv_wgrad_sp_workspace(&d) > 0, "wgrad_sp supported");
  CHECK(dn_conv_wgrad_sp(&d, NULL, NULL, NULL, NULL, NULL, 0, 0, 256.f, 16.f, NULL) == DN_ERR_ARG, "wgrad_sp null");
  d.c0 = 13; d.ld0 = 13;     /* the voxel grid: one source of any width takes the 32-channel blocks too (dword loads) */
  CHECK(dn_conv_wgrad_sp_supported(&d) == 32, "wgrad_sp: 13 channels");
  d.stride = 2;
  CHECK(dn_conv_wgrad_sp_supported(&d) == 0 && dn_conv_wgrad_sp_workspace(&d) == 0, "wgrad_sp: stride 2");
  d.stride = 1; d.c0 = 32; d.ld0 = 32;
  CHECK(dn_adam_step(NULL, NULL, NULL, NULL, 10, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, NULL) == DN_ERR_ARG,
        "adam null");
  CHECK(dn_bn_train_stats(NULL, 1, 10, 600, 600, NULL, 0, NULL, NULL, NULL, NULL, 0.f, NULL) == DN_ERR_ARG, "bn null");
  /* round 5: two-phase BatchNorm reductions (agent-parallel training) and the K-slice query */
  CHECK(dn_bn_train_stats_partial(NULL, 1, 10, 8, 8, NULL, 0, NULL) == DN_ERR_ARG, "bn stats partial null");
  CHECK(dn_bn_train_stats_finish(NULL, 1, 10, 8, NULL, NULL, NULL) == DN_ERR_ARG, "bn stats finish null");
  {
    /* the optional outputs of the BatchNorm passes: each condition sits on the pointer that selects the form */
    float* const p = (float*)16;      /* never dereferenced: every call below is refused on the host */
    CHECK(dn_bn_train_stats(NULL, 1, 16, 16, 16, NULL, 0, NULL, NULL, NULL, NULL, 0.1f, NULL) == DN_ERR_ARG, "bn stats (+ running) null");
    CHECK(dn_bn_train_stats(p, 1, 16, 16, 16, (double*)p, 1 << 20, p, p, p, NULL, 0.1f, NULL) == DN_ERR_ARG && strstr(dn_last_error(), "running"),
          "bn stats: running_mean without running_var: %s", dn_last_error());
    CHECK(dn_bn_bias_workspace_bytes(0, 32) == 0 && dn_bn_bias_workspace_bytes(1024, 32) == 8u * 32u * (1 + 32), "bn bias workspace");
    CHECK(dn_bn_train_apply(NULL, NULL, NULL, NULL, NULL, 1e-5f, 1, 1, 16, 16, 16, NULL, NULL, NULL, 16, NULL) == DN_ERR_ARG,
          "bn apply (mask + SP) null");
    CHECK(dn_bn_train_apply(p, p, p, p, p, 1e-5f, 1, 1, 16, 24, 24, p, (unsigned char*)p, p, 16, NULL) == DN_ERR_ARG &&
              strstr(dn_last_error(), "c % 16"), "bn apply (mask + SP): c %% 16: %s", dn_last_error());
    CHECK(dn_bn_train_apply(p, p, p, p, p, 1e-5f, 1, 1, 16, 16, 16, p, NULL, p, 16, NULL) == DN_ERR_ARG, "bn apply: y_sp without relu_mask");
    CHECK(dn_bn_train_stats_finish((const double*)16, 1, 0, 8, (float*)16, (float*)16, NULL) == DN_ERR_ARG, "bn stats finish: zero rows");
    dn_bn_bwd_desc b;
    dn_bn_bwd_out o;
    memset(&b, 0, sizeof b);
    memset(&o, 0, sizeof o);
    b.ld_a = 8; b.n_groups = 1; b.h = 4; b.w = 4; b.images_per_group = 1; b.c = 8; b.eps = 1e-5f;
    CHECK(dn_bn_train_backward_partial(NULL, NULL, 0, NULL, NULL, 0, NULL) == DN_ERR_ARG, "bn bwd partial: no descriptor");
    CHECK(dn_bn_train_backward_partial(&b, NULL, 0, NULL, NULL, 0, NULL) == DN_ERR_ARG, "bn bwd partial null");
    CHECK(dn_bn_train_backward_finish(&b, NULL, 16, &o, NULL) == DN_ERR_ARG, "bn bwd finish null");
    CHECK(dn_bn_train_backward(&b, NULL, 0, &o, NULL, NULL, 0, NULL) == DN_ERR_ARG, "bn bwd null");
    b.dy_a = b.z = b.mean = b.var = b.gamma = p;
    CHECK(dn_bn_train_backward_finish(&b, (const double*)p, 16, NULL, NULL) == DN_ERR_ARG, "bn bwd finish: no outputs");
    CHECK(dn_bn_train_backward_finish(&b, (const double*)p, 16, &o, NULL) == DN_ERR_ARG, "bn bwd finish: neither dz nor dz_sp");
    b.ld_a = 16; b.c = 16;
    o.dz = p; o.dbias = p;      /* the fused bias gradient without its workspace */
    CHECK(dn_bn_train_backward_finish(&b, (const double*)p, 16, &o, NULL) == DN_ERR_ARG && strstr(dn_last_error(), "bias workspace"),
          "bn backward finish (+ bias) null: %s", dn_last_error());
    int blocks = 0;
    o.bias_ws = (double*)p; o.bias_ws_bytes = 1 << 20; o.n_blocks = &blocks;
    CHECK(dn_bn_train_backward_finish(&b, (const double*)p, 16, &o, NULL) == DN_ERR_ARG && strstr(dn_last_error(), "not both"),
          "bn backward finish: dbias and n_blocks: %s", dn_last_error());
    o.n_blocks = NULL;
    b.n_groups = 2;             /* the bias gradient is a one-group form: the removed entry points could not even say this */
    CHECK(dn_bn_train_backward_finish(&b, (const double*)p, 16, &o, NULL) == DN_ERR_ARG && strstr(dn_last_error(), "one group"),
          "bn backward finish (+ bias), two groups: %s", dn_last_error());
  }
  memset(&d, 0, sizeof d);
  d.n_images = 4; d.h_in = 32; d.w_in = 32; d.c0 = 256; d.c_out = 256; d.ksize = 3; d.stride = 1; d.math = 2;
  CHECK(dn_spconv_ks_supported(&d, 1) == 1 && dn_spconv_ks_supported(&d, 4) == 1 && dn_spconv_ks_supported(&d, 3) == 0, "ks supported");
  d.c0 = 32;      /* two chunks: not four slices */
  CHECK(dn_spconv_ks_supported(&d, 4) == 0 && dn_spconv_ks_supported(&d, 2) == 1, "ks: fewer chunks than slices");
  d.ksize = 1;
  CHECK(dn_spconv_ks_supported(&d, 2) == 0, "ks: 1x1 layers have no sliced form");
  printf("C ABI error behaviour: ok\n");
  return 0;
}

static int gpu_conv(int math) {
  const int n = 2, h = 12, w = 20, cin = 32, cout = 48;
  dn_conv_desc d;
  memset(&d, 0, sizeof d);
  d.n_images = n; d.h_in = h; d.w_in = w; d.c0 = cin; d.c_out = cout; d.ksize = 3; d.stride = 1;
  d.relu = 1; d.ld0 = cin; d.ldo = cout; d.math = math;
  const size_t nx = (size_t)n * h * w * cin, ny = (size_t)n * h * w * cout, nw = (size_t)cout * cin * 9;
  float *x = malloc(nx * 4), *wt = malloc(nw * 4), *bias = malloc(cout * 4), *y = malloc(ny * 4), *ref = malloc(ny * 4);
  unsigned s = 7;
  for (size_t i = 0; i < nx; ++i) x[i] = frand(&s);
  for (size_t i = 0; i < nw; ++i) wt[i] = frand(&s) * 0.08f;
  for (int i = 0; i < cout; ++i) bias[i] = frand(&s) * 0.1f;
  for (int im = 0; im < n; ++im) for (int oy = 0; oy < h; ++oy) for (int ox = 0; ox < w; ++ox) for (int co = 0; co < cout; ++co) {
    double acc = bias[co];
    for (int dy = 0; dy < 3; ++dy) for (int dx = 0; dx < 3; ++dx) {
      const int iy = oy + dy - 1, ix = ox + dx - 1;
      if (iy < 0 || iy >= h || ix < 0 || ix >= w) continue;
      for (int ci = 0; ci < cin; ++ci)
        acc += (double)x[((size_t)(im * h + iy) * w + ix) * cin + ci] * wt[((size_t)co * cin + ci) * 9 + dy * 3 + dx];
    }
    ref[((size_t)(im * h + oy) * w + ox) * cout + co] = acc > 0 ? (float)acc : 0.f;
  }
  float *dx_, *dw, *db, *dp, *dsc, *dsh, *dy_;
  const size_t np = dn_conv_packed_weight_floats(&d);
  CHECK(np > 0, "packed size: %s", dn_last_error());
  HIP(hipMalloc((void**)&dx_, nx * 4)); HIP(hipMalloc((void**)&dw, nw * 4)); HIP(hipMalloc((void**)&db, cout * 4));
  HIP(hipMalloc((void**)&dp, np * 4)); HIP(hipMalloc((void**)&dsc, cout * 4)); HIP(hipMalloc((void**)&dsh, cout * 4));
  HIP(hipMalloc((void**)&dy_, ny * 4));
  HIP(hipMemcpy(dx_, x, nx * 4, hipMemcpyHostToDevice)); HIP(hipMemcpy(dw, wt, nw * 4, hipMemcpyHostToDevice));
  HIP(hipMemcpy(db, bias, cout * 4, hipMemcpyHostToDevice));
  CHECK(dn_conv_pack_weights(&d, dw, dp, NULL) == DN_OK, "pack: %s", dn_last_error());
  CHECK(dn_fold_bn(db, NULL, NULL, NULL, NULL, 0.f, cout, dsc, dsh, NULL) == DN_OK, "fold: %s", dn_last_error());
  CHECK(dn_conv2d(&d, dx_, NULL, dp, dsc, dsh, dy_, NULL) == DN_OK, "conv: %s", dn_last_error());
  HIP(hipDeviceSynchronize());
  HIP(hipMemcpy(y, dy_, ny * 4, hipMemcpyDeviceToHost));
  double err = 0;
  for (size_t i = 0; i < ny; ++i) { const double e = fabs((double)y[i] - ref[i]); if (e > err) err = e; }
  printf("C ABI conv3x3 math=%d: max abs err %.3e\n", math, err);
  CHECK(err <= 1e-4, "conv error too large");
  /* dn_conv_last_form names that launch; dn_conv_force_config(2 = T3_128x64) moves it onto the 8 x 16 x 64 tile, whose
   * result is held to the same reference; an id of another family (4 = T3S2_64x64) leaves the choice to the cost model */
  {
    int form[11];
    CHECK(dn_conv_last_form(form, 11) == 11 && form[0] == 0 && form[1] == 3 && form[2] == 1 && form[7] == math && form[8] == 0 &&
          form[9] > 0 && form[9] <= form[10], "last form after dn_conv2d: entry %d KS %d", form[0], form[1]);
    CHECK(dn_conv_force_config(2) == DN_OK, "force: %s", dn_last_error());
    const int rc = dn_conv2d(&d, dx_, NULL, dp, dsc, dsh, dy_, NULL);
    dn_conv_force_config(-1);
    CHECK(rc == DN_OK, "conv (forced): %s", dn_last_error());
    HIP(hipDeviceSynchronize());
    HIP(hipMemcpy(y, dy_, ny * 4, hipMemcpyDeviceToHost));
    CHECK(dn_conv_last_form(form, 11) == 11 && form[3] == 8 && form[4] == 16 && form[5] == 64, "forced T3_128x64 ran %dx%dx%d", form[3], form[4], form[5]);
    double e3 = 0;
    for (size_t i = 0; i < ny; ++i) { const double e = fabs((double)y[i] - ref[i]); if (e > e3) e3 = e; }
    CHECK(e3 <= 1e-4, "forced-tile conv error too large");
    CHECK(dn_conv_force_config(4) == DN_OK, "force: %s", dn_last_error());      /* a stride-2 id: not a candidate here */
    const int rc2 = dn_conv2d(&d, dx_, NULL, dp, dsc, dsh, dy_, NULL);
    dn_conv_force_config(-1);
    CHECK(rc2 == DN_OK, "conv (foreign id): %s", dn_last_error());
    HIP(hipDeviceSynchronize());
    HIP(hipMemcpy(y, dy_, ny * 4, hipMemcpyDeviceToHost));
    CHECK(dn_conv_last_form(form, 11) == 11 && form[2] == 1, "a foreign forced id changed the stride");
  }
  /* dn_conv2d_taps: every tap enabled and the dense output strides == dn_conv2d, bit for bit; the centre tap alone
   * (mask 1 << 4) into every other pixel column of a twice-as-wide buffer == the 1x1 conv of the centre weights */
  {
    float *dy2, *y2 = malloc(ny * 4 * 2);
    HIP(hipMalloc((void**)&dy2, ny * 4 * 2)); HIP(hipMemset(dy2, 0, ny * 4 * 2));
    CHECK(dn_conv2d_taps(&d, dx_, NULL, dp, dsc, dsh, dy2, 0x1ff, (long)h * w * cout, w * cout, cout, NULL) == DN_OK, "taps: %s", dn_last_error());
    HIP(hipDeviceSynchronize());
    HIP(hipMemcpy(y2, dy2, ny * 4, hipMemcpyDeviceToHost));
    CHECK(memcmp(y, y2, ny * 4) == 0, "dn_conv2d_taps with every tap differs from dn_conv2d");
    CHECK(dn_conv2d_taps(&d, dx_, NULL, dp, dsc, dsh, dy2, 1 << 4, (long)h * w * cout * 2, w * cout * 2, cout * 2, NULL) == DN_OK, "taps: %s", dn_last_error());
    HIP(hipDeviceSynchronize());
    HIP(hipMemcpy(y2, dy2, ny * 4 * 2, hipMemcpyDeviceToHost));
    double e2 = 0;
    for (int im = 0; im < n; ++im) for (int oy = 0; oy < h; ++oy) for (int ox = 0; ox < w; ++ox) for (int co = 0; co < cout; ++co) {
      double acc = bias[co];
      for (int ci = 0; ci < cin; ++ci) acc += (double)x[((size_t)(im * h + oy) * w + ox) * cin + ci] * wt[((size_t)co * cin + ci) * 9 + 4];
      const double want = acc > 0 ? acc : 0, got = y2[(((size_t)(im * h + oy) * w + ox) * 2) * cout + co];
      if (fabs(got - want) > e2) e2 = fabs(got - want);
    }
    printf("C ABI conv3x3 math=%d, centre tap only, strided output: max abs err %.3e\n", math, e2);
    CHECK(e2 <= 1e-4, "tap-masked conv error too large");
    CHECK(dn_conv2d_taps(&d, dx_, NULL, dp, dsc, dsh, dy2, 0, 1, 1, cout, NULL) == DN_ERR_ARG, "empty tap mask accepted");
  }
  return 0;
}

static int gpu_voxel(void) {
  const int npts = 5000;
  float* pts = malloc((size_t)npts * 4 * 4);
  unsigned s = 3;
  for (int i = 0; i < npts; ++i) {
    pts[4 * i] = frand(&s) * 33.f; pts[4 * i + 1] = frand(&s) * 33.f; pts[4 * i + 2] = frand(&s) * 3.f - 0.5f; pts[4 * i + 3] = 0.f;
  }
  const double vs[3] = {0.25, 0.25, 0.4}, ext[6] = {-32, 32, -32, 32, -3, 2};
  const int dims[3] = {256, 256, 13};
  const size_t cells = 256 * 256 * 13;
  float* ref = calloc(cells, 4);
  for (int i = 0; i < npts; ++i) {
    const double x = pts[4 * i], y = pts[4 * i + 1], z = pts[4 * i + 2];
    if (!(ext[0] < x && x < ext[1] && ext[2] < y && y < ext[3] && ext[4] < z && z < ext[5])) continue;
    const int qx = (int)floor(x / vs[0]) + 128, qy = (int)floor(y / vs[1]) + 128, qz = (int)floor(z / vs[2]) + 8;
    ref[((size_t)qx * 256 + qy) * 13 + qz] = 1.f;
  }
  float *dp, *dd, *out = malloc(cells * 4);
  HIP(hipMalloc((void**)&dp, (size_t)npts * 16)); HIP(hipMalloc((void**)&dd, cells * 4));
  HIP(hipMemcpy(dp, pts, (size_t)npts * 16, hipMemcpyHostToDevice));
  CHECK(dn_voxelize_occupy(dp, npts, 4, vs, ext, dims, dd, NULL) == DN_OK, "voxelize: %s", dn_last_error());
  HIP(hipDeviceSynchronize());
  HIP(hipMemcpy(out, dd, cells * 4, hipMemcpyDeviceToHost));
  CHECK(memcmp(out, ref, cells * 4) == 0, "voxel grids differ");
  printf("C ABI voxelizer: bit-exact\n");
  return 0;
}

/* ---- the inference engine's default path: dn_spconv_pack_weights -> dn_spconv2d -> dn_sp_to_nhwc, plain and
 * over cat([upsample x2 (src0), src1]) (the tap-merged image / kernel), against C loops ---- */
static int gpu_spconv(int up) {
  const int n = 2, h = 16, w = 40, c0 = up ? 32 : 24, c1 = up ? 16 : 0, cin = c0 + c1, cout = 40;
  const int h0 = up ? h / 2 : h, w0 = up ? w / 2 : w;
  dn_conv_desc d;
  memset(&d, 0, sizeof d);
  d.n_images = n; d.h_in = h; d.w_in = w; d.c0 = c0; d.c1 = c1; d.up0 = up; d.c_out = cout; d.ksize = 3; d.stride = 1;
  d.relu = 1; d.ld0 = c0; d.ld1 = c1; d.ldo = cout; d.math = 2;
  const size_t n0 = (size_t)n * h0 * w0 * c0, n1 = (size_t)n * h * w * c1, ny = (size_t)n * h * w * cout, nw = (size_t)cout * cin * 9;
  float *x0 = malloc(n0 * 4), *x1 = malloc((n1 + 1) * 4), *wt = malloc(nw * 4), *bias = malloc(cout * 4), *y = malloc(ny * 4), *ref = malloc(ny * 4);
  unsigned s = 11 + up;
  for (size_t i = 0; i < n0; ++i) x0[i] = frand(&s);
  for (size_t i = 0; i < n1; ++i) x1[i] = frand(&s);
  for (size_t i = 0; i < nw; ++i) wt[i] = frand(&s) * 0.08f;
  for (int i = 0; i < cout; ++i) bias[i] = frand(&s) * 0.1f;
  for (int im = 0; im < n; ++im) for (int oy = 0; oy < h; ++oy) for (int ox = 0; ox < w; ++ox) for (int co = 0; co < cout; ++co) {
    double acc = bias[co];
    for (int dy = 0; dy < 3; ++dy) for (int dx = 0; dx < 3; ++dx) {
      const int iy = oy + dy - 1, ix = ox + dx - 1;
      if (iy < 0 || iy >= h || ix < 0 || ix >= w) continue;
      const int sy = up ? iy / 2 : iy, sx = up ? ix / 2 : ix;
      for (int ci = 0; ci < c0; ++ci)
        acc += (double)x0[((size_t)(im * h0 + sy) * w0 + sx) * c0 + ci] * wt[((size_t)co * cin + ci) * 9 + dy * 3 + dx];
      for (int ci = 0; ci < c1; ++ci)
        acc += (double)x1[((size_t)(im * h + iy) * w + ix) * c1 + ci] * wt[((size_t)co * cin + c0 + ci) * 9 + dy * 3 + dx];
    }
    ref[((size_t)(im * h + oy) * w + ox) * cout + co] = acc > 0 ? (float)acc : 0.f;
  }
  float *dx0, *dx1 = NULL, *dw, *db, *dsc, *dsh, *dy_;
  void *sp0, *sp1 = NULL, *spo, *pk;
  const size_t pkb = dn_spconv_packed_weight_bytes(&d);
  CHECK(pkb > 0, "sp packed size: %s", dn_last_error());
  HIP(hipMalloc((void**)&dx0, n0 * 4)); HIP(hipMalloc((void**)&dw, nw * 4)); HIP(hipMalloc((void**)&db, cout * 4));
  HIP(hipMalloc((void**)&dsc, cout * 4)); HIP(hipMalloc((void**)&dsh, cout * 4)); HIP(hipMalloc((void**)&dy_, ny * 4));
  HIP(hipMalloc(&sp0, dn_sp_tensor_bytes(n, h0, w0, c0))); HIP(hipMalloc(&spo, dn_sp_tensor_bytes(n, h, w, cout))); HIP(hipMalloc(&pk, pkb));
  HIP(hipMemcpy(dx0, x0, n0 * 4, hipMemcpyHostToDevice)); HIP(hipMemcpy(dw, wt, nw * 4, hipMemcpyHostToDevice));
  HIP(hipMemcpy(db, bias, cout * 4, hipMemcpyHostToDevice));
  CHECK(dn_sp_from_nhwc(dx0, n, h0, w0, c0, c0, sp0, NULL) == DN_OK, "from_nhwc: %s", dn_last_error());
  if (c1) {
    HIP(hipMalloc((void**)&dx1, n1 * 4)); HIP(hipMalloc(&sp1, dn_sp_tensor_bytes(n, h, w, c1)));
    HIP(hipMemcpy(dx1, x1, n1 * 4, hipMemcpyHostToDevice));
    CHECK(dn_sp_from_nhwc(dx1, n, h, w, c1, c1, sp1, NULL) == DN_OK, "from_nhwc: %s", dn_last_error());
  }
  const float wmul = 4096.f;   /* lifts |w| <= 0.08 out of the f16 subnormal range; undone in the scale */
  CHECK(dn_spconv_pack_weights(&d, dw, wmul, pk, NULL) == DN_OK, "sp pack: %s", dn_last_error());
  {
    /* the one-launch form of many packs (dn_spconv_pack_weights_multi): one mode-0 job = the call above, byte for byte; a
     * tap-merged layer (the upsampled source) is refused by the prepare step */
    dn_pack_job job;
    memset(&job, 0, sizeof job);
    void *pk2, *table;
    HIP(hipMalloc(&pk2, pkb));
    job.desc = d; job.weight = dw; job.packed = pk2; job.mode = 0; job.cin_total = cin; job.wmul = wmul;
    const size_t tb = dn_spconv_pack_multi_table_bytes(1);
    CHECK(tb > 0, "pack multi table size");
    void* host = malloc(tb);
    int blocks = 0;
    const int rc = dn_spconv_pack_multi_prepare(&job, 1, host, &blocks);
    if (up) {
      CHECK(rc == DN_ERR_UNSUPPORTED, "pack multi accepted a tap-merged layer");
    } else {
      CHECK(rc == DN_OK && blocks > 0, "pack multi prepare: %s", dn_last_error());
      HIP(hipMalloc(&table, tb));
      HIP(hipMemcpy(table, host, tb, hipMemcpyHostToDevice));
      CHECK(dn_spconv_pack_weights_multi(table, 1, blocks, NULL) == DN_OK, "pack multi: %s", dn_last_error());
      HIP(hipDeviceSynchronize());
      unsigned char *a = malloc(pkb), *b = malloc(pkb);
      HIP(hipMemcpy(a, pk, pkb, hipMemcpyDeviceToHost)); HIP(hipMemcpy(b, pk2, pkb, hipMemcpyDeviceToHost));
      CHECK(memcmp(a, b, pkb) == 0, "pack multi differs from dn_spconv_pack_weights");
      printf("C ABI spconv pack multi: %zu bytes equal to the single launch's\n", pkb);
      free(a); free(b); HIP(hipFree(table));
    }
    free(host); HIP(hipFree(pk2));
    /* the fp32-NHWC engine's twin: one mode-0 job with wmul = 1 == dn_conv_pack_weights, fp32 rows and split-f16 rows */
    for (int math = 0; math < 2; ++math) {
      dn_conv_desc dn = d;
      dn.up0 = 0; dn.c0 = cin; dn.c1 = 0; dn.ld0 = cin; dn.ld1 = 0; dn.ldo = cout; dn.math = math;
      const size_t nf = dn_conv_packed_weight_floats(&dn);
      CHECK(nf > 0, "nhwc packed size: %s", dn_last_error());
      float *p1, *p2;
      HIP(hipMalloc((void**)&p1, nf * 4)); HIP(hipMalloc((void**)&p2, nf * 4));
      CHECK(dn_conv_pack_weights(&dn, dw, p1, NULL) == DN_OK, "nhwc pack: %s", dn_last_error());
      memset(&job, 0, sizeof job);
      job.desc = dn; job.weight = dw; job.packed = p2; job.mode = 0; job.cin_total = cin; job.wmul = 1.f;
      const size_t tn = dn_conv_pack_multi_table_bytes(1);
      void* hostn = malloc(tn);
      CHECK(dn_conv_pack_multi_prepare(&job, 1, hostn, &blocks) == DN_OK && blocks > 0, "nhwc pack multi prepare: %s", dn_last_error());
      HIP(hipMalloc(&table, tn));
      HIP(hipMemcpy(table, hostn, tn, hipMemcpyHostToDevice));
      CHECK(dn_conv_pack_weights_multi(table, 1, blocks, NULL) == DN_OK, "nhwc pack multi: %s", dn_last_error());
      HIP(hipDeviceSynchronize());
      unsigned char *a = malloc(nf * 4), *b = malloc(nf * 4);
      HIP(hipMemcpy(a, p1, nf * 4, hipMemcpyDeviceToHost)); HIP(hipMemcpy(b, p2, nf * 4, hipMemcpyDeviceToHost));
      CHECK(memcmp(a, b, nf * 4) == 0, "nhwc pack multi differs from dn_conv_pack_weights (math %d)", math);
      free(a); free(b); free(hostn); HIP(hipFree(table)); HIP(hipFree(p1)); HIP(hipFree(p2));
    }
    printf("C ABI conv pack multi: equal to dn_conv_pack_weights, fp32 and split-f16 rows\n");
  }
  CHECK(dn_fold_bn(db, NULL, NULL, NULL, NULL, 0.f, cout, dsc, dsh, NULL) == DN_OK, "fold: %s", dn_last_error());
  float* hsc = malloc(cout * 4);
  HIP(hipMemcpy(hsc, dsc, cout * 4, hipMemcpyDeviceToHost));
  for (int i = 0; i < cout; ++i) hsc[i] /= wmul;
  HIP(hipMemcpy(dsc, hsc, cout * 4, hipMemcpyHostToDevice));
  CHECK(dn_spconv2d(&d, sp0, sp1, pk, dsc, dsh, spo, NULL) == DN_OK, "spconv: %s", dn_last_error());
  CHECK(dn_sp_to_nhwc(spo, n, h, w, cout, cout, dy_, NULL) == DN_OK, "to_nhwc: %s", dn_last_error());
  HIP(hipDeviceSynchronize());
  HIP(hipMemcpy(y, dy_, ny * 4, hipMemcpyDeviceToHost));
  double err = 0;
  for (size_t i = 0; i < ny; ++i) { const double e = fabs((double)y[i] - ref[i]); if (e > err) err = e; }
  printf("C ABI spconv 3x3 %s: max abs err %.3e, range flags %u\n", up ? "over cat(up2(src0), src1)" : "plain", err,
         dn_sp_range_flags(0));
  CHECK(err <= 1e-4, "spconv error too large");
  CHECK(dn_sp_range_flags(1) == 0, "range flags set on O(1) data");
  /* K-sliced form (2 slices: cin is 24 or 48 channels = 2 or 3 chunks): split through the workspace == every tile whole,
   * bit for bit; values within the engine's tolerance of the C loops */
  {
    const size_t ob = dn_sp_tensor_bytes(n, h, w, cout), wsb = dn_spconv_workspace_bytes(&d, 2);
    void *o1, *o2, *ws;
    CHECK(wsb > 0, "ks workspace size");
    HIP(hipMalloc(&o1, ob)); HIP(hipMalloc(&o2, ob)); HIP(hipMalloc(&ws, wsb));
    CHECK(dn_spconv2d_ks(&d, 2, sp0, sp1, pk, dsc, dsh, o1, NULL, 0, ws, wsb, NULL) == DN_OK, "spconv ks: %s", dn_last_error());
    CHECK(dn_spconv2d_ks(&d, 2, sp0, sp1, pk, dsc, dsh, o2, NULL, 0, NULL, 0, NULL) == DN_OK, "spconv ks (no workspace): %s", dn_last_error());
    CHECK(dn_sp_to_nhwc(o1, n, h, w, cout, cout, dy_, NULL) == DN_OK, "to_nhwc: %s", dn_last_error());
    HIP(hipDeviceSynchronize());
    unsigned char *b1 = malloc(ob), *b2 = malloc(ob);
    HIP(hipMemcpy(b1, o1, ob, hipMemcpyDeviceToHost)); HIP(hipMemcpy(b2, o2, ob, hipMemcpyDeviceToHost));
    HIP(hipMemcpy(y, dy_, ny * 4, hipMemcpyDeviceToHost));
    double e2 = 0;
    for (size_t i = 0; i < ny; ++i) { const double e = fabs((double)y[i] - ref[i]); if (e > e2) e2 = e; }
    CHECK(memcmp(b1, b2, ob) == 0, "K-sliced conv: split and whole tiles differ");
    CHECK(e2 <= 1e-4, "K-sliced conv error too large");
    CHECK(dn_spconv2d_ks(&d, 3, sp0, sp1, pk, dsc, dsh, o1, NULL, 0, ws, wsb, NULL) == DN_ERR_ARG, "kslices = 3 accepted");
    printf("C ABI spconv K-sliced (2 slices): max abs err %.3e, split == whole bitwise\n", e2);
  }
  return 0;
}

/* ---- hi-only occupancy planes: dn_scatter_dense_sp_hi + dn_spconv2d(math = 3) == the full SP form, bit for bit;
 * and the range flag: a value above 65504 through dn_sp_from_nhwc must raise bit 0 ---- */
static int gpu_hi_only_and_flags(void) {
  const int n = 2, X = 24, Y = 40, Z = 13, cout = 32, nidx = 900;
  int32_t* idx = malloc((size_t)nidx * 12);
  int32_t off[3] = {0, 400, nidx};
  unsigned s = 5;
  for (int i = 0; i < nidx; ++i) {
    idx[3 * i] = (int)((frand(&s) * 0.5f + 0.5f) * X) % X; idx[3 * i + 1] = (int)((frand(&s) * 0.5f + 0.5f) * Y) % Y;
    idx[3 * i + 2] = (int)((frand(&s) * 0.5f + 0.5f) * Z) % Z;
  }
  const int dims[3] = {X, Y, Z};
  dn_conv_desc d;
  memset(&d, 0, sizeof d);
  d.n_images = n; d.h_in = X; d.w_in = Y; d.c0 = Z; d.c_out = cout; d.ksize = 3; d.stride = 1; d.relu = 1; d.math = 2;
  const size_t nw = (size_t)cout * Z * 9, full_b = dn_sp_tensor_bytes(n, X, Y, Z), ob = dn_sp_tensor_bytes(n, X, Y, cout);
  float *wt = malloc(nw * 4), *sc = malloc(cout * 4), *sh = malloc(cout * 4);
  for (size_t i = 0; i < nw; ++i) wt[i] = frand(&s) * 0.2f;
  for (int i = 0; i < cout; ++i) { sc[i] = 1.f / 1024.f; sh[i] = frand(&s) * 0.1f; }
  int32_t *didx, *doff; float *dw, *dsc, *dsh; void *spf, *sph, *pk, *o1, *o2;
  HIP(hipMalloc((void**)&didx, (size_t)nidx * 12)); HIP(hipMalloc((void**)&doff, 12)); HIP(hipMalloc((void**)&dw, nw * 4));
  HIP(hipMalloc((void**)&dsc, cout * 4)); HIP(hipMalloc((void**)&dsh, cout * 4));
  HIP(hipMalloc(&spf, full_b)); HIP(hipMalloc(&sph, full_b / 2)); HIP(hipMalloc(&o1, ob)); HIP(hipMalloc(&o2, ob));
  HIP(hipMalloc(&pk, dn_spconv_packed_weight_bytes(&d)));
  HIP(hipMemcpy(didx, idx, (size_t)nidx * 12, hipMemcpyHostToDevice)); HIP(hipMemcpy(doff, off, 12, hipMemcpyHostToDevice));
  HIP(hipMemcpy(dw, wt, nw * 4, hipMemcpyHostToDevice)); HIP(hipMemcpy(dsc, sc, cout * 4, hipMemcpyHostToDevice));
  HIP(hipMemcpy(dsh, sh, cout * 4, hipMemcpyHostToDevice));
  CHECK(dn_scatter_dense_sp(didx, doff, n, nidx, dims, spf, NULL) == DN_OK, "scatter sp: %s", dn_last_error());
  CHECK(dn_scatter_dense_sp_hi(didx, doff, n, nidx, dims, sph, NULL) == DN_OK, "scatter sp hi: %s", dn_last_error());
  CHECK(dn_spconv_pack_weights(&d, dw, 1024.f, pk, NULL) == DN_OK, "pack: %s", dn_last_error());
  CHECK(dn_spconv2d(&d, spf, NULL, pk, dsc, dsh, o1, NULL) == DN_OK, "spconv full: %s", dn_last_error());
  d.math = 3;
  CHECK(dn_spconv2d(&d, sph, NULL, pk, dsc, dsh, o2, NULL) == DN_OK, "spconv hi-only: %s", dn_last_error());
  HIP(hipDeviceSynchronize());
  unsigned char *h1 = malloc(ob), *h2 = malloc(ob);
  HIP(hipMemcpy(h1, o1, ob, hipMemcpyDeviceToHost)); HIP(hipMemcpy(h2, o2, ob, hipMemcpyDeviceToHost));
  CHECK(memcmp(h1, h2, ob) == 0, "hi-only conv differs from the full form");
  printf("C ABI hi-only occupancy planes: conv output bit-equal to the full form\n");
  /* occupancy words: dn_scatter_dense_bits against a host loop, dn_spconv2d(math = 4) against the same bytes */
  {
    uint32_t *dbits, *hb = malloc((size_t)n * X * Y * 4), *want = calloc((size_t)n * X * Y, 4);
    HIP(hipMalloc((void**)&dbits, (size_t)n * X * Y * 4));
    CHECK(dn_scatter_dense_bits(didx, doff, n, nidx, dims, dbits, NULL) == DN_OK, "scatter bits: %s", dn_last_error());
    HIP(hipMemset(o2, 0xff, ob));
    d.math = 4;
    CHECK(dn_spconv2d(&d, dbits, NULL, pk, dsc, dsh, o2, NULL) == DN_OK, "spconv bit grid: %s", dn_last_error());
    HIP(hipDeviceSynchronize());
    HIP(hipMemcpy(hb, dbits, (size_t)n * X * Y * 4, hipMemcpyDeviceToHost));
    for (int g = 0; g < n; ++g)
      for (int i = off[g]; i < off[g + 1]; ++i)
        want[((size_t)g * X + idx[3 * i]) * Y + idx[3 * i + 1]] |= 1u << idx[3 * i + 2];
    CHECK(memcmp(hb, want, (size_t)n * X * Y * 4) == 0, "occupancy words differ from the host loop");
    HIP(hipMemcpy(h2, o2, ob, hipMemcpyDeviceToHost));
    CHECK(memcmp(h1, h2, ob) == 0, "bit-grid conv differs from the full form");
    const int dims33[3] = {X, Y, 33};
    CHECK(dn_scatter_dense_bits(didx, doff, n, nidx, dims33, dbits, NULL) == DN_ERR_ARG, "33 bins accepted");
    d.c_out = 64;
    CHECK(dn_spconv2d(&d, dbits, NULL, pk, dsc, dsh, o2, NULL) != DN_OK, "bit grid with 64 output channels accepted");
    d.c_out = cout; d.math = 4;
    /* the stem pair in one launch: dn_spconv2d_pre_pair == dn_spconv2d(math 4) then dn_spconv2d, bit for bit */
    {
      dn_conv_desc d2 = d;
      d2.c0 = cout; d2.c_out = 24; d2.math = 2;
      const size_t nw2 = (size_t)24 * cout * 9, ob2 = dn_sp_tensor_bytes(n, X, Y, 24);
      float* wt2 = malloc(nw2 * 4);
      for (size_t i = 0; i < nw2; ++i) wt2[i] = frand(&s) * 0.1f;
      float* dw2; void *pk2, *mid, *o3, *o4;
      HIP(hipMalloc((void**)&dw2, nw2 * 4)); HIP(hipMalloc(&pk2, dn_spconv_packed_weight_bytes(&d2)));
      HIP(hipMalloc(&mid, ob)); HIP(hipMalloc(&o3, ob2)); HIP(hipMalloc(&o4, ob2));
      HIP(hipMemcpy(dw2, wt2, nw2 * 4, hipMemcpyHostToDevice));
      CHECK(dn_spconv_pack_weights(&d2, dw2, 1024.f, pk2, NULL) == DN_OK, "pack 2: %s", dn_last_error());
      CHECK(dn_spconv2d_pre_pair_supported(&d, &d2) == 1, "stem pair not supported");
      CHECK(dn_spconv2d(&d, dbits, NULL, pk, dsc, dsh, mid, NULL) == DN_OK, "layer 1: %s", dn_last_error());
      CHECK(dn_spconv2d(&d2, mid, NULL, pk2, dsc, dsh, o3, NULL) == DN_OK, "layer 2: %s", dn_last_error());
      HIP(hipMemset(o4, 0xff, ob2));
      CHECK(dn_spconv2d_pre_pair(&d, &d2, dbits, pk, dsc, dsh, pk2, dsc, dsh, o4, NULL) == DN_OK, "pre pair: %s", dn_last_error());
      HIP(hipDeviceSynchronize());
      unsigned char *h3 = malloc(ob2), *h4 = malloc(ob2);
      HIP(hipMemcpy(h3, o3, ob2, hipMemcpyDeviceToHost)); HIP(hipMemcpy(h4, o4, ob2, hipMemcpyDeviceToHost));
      CHECK(memcmp(h3, h4, ob2) == 0, "one-launch stem pair differs from the two launches");
      d2.stride = 2;
      CHECK(dn_spconv2d_pre_pair(&d, &d2, dbits, pk, dsc, dsh, pk2, dsc, dsh, o4, NULL) == DN_ERR_ARG, "stride-2 second layer accepted");
      printf("C ABI stem pair: one launch bit-equal to the two launches\n");
    }
    d.math = 3;
    printf("C ABI occupancy words: scatter == host loop, conv output bit-equal to the full form\n");
  }
  /* range guard */
  CHECK(dn_sp_range_flags(1) == 0, "flags not clean before the probe");
  float big[16] = {0}; big[3] = 70000.f; big[9] = 20000.f;
  float* dbig; void* spb;
  HIP(hipMalloc((void**)&dbig, sizeof big)); HIP(hipMalloc(&spb, dn_sp_tensor_bytes(1, 1, 1, 16)));
  HIP(hipMemcpy(dbig, big, sizeof big, hipMemcpyHostToDevice));
  CHECK(dn_sp_from_nhwc(dbig, 1, 1, 1, 16, 16, spb, NULL) == DN_OK, "from_nhwc: %s", dn_last_error());
  const unsigned f = dn_sp_range_flags(1);
  CHECK(f == 3u, "range flags after splitting 70000: %u (want 3)", f);
  CHECK(dn_sp_range_flags(0) == 0, "flags not cleared by reset");
  printf("C ABI range guard: clamp reported (flags 3), cleared by reset\n");
  return 0;
}

/* ---- fusion block on a small scene: dn_warp_neighbors + dn_disco_fuse_mlp
 * against a C restatement (two bilinear passes with zero padding, 4-layer MLP in double, exp / sum / weighted sum) ---- */
static float bil(const float* img, int h, int w, int c, float gx, float gy, int ch) {
  const float ix = ((gx + 1.f) * w - 1.f) * 0.5f, iy = ((gy + 1.f) * h - 1.f) * 0.5f;
  const float fx = floorf(ix), fy = floorf(iy);
  const int x0 = (int)fx, y0 = (int)fy;
  const float wx1 = ix - fx, wy1 = iy - fy;
  float acc = 0.f;
  for (int k = 0; k < 4; ++k) {
    const int x = x0 + (k & 1), y = y0 + (k >> 1);
    if (x < 0 || x >= w || y < 0 || y >= h) continue;
    acc += img[((size_t)y * w + x) * c + ch] * ((k & 1) ? wx1 : 1.f - wx1) * ((k >> 1) ? wy1 : 1.f - wy1);
  }
  return acc;
}

static int gpu_fusion(void) {
  enum { A = 3, B = 1, H = 8, W = 16, C = 64, HW = H * W };
  unsigned s = 21;
  float* feat = malloc((size_t)A * B * HW * C * 4);
  for (size_t i = 0; i < (size_t)A * B * HW * C; ++i) { const float v = frand(&s); feat[i] = v > 0 ? v : 0.f; }
  float trans[B][A][A][16];
  for (int i = 0; i < A; ++i) for (int j = 0; j < A; ++j) {
    const float th = 0.2f * (j - i), tx = 3.f * (j - i), ty = -2.f * (j - i);
    float* m = trans[0][i][j];
    memset(m, 0, 64);
    m[0] = cosf(th); m[1] = -sinf(th); m[4] = sinf(th); m[5] = cosf(th); m[3] = tx; m[7] = ty; m[10] = 1.f; m[15] = 1.f;
  }
  float w1[128 * 2 * C], b1[128], w2[32 * 128], b2[32], w3[8 * 32], b3[8], w4[8], b4[1];
  for (int i = 0; i < 128 * 2 * C; ++i) w1[i] = frand(&s) * 0.06f;   /* amplitudes keep s_k = O(1): exp() stays finite */
  for (int i = 0; i < 32 * 128; ++i) w2[i] = frand(&s) * 0.08f;
  for (int i = 0; i < 8 * 32; ++i) w3[i] = frand(&s) * 0.4f;
  for (int i = 0; i < 8; ++i) { w4[i] = frand(&s) * 1.5f; b3[i] = frand(&s) * 0.1f; }
  for (int i = 0; i < 128; ++i) b1[i] = frand(&s) * 0.1f;
  for (int i = 0; i < 32; ++i) b2[i] = frand(&s) * 0.1f;
  b4[0] = 0.05f;
  /* reference: warped maps, then the fusion of every ego */
  float* warped = calloc((size_t)A * (A - 1) * HW * C, 4);
  float* rot = malloc((size_t)HW * C * 4);
  for (int i = 0; i < A; ++i) for (int j = 0, jj = 0; j < A; ++j) {
    if (j == i) continue;
    const float* m = trans[0][i][j];
    const float* src = feat + (size_t)j * HW * C;
    const float xt = (4.f * m[3]) / 128.f, yt = -(4.f * m[7]) / 128.f;
    for (int y = 0; y < H; ++y) for (int x = 0; x < W; ++x) {
      const float bx = (2.f * x + 1.f) / W - 1.f, by = (2.f * y + 1.f) / H - 1.f;
      for (int ch = 0; ch < C; ++ch) rot[((size_t)y * W + x) * C + ch] = bil(src, H, W, C, m[0] * bx + m[1] * by, m[4] * bx + m[5] * by, ch);
    }
    for (int y = 0; y < H; ++y) for (int x = 0; x < W; ++x) {
      const float bx = (2.f * x + 1.f) / W - 1.f, by = (2.f * y + 1.f) / H - 1.f;
      for (int ch = 0; ch < C; ++ch)
        warped[(((size_t)i * (A - 1) + jj) * HW + (size_t)y * W + x) * C + ch] = bil(rot, H, W, C, bx + xt, by + yt, ch);
    }
    ++jj;
  }
  float* ref = malloc((size_t)A * HW * C * 4);
  for (int i = 0; i < A; ++i) for (int p = 0; p < HW; ++p) {
    const float* ego = feat + ((size_t)i * HW + p) * C;
    const float* nb[A];
    nb[0] = ego;
    for (int jj = 0; jj < A - 1; ++jj) nb[1 + jj] = warped + (((size_t)i * (A - 1) + jj) * HW + p) * C;
    double e[A], den = 0;
    for (int k = 0; k < A; ++k) {
      double h1[128], h2[32], h3[8], sk = b4[0];
      for (int u = 0; u < 128; ++u) {
        double acc = b1[u];
        for (int ch = 0; ch < C; ++ch) acc += (double)w1[u * 2 * C + ch] * ego[ch] + (double)w1[u * 2 * C + C + ch] * nb[k][ch];
        h1[u] = acc > 0 ? acc : 0;
      }
      for (int u = 0; u < 32; ++u) { double acc = b2[u]; for (int v = 0; v < 128; ++v) acc += w2[u * 128 + v] * h1[v]; h2[u] = acc > 0 ? acc : 0; }
      for (int u = 0; u < 8; ++u) { double acc = b3[u]; for (int v = 0; v < 32; ++v) acc += w3[u * 32 + v] * h2[v]; h3[u] = acc > 0 ? acc : 0; }
      for (int u = 0; u < 8; ++u) sk += w4[u] * h3[u];
      e[k] = exp(sk > 0 ? sk : 0);
      den += e[k];
    }
    for (int ch = 0; ch < C; ++ch) {
      double acc = 0;
      for (int k = 0; k < A; ++k) acc += e[k] / den * nb[k][ch];
      ref[((size_t)i * HW + p) * C + ch] = (float)acc;
    }
  }
  /* device side */
  float *dfeat, *dtrans, *dwarp, *dw1, *dw2, *dw3, *dv, *dout1, *dout2;
  int32_t* dna; void* dpk;
  const int32_t na = A;
  HIP(hipMalloc((void**)&dfeat, (size_t)A * HW * C * 4)); HIP(hipMalloc((void**)&dtrans, sizeof trans)); HIP(hipMalloc((void**)&dna, 4));
  HIP(hipMalloc((void**)&dwarp, (size_t)A * (A - 1) * HW * C * 4)); HIP(hipMalloc((void**)&dw1, sizeof w1)); HIP(hipMalloc((void**)&dw2, sizeof w2));
  HIP(hipMalloc((void**)&dw3, sizeof w3)); HIP(hipMalloc(&dpk, dn_fuse_mlp_packed_bytes(C)));
  HIP(hipMalloc((void**)&dout1, (size_t)A * HW * C * 4)); HIP(hipMalloc((void**)&dout2, (size_t)A * HW * C * 4));
  HIP(hipMemcpy(dfeat, feat, (size_t)A * HW * C * 4, hipMemcpyHostToDevice)); HIP(hipMemcpy(dtrans, trans, sizeof trans, hipMemcpyHostToDevice));
  HIP(hipMemcpy(dna, &na, 4, hipMemcpyHostToDevice)); HIP(hipMemcpy(dw1, w1, sizeof w1, hipMemcpyHostToDevice));
  HIP(hipMemcpy(dw2, w2, sizeof w2, hipMemcpyHostToDevice)); HIP(hipMemcpy(dw3, w3, sizeof w3, hipMemcpyHostToDevice));
  const float m1 = 16384.f, m2 = 16384.f, m3 = 8192.f;     /* powers of two lifting the weights; undone in s1..s3 */
  CHECK(dn_fuse_mlp_pack(dw1, dw2, dw3, C, m1, m2, m3, dpk, NULL) == DN_OK, "mlp pack: %s", dn_last_error());
  float vec[128 + 128 + 32 + 32 + 8 + 8 + 8 + 4];   /* s1 t1 s2 t2 s3 t3 w4 b4 (no BatchNorm: scale = 1 / wmul, shift = bias) */
  float *s1 = vec, *t1 = vec + 128, *s2 = vec + 256, *t2 = vec + 288, *s3 = vec + 320, *t3 = vec + 328, *pw4 = vec + 336, *pb4 = vec + 344;
  for (int i = 0; i < 128; ++i) { s1[i] = 1.f / m1; t1[i] = b1[i]; }
  for (int i = 0; i < 32; ++i) { s2[i] = 1.f / m2; t2[i] = b2[i]; }
  for (int i = 0; i < 8; ++i) { s3[i] = 1.f / m3; t3[i] = b3[i]; pw4[i] = w4[i]; }
  pb4[0] = b4[0];
  HIP(hipMalloc((void**)&dv, sizeof vec)); HIP(hipMemcpy(dv, vec, sizeof vec, hipMemcpyHostToDevice));
  dn_fuse_mlp_params prm = {dpk, dv, dv + 128, dv + 256, dv + 288, dv + 320, dv + 328, dv + 336, dv + 344};
  CHECK(dn_warp_neighbors(dfeat, dtrans, dna, B, A, H, W, C, 0, 0, A, dwarp, NULL) == DN_OK, "warp: %s", dn_last_error());
  CHECK(dn_disco_fuse_mlp(dfeat, dwarp, dna, &prm, B, A, HW, C, 0, 0, A, NULL, dout1, NULL, NULL) == DN_OK, "fuse_mlp: %s", dn_last_error());
  HIP(hipDeviceSynchronize());
  float *hw_ = malloc((size_t)A * (A - 1) * HW * C * 4), *o1 = malloc((size_t)A * HW * C * 4);
  HIP(hipMemcpy(hw_, dwarp, (size_t)A * (A - 1) * HW * C * 4, hipMemcpyDeviceToHost));
  HIP(hipMemcpy(o1, dout1, (size_t)A * HW * C * 4, hipMemcpyDeviceToHost));
  double ew = 0, e1 = 0;
  for (size_t i = 0; i < (size_t)A * (A - 1) * HW * C; ++i) { const double e = fabs((double)hw_[i] - warped[i]); if (e > ew) ew = e; }
  for (size_t i = 0; i < (size_t)A * HW * C; ++i) {
    const double e = fabs((double)o1[i] - ref[i]); if (e > e1) e1 = e;
  }
  printf("C ABI fusion: warp max abs err %.3e, warp + fuse_mlp %.3e\n", ew, e1);
  CHECK(ew <= 1e-5 && e1 <= 1e-4, "fusion error too large");
  /* fragment-major intermediate: dn_warp_neighbors_fm + dn_disco_fuse_mlp_fm == the pixel-major pair, bit for bit */
  CHECK(dn_warp_fm_supported(H, W, C), "fm form not offered for %d x %d x %d", H, W, C);
  CHECK(dn_warp_neighbors_fm(dfeat, dtrans, dna, B, A, H, W, C, 0, 0, A, dwarp, NULL) == DN_OK, "warp fm: %s", dn_last_error());
  CHECK(dn_disco_fuse_mlp_fm(dfeat, dwarp, dna, &prm, B, A, HW, C, 0, 0, A, NULL, dout2, NULL, NULL) == DN_OK, "fuse_mlp fm: %s", dn_last_error());
  {
    unsigned *dflag, hflag = 0;
    HIP(hipMalloc((void**)&dflag, 4)); HIP(hipMemcpy(dflag, &hflag, 4, hipMemcpyHostToDevice));
    CHECK(dn_sp_range_flags_async(dflag, 0, NULL) == DN_OK, "flags async: %s", dn_last_error());
    HIP(hipDeviceSynchronize());
    float* o2 = malloc((size_t)A * HW * C * 4);
    HIP(hipMemcpy(o2, dout2, (size_t)A * HW * C * 4, hipMemcpyDeviceToHost)); HIP(hipMemcpy(&hflag, dflag, 4, hipMemcpyDeviceToHost));
    CHECK(memcmp(o1, o2, (size_t)A * HW * C * 4) == 0, "fragment-major fusion differs from the pixel-major one");
    CHECK(hflag == 0, "stream-ordered range flags: %u on O(1) data", hflag);
    printf("C ABI fusion: fragment-major form == pixel-major form bitwise; stream-ordered range flags 0\n");
  }
  return 0;
}

int main(int argc, char** argv) {
  if (errors_only()) return 1;
  if (argc > 1 && strcmp(argv[1], "--gpu") == 0) {
    if (gpu_conv(0) || gpu_conv(1) || gpu_voxel()) return 1;
    if (gpu_spconv(0) || gpu_spconv(1) || gpu_hi_only_and_flags() || gpu_fusion()) return 1;
  }
  printf("OK\n");
  return 0;
}
