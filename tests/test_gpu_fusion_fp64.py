"""Every shipped form of the pose warp and of the fusion block against the float64 reference of tests/fusion_fp64.py,
over a pose sweep that goes round the circle, across the frame edge and through reflections and scalings, on square
and non-square maps.

Bounds.  Exact where exactness is promised (dead pairs and wholly out-of-frame warps are zeros, an ego sub-range is
the slice of the full result, the rigid backward on square maps repeats its bits).  Elsewhere: E = max |torch fp32 -
float64| of the same operation over the same sweep and inputs, computed in the test, and the kernel must stay within
FACTOR * E of float64.  FACTOR = 4 covers that the kernels form pixel-centre coordinates and contract multiply-adds in another
order than torch (each of the two passes can move a coordinate an ulp the other way); it is a margin over the
reference's own error, not over anything the kernels were seen to give.  Every element of every pose is compared.

Measured (MI355X; E on the CPU, `err` = max |kernel - float64| over all forms of the row):

forward warp (test_forward_warp_forms; 260 poses, 1024 randn channels, 250 poses leave a non-zero map)
    map      E          err        err / E
    32x32    1.468e-05  1.284e-05  0.87
    16x16    1.049e-05  5.354e-06  0.51
    64x64    4.870e-05  2.568e-05  0.53
    20x28    2.432e-05  1.498e-05  0.62
    12x16    9.537e-06  6.129e-06  0.64
    8x40     1.961e-05  2.821e-05  1.44   (list1024; the tiled kernel 2.578e-05, fragment-major the same bits)
    17x33    3.147e-05  1.551e-05  0.49   (no fragment-major form: refused)

warp backward (test_warp_backward_vs_float64_autograd; 272 poses, 262 of them non-zero; gradients summed over up to 67
warps per image)
    map      C     E          err scatter   err gather
    16x16    64    2.353e-05  1.278e-05     1.313e-05
    16x16    256   2.410e-05  1.334e-05     1.538e-05
    16x16    1024  2.667e-05  1.658e-05     1.605e-05
    32x32    64    2.889e-05  2.985e-05     2.665e-05
    32x32    256   3.237e-05  3.160e-05     3.008e-05
    32x32    1024  3.462e-05  3.157e-05     3.565e-05
    24x40    64    4.626e-05  4.936e-05     5.127e-05   (rigid=True on a non-square map: the scatter form)
    24x40    256   4.845e-05  5.204e-05     5.347e-05
    24x40    1024  5.468e-05  5.737e-05     5.737e-05
    (E moves by a few per cent from run to run: torch's threaded fp32 backward adds in no fixed order)

fusion block (test_fusion_block_forms_vs_fuse64): fused maps within 1e-4 (TOL of tests/test_gpu_fusion.py);
softmax weights within FACTOR * E_w, E_w = max |fp32 oracle weights - fuse64 weights|
    case                      E_w        err weights   err fused
    5x2 32x32x256             4.536e-08  4.172e-08     2.043e-06
    8x1 32x32x256             3.487e-08  3.393e-08     1.203e-06
    8x2 32x32x256 [5, 2]      8.427e-08  7.988e-08     3.421e-06
    4x2 20x28x128 [4, 3] v2i  8.929e-08  8.121e-08     2.766e-06
    3x1 12x16x64              5.540e-08  5.408e-08     1.091e-06
    1x2 16x16x256             0          0             0
    5x4 32x32x256             4.462e-08  4.631e-08     2.029e-06
    6x4 32x32x256 [6,3,6,1]   6.287e-08  6.287e-08     2.350e-06
    layer 4, 5x2 16x16x512    3.773e-08  3.638e-08     7.750e-07
    layer 4, 4x2 [4, 3] v2i   7.820e-08  7.164e-08     1.397e-06
    seg 3x2 12x16x512 [3, 2]  6.798e-08  6.798e-08     1.616e-06
    (wave layouts 0, 1, 2 and 4 of dn_disco_fuse_mlp gave the same figures in every row)

What these tests were seen to catch (value-only edits of warp.hip on a scratch copy, never committed):
  * `h` for `w` in the pass-2 base coordinate of warp_neighbors_tiled_kernel: fails the forward, indexing and fusion tests
    at every non-square map (the earlier suite passed it);
  * `wt[1]` / `wt[2]` swapped in the tiled kernel's pass-1 blend: fails at every map size;
  * the pass-2 clamp `WQ - 1` -> `WQ - 2` in tap2_row, and the candidate window -2..2 -> -1..1 of both warp_gather1
    kernels: NOT caught, and not catchable by a value test -- both variants gave the bits of the shipped kernels on every
    element of this sweep.  The tenth LDS column is read only when fp32 rounding splits floor() across a tile, and then
    with a weight of the size of that rounding; for |R R^T - 1| < 1e-3 a pixel q whose footprint reaches r lies within
    1.4143 of R^-1 r, hence within 1.92 (so: 1) of its rounding, per axis.  Both are safety margins, not arithmetic.
"""

import pytest
import torch

from tests import fusion_fp64 as f64

pytestmark = pytest.mark.gpu
FACTOR = 4.0
TOL = 1e-4                      # fused maps: tests/test_gpu_fusion.py, VERDICT row a9


def _dev():
    return torch.device("cuda:0")


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _pairs(A):
    """(ego i, neighbour j) in the order of warp_neighbors' [A, A-1] pair blocks"""
    return [(i, j) for i in range(A) for j in range(A) if j != i]


def _unpack_blocks(blocks, h, w, c):
    return torch.stack([f64.unpack_fm(b, h, w, c) for b in blocks.reshape(-1, h * w * c)])


def _report(title, rows):
    print("\n" + title)
    for r in rows:
        print("    " + r)


# ---------------------------------------------------------------------------------------------
# a. forward warp, every form on its own
# ---------------------------------------------------------------------------------------------
MASTER_C = 1024                 # one randn map per source image; a form at C channels sees the first C of them
TILED_C, PIXEL_C, LIST_C = (64, 128, 256, 512), (8, 36), (64, 1024)


@pytest.mark.parametrize("h,w", f64.MAP_SIZES)
def test_forward_warp_forms(h, w):
    """dn_warp_neighbors at C = 64 .. 512 (the tiled kernel every model runs), the same in the fragment-major order,
    C = 8 and 36 (one pixel per wave; 36: a partial row of lanes) and dn_warp_list at C = 64 and 1024: the whole sweep,
    thirty poses to a launch (six agents, one pose per (ego, neighbour) pair)."""
    from disconet_amd import ops, train_ops
    dev = _dev()
    poses, _ = f64.sweep(h, w)
    n = poses.shape[0]
    A = 6
    pairs = _pairs(A)
    fm_ok = (h * w) % 32 == 0
    assert ops.warp_fm_supported(h, w, 64) == fm_ok
    na = torch.tensor([A], dtype=torch.int32, device=dev)
    E, nonzero, errs = 0.0, 0, {}

    def note(form, out, want, zero):
        errs[form] = max(errs.get(form, 0.0), (out.double() - want).abs().max().item())
        if bool(zero.any()):                                      # wholly out of frame: zeros, exactly
            assert out[zero].abs().max().item() == 0.0, form

    for k0 in range(0, n, len(pairs)):
        chunk = poses[k0:k0 + len(pairs)]
        m = chunk.shape[0]
        maps = f64.sweep_maps(A, MASTER_C, h, w, seed=77 + k0)
        src = torch.tensor([j for _, j in pairs[:m]])
        ref64 = f64.warp_many(maps[src], chunk)
        ref32 = f64.warp_many(maps[src], chunk, torch.float32)
        E = max(E, (ref32.double() - ref64).abs().max().item())
        nonzero += int((ref64.abs().amax((1, 2, 3)) > 0).sum())
        # wholly out of frame: no tap of either pass in frame, in float64 and in fp32 alike.  (A shift of exactly one frame
        # width is on the edge: where w is no power of two, fp32 pixel centres land a rounding inside it -- torch's fp32
        # warp leaves 5e-6 at 64 m on the 20x28 map -- and the pose is held to the bound like any other.)
        zero = ((ref64.abs().amax((1, 2, 3)) == 0) & (ref32.abs().amax((1, 2, 3)) == 0)).to(dev)
        del ref32
        ref = _nhwc(ref64).to(dev)                               # [m, h, w, MASTER_C] float64
        del ref64
        trans = torch.eye(4).repeat(1, A, A, 1, 1)
        for k, (i, j) in enumerate(pairs[:m]):
            trans[0, i, j] = chunk[k]
        trans = trans.to(dev)
        for c in TILED_C + PIXEL_C:
            feat = _nhwc(maps[:, :c]).to(dev)
            out = ops.warp_neighbors(feat, trans, na, 1, A).view(len(pairs), h, w, c)[:m]
            note("nhwc%d" % c, out, ref[..., :c], zero)
            if c in TILED_C and fm_ok:
                out = ops.warp_neighbors(feat, trans, na, 1, A, fm=True)
                note("fm%d" % c, _unpack_blocks(out, h, w, c)[:m], ref[..., :c], zero)
        for c in LIST_C:
            feat = _nhwc(maps[:, :c]).to(dev)
            out = train_ops.warp_list(feat, chunk.to(dev), src.to(torch.int32).to(dev))
            note("list%d" % c, out, ref[..., :c], zero)
        del ref
    if not fm_ok:                                                 # no fragment-major form of this map: refused, by name
        feat = torch.zeros(A, h, w, 64, device=dev)
        with pytest.raises(Exception, match="fragment-major"):
            ops.warp_neighbors(feat, torch.eye(4).repeat(1, A, A, 1, 1).to(dev), na, 1, A, fm=True)
    worst = max(errs.values())
    _report("forward warp %dx%d: E = %.3e, worst form %.3e (%.2f E), %d of %d poses non-zero" % (h, w, E, worst, worst / E, nonzero, n),
            ["%-9s %.3e" % kv for kv in sorted(errs.items())])
    assert nonzero >= 0.9 * n
    assert len(errs) == len(TILED_C) * (2 if fm_ok else 1) + len(PIXEL_C) + len(LIST_C)
    for form, err in errs.items():
        assert err <= FACTOR * E, "%s: %.3e > %g * %.3e" % (form, err, FACTOR, E)


# ---------------------------------------------------------------------------------------------
# b. indexing of the batched form
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [64, 36])
@pytest.mark.parametrize("only_v2i", [False, True])
@pytest.mark.parametrize("A,B,live", [(5, 2, [3, 9]), (5, 2, [0, 5]), (8, 1, [6]), (8, 1, [11])])
def test_batched_warp_indexing(A, B, live, only_v2i, c):
    """a different pose for every (b, i, j): every live pair is warp64 of image j*B + b under trans[b, i, j], every
    dead pair (an agent beyond the live count -- a count above A is clamped --, only_v2i's skipped pairs) is zeros, an
    ego sub-range is bitwise the slice of the full result; tiled kernel (NHWC and fragment-major) and one-pixel kernel"""
    from disconet_amd import ops
    dev = _dev()
    h, w = 12, 16
    poses, _ = f64.sweep(h, w)
    g = torch.Generator().manual_seed(A * 100 + B * 10 + sum(live))
    trans = poses[torch.randperm(poses.shape[0], generator=g)[:B * A * A]].reshape(B, A, A, 4, 4).contiguous()
    maps = f64.sweep_maps(A * B, c, h, w, seed=5)
    pairs = _pairs(A)
    want = torch.zeros(B, A, A - 1, h, w, c, dtype=torch.float64)
    E, n_live = 0.0, 0
    dead = torch.ones(B, A, A - 1, dtype=torch.bool)
    for b in range(B):
        nb = max(0, min(live[b], A))
        for i, j in pairs:
            if i < nb and j < nb and not (only_v2i and i != 0 and j != 0):
                jj = j - (1 if j > i else 0)
                want[b, i, jj] = f64.warp64(maps[j * B + b], trans[b, i, j]).permute(1, 2, 0)
                ref32 = f64.warp_many(maps[j * B + b][None], trans[b, i, j][None], torch.float32)[0].permute(1, 2, 0)
                E = max(E, (ref32.double() - want[b, i, jj]).abs().max().item())
                dead[b, i, jj] = False
                n_live += 1
    assert (n_live > 0 or live[0] == 0) and n_live + int(dead.sum()) == B * A * (A - 1)
    feat = _nhwc(maps).to(dev)
    na = torch.tensor(live, dtype=torch.int32, device=dev)
    for fm in ((False, True) if c % 64 == 0 else (False,)):
        full = ops.warp_neighbors(feat, trans.to(dev), na, B, A, only_v2i, fm=fm)
        part = ops.warp_neighbors(feat, trans.to(dev), na, B, A, only_v2i, ego_first=1, ego_count=2, fm=fm)
        torch.cuda.synchronize()
        assert torch.equal(part, full[:, 1:3])
        got = (_unpack_blocks(full, h, w, c).view(full.shape) if fm else full).cpu()
        if bool(dead.any()):
            assert got[dead].abs().max().item() == 0.0
        err = (got.double() - want).abs().max().item()
        print("\nbatched warp A=%d B=%d live=%s v2i=%d c=%d fm=%d: E = %.3e, err = %.3e" % (A, B, live, only_v2i, c, fm, E, err))
        assert err <= FACTOR * E


# ---------------------------------------------------------------------------------------------
# c. warp backward against float64 autograd
# ---------------------------------------------------------------------------------------------
N_SRC, CHUNK = 4, 80


def _src_of(m):
    """source image of every warp of a chunk: image 0 feeds most of them (more than 64 when the chunk is full: two
    ballots of the lane-parallel gather), images 1 and 2 a few each, image 3 none"""
    return torch.tensor([{5: 1, 11: 2}.get(k % 12, 0) for k in range(m)], dtype=torch.int32)


@pytest.mark.parametrize("c", [64, 256, 1024])
@pytest.mark.parametrize("h,w", [(16, 16), (32, 32), (24, 40)])
def test_warp_backward_vs_float64_autograd(h, w, c):
    """dn_warp_backward against autograd through warp64: every pose of the sweep with rigid=False (atomic scatter),
    the rigid ones (the full circle, reflections, scale 1 +- 4e-4) with rigid=True as well (the gather form on square
    maps, run twice for the same bits; 24x40 must be right whichever kernel serves it).  The call ADDS to what d_src holds."""
    from disconet_amd import train_ops
    dev = _dev()
    poses, rigid = f64.sweep(h, w, backward=True)
    order = torch.cat([rigid.nonzero()[:, 0], (~rigid).nonzero()[:, 0]])
    n_rigid = int(rigid.sum())
    chunks = [(k, min(k + CHUNK, n_rigid), True) for k in range(0, n_rigid, CHUNK)] + [(n_rigid, len(order), False)]
    assert sum(b - a for a, b, _ in chunks) == poses.shape[0]
    assert int((_src_of(chunks[0][1] - chunks[0][0]) == 0).sum()) > 64           # two ballots of one image's warps
    E, nonzero, errs = 0.0, 0, {"scatter": 0.0, "gather": 0.0}
    for a, b, is_rigid in chunks:
        idx = order[a:b]
        m = len(idx)
        p = poses[idx]
        src = _src_of(m)
        g = torch.Generator().manual_seed(1000 * a + c)
        maps = torch.randn(N_SRC, c, h, w, generator=g)
        dwarp = torch.randn(m, c, h, w, generator=g)
        prior = torch.randn(N_SRC, c, h, w, generator=g)
        want = {}
        for dt in (torch.float64, torch.float32):
            x = maps.to(dt).requires_grad_(True)
            out = f64.warp_many(x[src.long()], p, dt)
            if dt == torch.float64:
                nonzero += int((out.detach().abs().amax((1, 2, 3)) > 0).sum())
            out.backward(dwarp.to(dt))
            want[dt] = prior.to(dt) + x.grad
            del out
        E = max(E, (want[torch.float32].double() - want[torch.float64]).abs().max().item())
        ref = _nhwc(want[torch.float64]).to(dev)
        dw, pd, sd = _nhwc(dwarp).to(dev), p.to(dev), src.to(dev)
        for form in (("scatter", "gather") if is_rigid else ("scatter",)):
            d_src = _nhwc(prior).to(dev)
            train_ops.warp_backward(dw, pd, sd, d_src, rigid=form == "gather")
            errs[form] = max(errs[form], (d_src.double() - ref).abs().max().item())
            assert torch.equal(d_src[3], _nhwc(prior)[3].to(dev))           # no warp reads image 3
            if form == "gather" and h == w:                      # the gather form (square maps): no atomics, same bits again
                again = _nhwc(prior).to(dev)
                train_ops.warp_backward(dw, pd, sd, again, rigid=True)
                assert torch.equal(again, d_src)
    print("\nwarp backward %dx%d C=%d: E = %.3e, scatter %.3e, gather %.3e, %d of %d poses non-zero"
          % (h, w, c, E, errs["scatter"], errs["gather"], nonzero, poses.shape[0]))
    assert nonzero >= 0.9 * poses.shape[0]
    for form, err in errs.items():
        assert err <= FACTOR * E, "%s: %.3e > %g * %.3e" % (form, err, FACTOR, E)


# ---------------------------------------------------------------------------------------------
# d. the whole fusion block
# ---------------------------------------------------------------------------------------------
def _sweep_trans(B, A, h, w, seed):
    """[B, A, A, 4, 4] drawn from the sweep (identity on the diagonal): neighbours rotate out of and into frame"""
    poses, _ = f64.sweep(h, w)
    g = torch.Generator().manual_seed(seed)
    trans = poses[torch.randint(0, poses.shape[0], (B * A * A,), generator=g)].reshape(B, A, A, 4, 4).clone()
    for i in range(A):
        trans[:, i, i] = torch.eye(4)
    return trans.contiguous()


def _set_bn_stats(fusion):
    for bn in (fusion.bn1_1, fusion.bn1_2, fusion.bn1_3):
        bn.running_mean.normal_(0, 0.1)
        bn.running_var.uniform_(0.5, 1.5)


def _check_fusion(name, run, fusion, A, B, h, w, c, live, v2i, layouts):
    """run(feat, trans, na) -> (fused [A*B, h, w, c], weights [B, A, A, hw]) on the GPU, in every wave layout of
    `layouts`, against fuse64 (fused maps: TOL; weights of the live egos: FACTOR * their fp32 oracle's distance)"""
    from disconet_amd import ops
    dev = _dev()
    live = live or [A] * B
    feat = torch.randn(A * B, h, w, c).clamp_(min=0)
    trans = _sweep_trans(B, A, h, w, seed=A * 10 + h)
    nchw = feat.permute(0, 3, 1, 2)
    fused64, w64 = f64.fuse64(f64.mlp_of(fusion, c), nchw, trans, live, A, B, v2i)
    _, w32 = f64.fuse32(f64.mlp_of(fusion, c, torch.float32), nchw, trans, live, A, B, v2i)
    E_w = (w32.double() - w64).abs().max().item()
    na = torch.tensor(live, dtype=torch.int32, device=dev)
    rows, bad = [], []
    try:
        for waves in layouts:
            if waves is not None:
                ops.set_fuse_mlp_waves(waves)
            fused, weights = run(feat.to(dev), trans.to(dev), na)
            torch.cuda.synchronize()
            err_f = (_nhwc(fused64) - fused.cpu().double()).abs().max().item()
            err_w = 0.0
            for b in range(B):
                nb = max(0, min(live[b], A))
                err_w = max(err_w, (weights[b, :nb].cpu().double() - w64[b, :nb]).abs().max().item())
            rows.append("%-24s waves=%-4s E_w = %.3e  weights %.3e  fused %.3e" % (name, waves, E_w, err_w, err_f))
            if err_f > TOL or err_w > FACTOR * E_w:
                bad.append(rows[-1])
    finally:
        ops.set_fuse_mlp_waves(0)
    _report("fusion block", rows)
    assert not bad, bad


@pytest.mark.parametrize("A,B,h,w,C,live,v2i", [
    (5, 2, 32, 32, 256, None, False),
    (8, 1, 32, 32, 256, None, False),
    (8, 2, 32, 32, 256, [5, 2], False),
    (4, 2, 20, 28, 128, [4, 3], True),
    (3, 1, 12, 16, 64, None, False),
    (1, 2, 16, 16, 256, None, False),
    (5, 4, 32, 32, 256, None, False),
    (6, 4, 32, 32, 256, [6, 3, 6, 1], False),
])
def test_fusion_block_forms_vs_fuse64(A, B, h, w, C, live, v2i):
    """the rows of test_four_wave_attention_launch_is_bit_identical_to_the_one_wave_form, each wave layout of
    dn_disco_fuse_mlp (the default choice, 1, 2, 4) against the float64 loop instead of against another layout"""
    from disconet_amd import Config, DiscoNet
    layer = {256: 3, 128: 2, 64: 1}[C]
    torch.manual_seed(3)
    m = DiscoNet(Config(), layer=layer, kd_flag=1, num_agent=A, only_v2i=v2i).eval()
    _set_bn_stats(m.pixel_weighted_fusion)
    m.cuda()
    P = m._get_plan()
    assert "_fuse_mlp" in P

    def run(feat, trans, na):
        return m.fuse(feat, trans, na, B, P, want_weights=True)
    _check_fusion("%dx%d %dx%dx%d" % (A, B, h, w, C), run, m.pixel_weighted_fusion, A, B, h, w, C, live, v2i, (0, 1, 2, 4))


@pytest.mark.parametrize("A,B,live,v2i", [(5, 2, None, False), (4, 2, [4, 3], True)])
def test_fusion_block_layer4_chain_vs_fuse64(A, B, live, v2i):
    """layer = 4 (C = 512): the dn_conv2d x2 + dn_disco_fuse_tail chain"""
    from disconet_amd import Config, DiscoNet
    torch.manual_seed(4)
    m = DiscoNet(Config(), layer=4, kd_flag=1, num_agent=A, only_v2i=v2i).eval()
    _set_bn_stats(m.pixel_weighted_fusion)
    m.cuda()
    P = m._get_plan()
    assert "_fuse_mlp" not in P

    def run(feat, trans, na):
        return m.fuse(feat, trans, na, B, P, want_weights=True)
    _check_fusion("layer4 %dx%d" % (A, B), run, m.pixel_weighted_fusion, A, B, 16, 16, 512, live, v2i, (None,))


def test_seg_model_fusion_vs_fuse64():
    """the segmentation model's fusion of its 512-channel bottleneck maps (non-square here)"""
    from disconet_amd.model import disco_fuse
    from disconet_amd.seg import SegDiscoNet
    torch.manual_seed(5)
    A, B = 3, 2
    m = SegDiscoNet(num_agent=A).eval()
    _set_bn_stats(m.pixel_weighted_fusion)
    m.cuda()
    P = m._get_plan()

    def run(feat, trans, na):
        fused, weights = disco_fuse(feat, trans, na, B, P, A, m.only_v2i, want_weights=True)
        assert torch.equal(m.fuse(feat, trans, na, B, P), fused)
        return fused, weights
    _check_fusion("seg %dx%d" % (A, B), run, m.pixel_weighted_fusion, A, B, 12, 16, 512, [3, 2], False, (None,))
