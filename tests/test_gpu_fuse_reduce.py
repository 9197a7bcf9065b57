"""The parameter-free collaboration baselines `--com sum | mean | max` on the GPU: the one-launch fusion
(ops.fuse_reduce, csrc/fuse_reduce.hip), the training step's list kernels, the three model classes, one training step and
the tools, against the float64 / fp32 twins of tests/reduce_fusion_ref.py.

Bounds (derived and computed in the tests, after tests/test_gpu_fusion_fp64.py).  E_w = max |fp32 torch warp - float64
warp| over the test's own warps, FACTOR = 4, R = (len - 1) 2^-24 max sum |terms| the rounding of the adds, len the longest
list; |kernel - float64| must stay within
    max: FACTOR E_w        mean: FACTOR E_w + R / len        sum: (len - 1) FACTOR E_w + R
Every test asserts E_w > 0 and that most warps leave a non-zero map.  Exact where exactness is promised: padded egos,
agents == 1, an ego whose neighbours are all wholly out of frame, max >= ego, an ego sub-range, two runs, a captured replay.

Measured (MI355X, one run; E_w on the CPU, err = max |kernel - float64|, 260 of 270 warps non-zero in every row):

sweep        E_w        sum err (bound)        mean err (bound)       max err (bound)
16x16x64     8.583e-06  7.356e-06 (1.750e-04)  1.226e-06 (3.489e-05)  4.511e-06 (3.433e-05)
12x20x128    9.421e-06  1.322e-05 (1.924e-04)  2.193e-06 (3.835e-05)  9.716e-06 (3.768e-05)
32x32x256    1.358e-05  1.485e-05 (2.754e-04)  2.455e-06 (5.495e-05)  9.595e-06 (5.431e-05)
16x16x512    1.144e-05  8.209e-06 (2.324e-04)  1.348e-06 (4.637e-05)  4.477e-06 (4.578e-05)
17x33x8      2.098e-05  1.941e-05 (4.233e-04)  3.245e-06 (8.453e-05)  1.426e-05 (8.392e-05)
17x33x36     2.432e-05  2.152e-05 (4.902e-04)  3.586e-06 (9.790e-05)  1.229e-05 (9.727e-05)

chain gradient   E (fp32 autograd vs float64)  err
16x16x64   sum 5.609e-06 / 4.589e-06, mean 1.610e-06 / 1.147e-06, max 3.931e-06 / 3.000e-06
32x32x256  sum 8.913e-06 / 7.067e-06, mean 2.394e-06 / 2.010e-06, max 6.978e-06 / 6.786e-06
"""
import os
import subprocess
import sys

import pytest
import torch

from tests import cases
from tests import fusion_fp64 as f64
from tests import reduce_fusion_ref as rf

pytestmark = pytest.mark.gpu
MODES = rf.MODES
TOL = 1e-4                      # the project's parity bar (tests/test_gpu_model.py)


def _dev():
    return torch.device("cuda:0")


def _same(a, b):
    """torch.equal with NaN == NaN (torch.equal treats +0 and -0 alike: the contract's tie rule does not tell them apart)"""
    return a.shape == b.shape and torch.equal(torch.isnan(a), torch.isnan(b)) and \
        torch.equal(torch.nan_to_num(a, nan=0.0), torch.nan_to_num(b, nan=0.0))


def _pairs(A):
    return [(i, j) for i in range(A) for j in range(A) if j != i]


# ---------------------------------------------------------------------------------------------
# a. the pose sweep
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,c", [(16, 16, 64), (12, 20, 128), (32, 32, 256), (16, 16, 512), (17, 33, 8), (17, 33, 36)])
def test_sweep_vs_float64(h, w, c):
    """every pose of fusion_fp64.sweep, thirty to a launch (six agents, one pose per (ego, neighbour) pair, lists of six),
    signed maps; the tiled kernel at c % 64 == 0 (12 x 20: ragged tiles both ways), the one-pixel-per-wave kernel at c = 8
    and 36 (a partial lane row)"""
    from disconet_amd import ops
    dev = _dev()
    poses, _ = f64.sweep(h, w)
    A, pairs = 6, _pairs(6)
    na = torch.tensor([A], dtype=torch.int32, device=dev)
    E_w, nonzero, n_warps, longest, sum_abs = 0.0, 0, 0, 1, 0.0
    errs = {m: 0.0 for m in MODES}
    for k0 in range(0, poses.shape[0], len(pairs)):
        chunk = poses[k0:k0 + len(pairs)]
        maps = f64.sweep_maps(A, c, h, w, seed=77 + k0)
        trans = torch.eye(4).repeat(1, A, A, 1, 1)
        for k in range(chunk.shape[0]):
            trans[0, pairs[k][0], pairs[k][1]] = chunk[k]
        ref = rf.Loop(maps, trans, [A], A, 1)
        E_w, longest, sum_abs = max(E_w, ref.E_w), max(longest, ref.longest), max(sum_abs, ref.sum_abs)
        nonzero, n_warps = nonzero + ref.nonzero, n_warps + ref.n_warps
        feat = rf.nhwc(maps).to(dev)
        for m in MODES:
            got = ops.fuse_reduce(feat, trans.to(dev), na, 1, A, m)
            errs[m] = max(errs[m], (got.cpu().double() - rf.nhwc(ref.fused[torch.float64][m])).abs().max().item())
            if m == "max":
                assert bool((got >= feat).all())
    print("\nfuse_reduce sweep %dx%dx%d: E_w = %.3e, %d of %d warps non-zero; %s" % (
        h, w, c, E_w, nonzero, n_warps, ", ".join("%s err %.3e (bound %.3e)" % (m, errs[m], rf.bound(m, E_w, longest, sum_abs))
                                                   for m in MODES)))
    assert E_w > 0 and nonzero >= 0.9 * n_warps and longest == A
    for m in MODES:
        assert errs[m] <= rf.bound(m, E_w, longest, sum_abs), (m, errs[m], rf.bound(m, E_w, longest, sum_abs))


# ---------------------------------------------------------------------------------------------
# b. indexing
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [64, 36])
@pytest.mark.parametrize("A,B,live,only_v2i", [(4, 2, [3, 2], False), (4, 2, [4, 3], True), (8, 1, [8], False),
                                               (4, 2, [0, 7], False)])
def test_indexing(A, B, live, only_v2i, c):
    """a different pose for every (b, i, j): live counts below A, 0 and above A (clamped), only_v2i, eight agents; padded
    egos pass through with their bits, an ego sub-range is the slice of the full result, two runs are bit-identical"""
    from disconet_amd import ops
    dev = _dev()
    h, w = 12, 16
    poses, _ = f64.sweep(h, w)
    g = torch.Generator().manual_seed(A * 100 + B * 10 + sum(live))
    trans = poses[torch.randperm(poses.shape[0], generator=g)[:B * A * A]].reshape(B, A, A, 4, 4).contiguous()
    maps = f64.sweep_maps(A * B, c, h, w, seed=5)
    ref = rf.Loop(maps, trans, live, A, B, only_v2i)
    feat = rf.nhwc(maps).to(dev)
    na = torch.tensor(live, dtype=torch.int32, device=dev)
    n_padded = 0
    for m in MODES:
        full = ops.fuse_reduce(feat, trans.to(dev), na, B, A, m, only_v2i)
        again = ops.fuse_reduce(feat, trans.to(dev), na, B, A, m, only_v2i)
        part = ops.fuse_reduce(feat, trans.to(dev), na, B, A, m, only_v2i, ego_first=1, ego_count=2)
        torch.cuda.synchronize()
        assert torch.equal(full, again)
        assert torch.equal(part, full[B:3 * B])
        for b, i, js in rf.lists_of(live, A, B, only_v2i):
            if not js:                                   # a padded ego, or only_v2i's ego without a listed neighbour
                assert torch.equal(full[i * B + b], feat[i * B + b]), (m, b, i)
                n_padded += 1
        err = (full.cpu().double() - rf.nhwc(ref.fused[torch.float64][m])).abs().max().item()
        print("\nfuse_reduce A=%d B=%d live=%s v2i=%d c=%d %s: E_w = %.3e, err = %.3e (bound %.3e)"
              % (A, B, live, only_v2i, c, m, ref.E_w, err, ref.bound(m)))
        assert err <= ref.bound(m)
        if m == "max":
            assert bool((full >= feat).all())
    assert ref.E_w > 0 and ref.nonzero >= 0.7 * ref.n_warps      # (random poses of the sweep: a quarter shift the map out)
    assert n_padded > 0 or live == [8]


def test_exact_where_exactness_is_promised():
    """agents == 1 copies; an ego whose neighbours are all wholly out of frame (float64 and fp32 references both zero): sum
    gives the ego's bits, mean the ego's map over (float)len, max the ego's map against zero"""
    from disconet_amd import ops
    dev = _dev()
    for c in (64, 36):
        h, w = 16, 24
        maps = f64.sweep_maps(3, c, h, w, seed=9)
        feat = rf.nhwc(maps).to(dev)
        eye = torch.eye(4).repeat(3, 1, 1, 1, 1).to(dev)
        for m in MODES:      # agents == 1, batch 3
            got = ops.fuse_reduce(feat, eye, torch.tensor([1, 0, 5], dtype=torch.int32, device=dev), 3, 1, m)
            assert torch.equal(got, feat), m
        A = 3
        trans = torch.eye(4).repeat(1, A, A, 1, 1)
        far = [f64.pose(0.3, 500.0, 500.0), f64.pose(0.0, -500.0, 3.0), f64.pose(1.0, 1e4, -1e4)]
        for k, (i, j) in enumerate(_pairs(A)):
            trans[0, i, j] = torch.from_numpy(far[k % 3])
        ref = rf.Loop(maps, trans, [A], A, 1)
        assert all(ref.zero_nb.values()) and ref.n_warps == 6
        na = torch.tensor([A], dtype=torch.int32, device=dev)
        three = torch.tensor(3.0, device=dev)
        assert torch.equal(ops.fuse_reduce(feat, trans.to(dev), na, 1, A, "sum"), feat)
        assert torch.equal(ops.fuse_reduce(feat, trans.to(dev), na, 1, A, "mean"), feat / three)
        assert torch.equal(ops.fuse_reduce(feat, trans.to(dev), na, 1, A, "max"), feat.clamp(min=0))


def test_max_choice_on_ties_zeros_nan_and_inf():
    """post-ReLU maps with many exact zeros (ties between the ego and its neighbours), NaN and +-inf planted in one
    neighbour; identity and whole-pixel poses on a 32 x 32 map, where torch's fp32 warp and the kernel's are both exact
    copies: the kernel's result equals host_fuse_reduce's, NaN for NaN"""
    from disconet_amd import ops
    from disconet_amd.fusion_modes import host_fuse_reduce
    dev = _dev()
    A, B, h, w, c = 3, 2, 32, 32, 64
    g = torch.Generator().manual_seed(3)
    feat = torch.randn(A * B, h, w, c, generator=g).clamp_(min=0)
    feat[1 * B + 0, 14, 15, 3] = float("nan")
    feat[1 * B + 0, 16, 12, 7] = float("inf")
    feat[1 * B + 0, 17, 18, 9] = float("-inf")
    feat[2 * B + 1, 10, 10, :] = float("nan")
    px = f64.FRAME_M / w
    shifts = [(0, 0), (1, 0), (-2, 1), (0, -2), (2, 2), (-1, -1)]
    trans = torch.eye(4).repeat(B, A, A, 1, 1)
    for b in range(B):
        for k, (i, j) in enumerate(_pairs(A)):
            sx, sy = shifts[(k + b) % len(shifts)]
            trans[b, i, j] = torch.from_numpy(f64.pose(0.0, sx * px, sy * px))
    live = [3, 3]
    na = torch.tensor(live, dtype=torch.int32, device=dev)
    for m in MODES:
        want = host_fuse_reduce(feat, trans, live, B, A, m)
        got = ops.fuse_reduce(feat.to(dev), trans.to(dev), na, B, A, m).cpu()
        assert bool(torch.isnan(want).any()) and int((want == 0).sum()) > 1000
        assert _same(got, want), m


def test_refusals_and_graph_replay():
    from disconet_amd import ops
    from disconet_amd._lib import DnError
    dev = _dev()
    A, B, h, w = 3, 2, 16, 16
    feat = torch.randn(A * B, h, w, 64, device=dev)
    poses, _ = f64.sweep(h, w)
    trans = poses[40:40 + B * A * A].reshape(B, A, A, 4, 4).contiguous().to(dev)
    na = torch.tensor([3, 2], dtype=torch.int32, device=dev)
    with pytest.raises(DnError, match="multiple of 4"):
        ops.fuse_reduce(torch.zeros(A * B, h, w, 6, device=dev), trans, na, B, A, "sum")
    with pytest.raises(DnError, match="ego range"):
        ops.fuse_reduce(feat, trans, na, B, A, "sum", ego_first=2, ego_count=2)
    with pytest.raises(ValueError):
        ops.fuse_reduce(feat, trans, na, B, A, "v2v")
    lib = ops._lib.load()
    assert lib.dn_fuse_reduce(None, None, None, B, A, h, w, 64, 0, 0, A, 0, None, None) != 0
    assert b"null" in lib.dn_last_error()
    assert lib.dn_fuse_reduce(feat.data_ptr(), trans.data_ptr(), na.data_ptr(), B, A, h, w, 64, 0, 0, A, 3,
                              feat.data_ptr(), None) != 0
    assert b"unknown mode" in lib.dn_last_error()
    # a captured replay equals the eager call
    for m in MODES:
        eager = ops.fuse_reduce(feat, trans, na, B, A, m)
        out = torch.empty_like(eager)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            ops.fuse_reduce(feat, trans, na, B, A, m, out=out)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            ops.fuse_reduce(feat, trans, na, B, A, m, out=out)
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager), m


# ---------------------------------------------------------------------------------------------
# c. the list kernels of the training step
# ---------------------------------------------------------------------------------------------
def _lists(lengths, dev):
    """lists of the given lengths over maps [sum(lengths)]: the images of a list are scattered over the buffer, the outputs
    are written in reverse order"""
    n = sum(lengths)
    g = torch.Generator().manual_seed(n)
    image = torch.randperm(n, generator=g).tolist()
    first = [0]
    for k in lengths:
        first.append(first[-1] + k)
    ego_out = list(range(len(lengths)))[::-1]
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)
    return first, image, ego_out, (i32(first), i32(image), i32(ego_out))


@pytest.mark.parametrize("hw,c", [((8, 8), 64), ((5, 7), 36)])
def test_list_kernels_are_exact(hw, c):
    """forward: torch's sequential adds, that sum / len and torch.max(dim=0) on the same maps, bit for bit; backward rows: dfused, dfused / len
    (torch on the device) and the contract's winner mask; lists of 1, 2, 5 and 16 maps; dfused as a channel slice"""
    from disconet_amd import train_ops as T
    dev = _dev()
    lengths = [1, 2, 5, 16, 1, 3]
    first, image, ego_out, (d_first, d_image, d_out) = _lists(lengths, dev)
    g = torch.Generator().manual_seed(c)
    maps = torch.randn(sum(lengths), hw[0], hw[1], c, generator=g).clamp_(min=-0.5)      # ties at -0.5
    maps[image[first[3] + 4], 2, 3, 1] = float("nan")
    maps[image[first[3] + 9], 2, 3, 1] = float("nan")
    maps = maps.to(dev)
    wide = torch.randn(len(lengths), hw[0], hw[1], c + 12, generator=g).to(dev)
    dfused = wide[..., 8:8 + c]                                                            # ld = c + 12, 16-byte aligned rows
    for m in MODES:
        fused = torch.full((len(lengths),) + tuple(maps.shape[1:]), 7.0, device=dev)
        T.fuse_reduce_lists(maps, d_first, d_image, d_out, m, fused)
        dmaps = torch.full_like(maps, 7.0)
        T.fuse_reduce_lists_backward(dfused, maps, fused, d_first, d_image, d_out, m, dmaps)
        torch.cuda.synchronize()
        for e, n in enumerate(lengths):
            idx = image[first[e]:first[e + 1]]
            stack = maps[idx].cpu()
            if m == "max":
                want = rf.reduce_stack(stack, m)
            else:      # the contract's order, one add after the other (torch.stack(...).sum(0) at a feature map's size)
                want = stack[0].clone()
                for k in range(1, n):
                    want = want + stack[k]
                want = want / float(n) if m == "mean" else want
            assert _same(fused[ego_out[e]].cpu(), want), (m, e)
            if n == 1:
                assert torch.equal(fused[ego_out[e]], maps[idx[0]])
            df = dfused[ego_out[e]]
            if m == "sum":
                rows = [df] * n
            elif m == "mean":
                rows = [df / torch.tensor(float(n), device=dev)] * n
            else:
                win = torch.max(stack, dim=0)[1].to(dev)  # the first index among ties, the first NaN
                rows = [torch.where(win == k, df, torch.zeros_like(df)) for k in range(n)]
            for k, row in zip(idx, rows):
                assert torch.equal(dmaps[k], row), (m, e, k)


def test_more_than_sixteen_maps_in_a_list_still_raise():
    from disconet_amd import train
    from disconet_amd._lib import DnError
    with pytest.raises(DnError, match="at most 16"):
        train.fusion_lists(18, False, torch.eye(4).repeat(1, 18, 18, 1, 1), torch.tensor([18]), 1, torch.device("cpu"))


@pytest.mark.parametrize("h,c", [(16, 64), (32, 256)])
def test_chain_gradient_vs_float64_autograd(h, c):
    """warp_list -> combine -> combine backward -> warp_backward against float64 autograd of the twin's list reduction,
    held to FACTOR * E, E = max |torch fp32 autograd - float64| of the same chain (test_warp_backward_vs_float64_autograd's
    rule).  max: the winner of an element is decided by the warped values, and a kernel's warped value may sit FACTOR * E_w
    from float64 (the bound of the forward tests), so two entries closer than 2 * FACTOR * E_w in float64 may swap places
    and the gradient of that element is not defined by the contract.  The gradient handed in is zero there -- the mask comes
    from the float64 reference, never from the kernel.  What is left out is asserted: at most a quarter of the elements, and
    at least 95 % of them exact ties at zero between the zero padding of two warps (a tap on the frame's edge may be in
    frame in one arithmetic and out in another); measured 10 % / 18 % left out, 99 % / 99.9 % of them such ties."""
    from disconet_amd import train
    from disconet_amd import train_ops as T
    dev = _dev()
    w = h
    A, B, live = 4, 2, [4, 3]
    poses, rigid = f64.sweep(h, w)
    pool = poses[rigid]
    g = torch.Generator().manual_seed(h + c)
    trans = pool[torch.randperm(pool.shape[0], generator=g)[:B * A * A]].reshape(B, A, A, 4, 4).contiguous()
    maps = torch.randn(A * B, c, h, w, generator=g)
    lists = train.fusion_lists(A, False, trans.to(dev), torch.tensor(live), B, dev)
    NI, NW = A * B, lists["n_warps"]
    first, map_image, ego_out = (lists[k].tolist() for k in ("first", "map_image", "ego_out"))
    src, p = lists["src_image"].cpu().long(), lists["poses"].cpu()
    dfused0 = torch.randn(len(ego_out), c, h, w, generator=g)

    def chain(dt, mode, dfused):
        x = maps.detach().to(dt).clone().requires_grad_(True)
        warped = f64.warp_many(x[src], p, dt)
        every = torch.cat([x, warped], 0)
        out = torch.stack([rf.reduce_stack(every[map_image[first[e]:first[e + 1]]], mode) for e in range(len(ego_out))])
        (out[torch.tensor(ego_out).argsort()] * dfused.to(dt)).sum().backward()
        return x.grad, warped.detach(), every.detach()

    _, w64, every64 = chain(torch.float64, "sum", dfused0)
    _, w32, _ = chain(torch.float32, "sum", dfused0)
    E_w = (w32.double() - w64).abs().max().item()
    assert E_w > 0 and int((w64.abs().amax((1, 2, 3)) > 0).sum()) >= 0.6 * NW
    for mode in MODES:
        dfused = dfused0.clone()
        if mode == "max":
            n_all = n_out = n_zero_ties = 0
            for e in range(len(ego_out)):
                n = first[e + 1] - first[e]
                n_all += dfused[ego_out[e]].numel()
                if n > 1:
                    top = every64[map_image[first[e]:first[e + 1]]].topk(2, dim=0)[0]
                    out = (top[0] - top[1]) < 2 * rf.FACTOR * E_w
                    dfused[ego_out[e]][out] = 0.0
                    n_out += int(out.sum())
                    n_zero_ties += int((out & (top[0] == 0) & (top[1] == 0)).sum())
            print("\nchain gradient %dx%dx%d max: %.4f of the elements left out, %.4f of those exact-zero ties"
                  % (h, w, c, n_out / n_all, n_zero_ties / max(n_out, 1)))
            assert n_out <= 0.25 * n_all and n_zero_ties >= 0.95 * n_out
        g64, _, _ = chain(torch.float64, mode, dfused)
        g32, _, _ = chain(torch.float32, mode, dfused)
        E = (g32.double() - g64).abs().max().item()
        buf = torch.empty(NI + NW, h, w, c, device=dev)
        buf[:NI] = rf.nhwc(maps).to(dev)
        T.warp_list(buf, lists["poses"], lists["src_image"], out=buf[NI:])
        fused = torch.empty(len(ego_out), h, w, c, device=dev)
        T.fuse_reduce_lists(buf, lists["first"], lists["map_image"], lists["ego_out"], mode, fused)
        dmaps = torch.empty_like(buf)
        T.fuse_reduce_lists_backward(rf.nhwc(dfused).to(dev), buf, fused, lists["first"], lists["map_image"],
                                     lists["ego_out"], mode, dmaps)
        T.warp_backward(dmaps[NI:], lists["poses"], lists["src_image"], dmaps[:NI], rigid=bool(lists["rigid"]))
        err = (dmaps[:NI].cpu().double() - rf.nhwc(g64)).abs().max().item()
        print("\nchain gradient %dx%dx%d %s: E_w = %.3e, E = %.3e, err = %.3e" % (h, w, c, mode, E_w, E, err))
        assert E > 0 and err <= rf.FACTOR * E, (mode, err, E)


# ---------------------------------------------------------------------------------------------
# d. the models
# ---------------------------------------------------------------------------------------------
_REF = {}


def _ref_outputs(mode, case):
    """the twin and its outputs for a model case, computed once per process"""
    if (mode, case) not in _REF:
        c = cases.MODEL_CASES[case]
        ref = rf.build_reduce_ref(mode, c["map_hw"], c["agents"], kd_flag=1)
        bevs, trans, na = cases.model_inputs(case)
        with torch.no_grad():
            res, x8, x7, x6, x5, fused = ref(bevs, trans, na, c["batch"])
        _REF[(mode, case)] = (ref, {"cls": res["cls"], "loc": res["loc"], "x8": x8, "x5": x5, "fused": fused})
    return _REF[(mode, case)]


def _product(mode, ref, map_hw, agents, math, kd_flag=1):
    from disconet_amd import Config, build_model
    m = build_model(mode, Config(map_hw=map_hw), kd_flag=kd_flag, num_agent=agents).eval()
    m.conv_math = math
    m.load_state_dict({"module." + k: v for k, v in ref.state_dict().items()})
    return m.cuda()


@pytest.mark.parametrize("math", ["f32", "f16x3", "sp"])
@pytest.mark.parametrize("case", ["cfg1_f1", "ragged_a4"])
@pytest.mark.parametrize("mode", MODES)
def test_models_vs_twin(mode, case, math):
    from disconet_amd import MaxFusion, MeanFusion, SumFusion
    c = cases.MODEL_CASES[case]
    ref, want = _ref_outputs(mode, case)
    m = _product(mode, ref, c["map_hw"], c["agents"], math)
    assert type(m) is {"sum": SumFusion, "mean": MeanFusion, "max": MaxFusion}[mode]
    bevs, trans, na = cases.model_inputs(case)
    with torch.no_grad():
        res, x8, x7, x6, x5, fused = m(bevs.cuda(), trans.cuda(), na.cuda(), c["batch"])
    torch.cuda.synchronize()
    got = {"cls": res["cls"].cpu(), "loc": res["loc"].cpu(), "x8": x8.cpu(), "x5": x5.cpu(), "fused": fused.cpu()}
    for name in want:
        assert got[name].shape == want[name].shape, name
        err = (got[name] - want[name]).abs().max().item()
        assert err <= TOL, "%s/%s/%s %s max abs err %.3e" % (mode, case, math, name, err)


def test_kd_flag_zero_returns_the_dict_and_a_graphed_step_replays_the_eager_bits():
    from disconet_amd.graph import GraphedStep
    case = "ragged_a4"
    c = cases.MODEL_CASES[case]
    ref, want = _ref_outputs("max", case)
    m = _product("max", ref, c["map_hw"], c["agents"], "sp", kd_flag=0)
    bevs, trans, na = (t.cuda() for t in cases.model_inputs(case))
    with torch.no_grad():
        eager = m(bevs, trans, na, c["batch"])
        assert isinstance(eager, dict) and set(eager) == {"loc", "cls"}
        assert eager["cls"].shape == want["cls"].shape and eager["loc"].shape == want["loc"].shape
        na32 = na[:, 0].int().contiguous()
        step = GraphedStep(lambda: m(bevs, trans, na32, c["batch"]))
        out = step()
        step.drain()
    assert torch.equal(out["cls"], eager["cls"]) and torch.equal(out["loc"], eager["loc"])


# ---------------------------------------------------------------------------------------------
# e. one training step
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["cfg1", "ragged_a4"])
@pytest.mark.parametrize("mode", ["max", "mean"])
def test_one_training_step_vs_twin(mode, case, monkeypatch):
    """losses within 2e-5 relative of the twin's fp32 step; every gradient under the acceptance rule of
    tests/test_gpu_train_step.py :: _assert_grads, unchanged, against the twin's float64 autograd"""
    from disconet_amd import CoDetModule, Config, build_model
    from oracle.train_ref import train_step
    from tests.test_gpu_train_step import _assert_grads, _fp64_grads, _grad_report
    c = cases.TRAIN_CASES[case]
    (bevs, trans, na), (labels, targets, mask) = cases.train_inputs(case)
    ref = rf.build_reduce_ref(mode, c["map_hw"], c["agents"], kd_flag=0)
    model = build_model(mode, Config(map_hw=c["map_hw"]), kd_flag=0, num_agent=c["agents"])
    model.load_state_dict(ref.state_dict())
    model = model.cuda()
    g64 = _fp64_grads(ref, (bevs, trans, na), (labels, targets, mask), c["batch"], monkeypatch)
    opt = torch.optim.Adam(ref.parameters(), lr=1e-3)
    l_ref = train_step(ref, opt, bevs, trans, na, c["batch"], labels, targets, mask)
    mod = CoDetModule(model, lr=1e-3)
    assert type(mod.engine).__name__ == "ReduceTrainEngine"
    data = {"bev_seq": bevs.cuda(), "trans_matrices": trans.cuda(), "num_agent": na.cuda(),
            "labels": labels.cuda(), "reg_targets": targets.cuda(), "reg_loss_mask": mask.cuda()}
    out = mod.step(data, c["batch"])
    print("\n%s %s: losses %s, twin %s" % (mode, case, out, l_ref))
    assert abs(out["cls_loss"] - l_ref[0]) < 2e-5 * abs(l_ref[0]), (out, l_ref)
    assert abs(out["loc_loss"] - l_ref[1]) < 2e-5 * abs(l_ref[1]), (out, l_ref)
    _assert_grads(_grad_report(g64, ref, mod.engine, model))


def test_training_refuses_distillation_and_an_agent_shard():
    from disconet_amd import CoDetModule, Config, TeacherNet, build_model
    from disconet_amd.sharded import AgentShard
    model = build_model("max", Config(map_hw=128), kd_flag=0, num_agent=2).cuda()
    with pytest.raises(ValueError, match="DiscoGraph"):
        CoDetModule(model, teacher=TeacherNet(Config(map_hw=128)).cuda(), kd_flag=1)
    shard = AgentShard.__new__(AgentShard)      # (never used: the engine refuses before it looks at it)
    with pytest.raises(NotImplementedError):
        CoDetModule(model, shard=shard)


# ---------------------------------------------------------------------------------------------
# f. the tools
# ---------------------------------------------------------------------------------------------
def _run(args, timeout):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable] + args, cwd=root, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def test_tools_train_evaluate_and_track_a_baseline(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    logs = str(tmp_path / "logs")
    out = _run([os.path.join(root, "tools", "det", "train_codet.py"), "--com", "max", "--targets", "boxes", "--num_agent", "2",
                "--batch", "1", "--nepoch", "1", "--steps_per_epoch", "2", "--logpath", logs], 300)
    assert "epoch 1:" in out
    ck = torch.load(os.path.join(logs, "epoch_1.pth"), map_location="cpu", weights_only=False)
    assert not any(k.startswith("pixel_weighted_fusion") for k in ck["model_state_dict"])
    out = _run([os.path.join(root, "tools", "det", "eval_codet.py"), "--com", "max", "--gt", "scene", "--num_agent", "2",
                "--resume", os.path.join(logs, "epoch_1.pth")], 300)
    assert "mAP" in out
    out = _run([os.path.join(root, "tools", "track", "sort_codet.py"), "--com", "sum", "--source", "boxes", "--frames", "8"],
               300)
    assert out.strip()
