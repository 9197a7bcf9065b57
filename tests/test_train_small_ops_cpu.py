"""Pins tests/train_small_ops.py -- the float64 references and the case generators the GPU tests of the small
training kernels share -- without a GPU: the Adam restatement against torch.optim.Adam, the saturation sweep against the
float64 oracle, every "above the cap" case against its cap, the special values of the pool maps."""
import math

import pytest
import torch

from tests import train_small_ops as T


@pytest.mark.parametrize("wd", [0.0, 1e-4, 0.3])
def test_adam64_is_torch_adam_in_float64(wd):
    """1e-12 of each entry (torch forms m by lerp and v by addcmul: other orders of the same float64 operations)"""
    p, g, m, v = (t[:4096].double() for t in T.adam_case())
    for step, (m0, v0), eps in ((1, (torch.zeros_like(m), torch.zeros_like(v)), 1e-8), (2, (m, v), 1e-3), (5000, (m, v), 1e-8)):
        want = T.adam_torch(p, g, m0, v0, step, lr=1e-3, betas=(0.9, 0.999), eps=eps, weight_decay=wd)
        got = T.adam64(p, g, m0, v0, step, lr=1e-3, betas=(0.9, 0.999), eps=eps, weight_decay=wd)
        for a, b in zip(got, want):
            assert a.dtype == b.dtype == torch.float64
            assert bool(((a - b).abs() <= 1e-12 * b.abs() + 1e-300).all()), (step, wd)
    got = T.adam64(p, g, m, v, 7, lr=3e-3, betas=(0.8, 0.95), eps=1e-6, weight_decay=wd)
    want = T.adam_torch(p, g, m, v, 7, lr=3e-3, betas=(0.8, 0.95), eps=1e-6, weight_decay=wd)
    for a, b in zip(got, want):
        assert bool(((a - b).abs() <= 1e-12 * b.abs() + 1e-300).all())


def test_adam_case_mixes_the_gradient_kinds_and_runs_a_partial_last_pass():
    p, g, m, v = T.adam_case()
    assert T.ADAM_N > T.ADAM_CAP and T.ADAM_N % T.ADAM_CAP not in (0,) and T.ADAM_N < 2 * T.ADAM_CAP
    assert p.dtype == g.dtype == m.dtype == v.dtype == torch.float32
    zero = g == 0
    assert int(zero.sum()) > 1000 and bool((v[zero] == 0).all()) and bool((m[zero] == 0).all())
    tiny = g == 1e-20
    assert int(tiny.sum()) > 1000 and float((g[tiny] * g[tiny]).max()) < T.F32_MIN_NORMAL      # the square underflows
    assert int((g == 1e15).sum()) > 1000 and int((g == -1e15).sum()) > 1000
    assert bool(torch.isfinite(T.adam_grad(g, 3) ** 2).all())
    # every kind above the first pass of the capped grid too
    for sel in (zero, tiny, g == 1e15, g == -1e15):
        assert bool(sel[T.ADAM_CAP:].any())


def test_adam_update_bound_is_four_times_the_measured_float32_deviation():
    """re-measures ADAM_UPDATE_DEV_MEASURED: torch's float32 CPU Adam against adam64 over the GPU test's cases"""
    p, g, m, v = T.adam_case()
    worst = 0.0
    for wd, eps in T.ADAM_GRID:
        state = (p, torch.zeros_like(m), torch.zeros_like(v))
        for step in T.ADAM_STEPS:
            if step == 5000:
                state = (p, m, v)
            gs = T.adam_grad(g, step)
            p64, _, _ = T.adam64(*((state[0], gs) + state[1:]), step, eps=eps, weight_decay=wd)
            p32, m32, v32 = T.adam_torch(*((state[0], gs) + state[1:]), step, eps=eps, weight_decay=wd)
            worst = max(worst, float(((p32.double() - state[0].double()) - (p64 - state[0].double())).abs().max()))
            state = (p32, m32, v32)
    assert 0.5 * T.ADAM_UPDATE_DEV_MEASURED <= worst <= T.ADAM_UPDATE_DEV_MEASURED, worst
    assert T.ADAM_UPDATE_BOUND == 4 * T.ADAM_UPDATE_DEV_MEASURED


def test_adam_moment_bounds_hold_for_float32_arithmetic_and_catch_a_wrong_beta():
    """the derived m / v bounds: torch's float32 Adam sits inside them, betas off by 1e-6 do not"""
    p, g, m, v = T.adam_case()
    for wd in (0.0, 1e-4):
        _, m64, v64 = T.adam64(p, g, m, v, 5000, weight_decay=wd)
        _, m32, v32 = T.adam_torch(p, g, m, v, 5000, weight_decay=wd)
        bm, bv = T.adam_mv_bounds(p, g, m, v, (0.9, 0.999), wd)
        assert bool(((m32.double() - m64).abs() <= bm).all()) and bool(((v32.double() - v64).abs() <= bv).all())
        _, mb, vb = T.adam_torch(p, g, m, v, 5000, betas=(0.9 + 1e-6, 0.999 - 1e-6), weight_decay=wd)
        assert not bool(((mb.double() - m64).abs() <= bm).all()) and not bool(((vb.double() - v64).abs() <= bv).all())


@pytest.mark.parametrize("fg", [False, True])
def test_sweep_generator_and_the_float64_oracle_on_it(fg):
    assert T.GAPS[0] == 0 and max(g for g in T.GAPS if g < 1e3) == 120 and T.GAPS[-1] == 1e4 and len(T.GAPS) >= 12
    assert any(69 < g <= 70 for g in T.GAPS) and any(g == 104 for g in T.GAPS)
    for gap in T.GAPS:
        cls, labels, loc, targets, mask = T.sweep_case(gap, fg)
        t = 1 if fg else 0
        assert cls.dtype == torch.float32 and tuple(cls.shape) == (4, 2)
        # the intended gaps, exactly, in float32 and on the intended class
        assert torch.equal((cls[:, 1 - t] - cls[:, t]).double(), torch.tensor(T.SWEEP_SIGNS, dtype=torch.float64) * gap)
        assert bool((labels[:, t] == 1).all()) and bool((labels[:, 1 - t] == 0).all())
        for alpha, gamma in ((0.25, 2.0), (0.5, 1.0), (0.25, 0.0)):
            l_cls, l_loc, dcls, dloc = T.det_ref(cls, labels, loc, targets, mask, 2.0, alpha, gamma, 3.0)
            assert math.isfinite(l_cls) and math.isfinite(l_loc) and bool(torch.isfinite(dcls).all())
            scale = T.focal_grad_scale(labels, alpha, 2.0)
            assert torch.equal(scale, torch.full((4,), (alpha if fg else 1 - alpha) / 2.0, dtype=torch.float64))
            assert bool((dcls.sum(1).abs() <= 1e-15).all())                      # d/dz_other = -d/dz_t
            if gap >= 60:
                wrong = torch.tensor(T.SWEEP_SIGNS) > 0
                # |d/dz_t| -> a_t / norm on the wrong side, -> 0 on the right side; the loss grows like a_t * gap
                assert bool(((dcls[wrong, t] + scale[wrong]).abs() <= 1e-12 * scale[wrong]).all()), (gap, gamma)
                assert bool((dcls[~wrong, t].abs() <= 1e-20).all())
                assert abs(l_cls - 2 * gap * float(scale[0])) <= 1e-12 * l_cls


def test_dispatch_rule_of_the_sweep_calls():
    """what the GPU sweep relies on to reach both kernels: 4 anchors take the float4 path for code 6 and 7 when aligned,
    the scalar path from an 8-byte-offset view, with an odd count, and with code 7 at an even count of 6"""
    for code in (6, 7):
        assert T.det_takes_float4_path(4, code, 0, 16, 256)
        assert not T.det_takes_float4_path(4, code, 8, 16)
        assert not T.det_takes_float4_path(5, code, 0)
    assert not T.det_takes_float4_path(6, 7, 0) and T.det_takes_float4_path(6, 6, 0)
    v = T.unaligned_copy(torch.arange(8.0).view(4, 2))
    assert v.data_ptr() % 16 == 8 and torch.equal(v, torch.arange(8.0).view(4, 2))


@pytest.mark.parametrize("sigma", [1.0, 3.0])
@pytest.mark.parametrize("code", [6, 7])
def test_smooth_l1_edge_case_holds_the_threshold_and_its_neighbours(sigma, code):
    for big in (False, True):
        cls, labels, loc, targets, mask = T.smooth_l1_edge_case(sigma, code, big)
        n = loc.shape[0]
        assert n % 4 == 0 and tuple(cls.shape) == (n, 2) and mask.numel() == n and float(targets.abs().max()) == 0
        t = torch.tensor(1.0 / (sigma * sigma), dtype=torch.float32)
        live = loc[mask == 1].flatten()
        dead = loc[mask == 0].flatten()
        for s in (1.0, -1.0):
            for v in (s * t, s * torch.nextafter(t, torch.tensor(float("inf"))), s * torch.nextafter(t, torch.tensor(float("-inf")))):
                assert bool((live == v).any()) and bool((dead == v).any())
        assert bool((live == 0).any()) and bool(((live == 0) & torch.signbit(live)).any())
        assert bool((live.abs() == 1e6).any()) == big
        assert bool((labels.sum(1) == 0).any())                       # a "don't care" row
        l_cls, l_loc, dcls, dloc = T.det_ref(cls, labels, loc, targets, mask, 2.0, 0.25, 2.0, sigma)
        assert math.isfinite(l_loc) and bool((dloc[mask == 0] == 0).all())
        assert float(dloc.abs().max()) <= 0.5 + 1e-12                 # |g| <= 1, / norm


def test_long_detection_case():
    cls, labels, loc, targets, mask, sat = T.long_det_case()
    n, code = T.LONG_DET_N, 6
    assert n == 786432 and tuple(cls.shape) == (n, 2) and tuple(loc.shape) == (n, code)
    assert n * code // 4 > T.DET_V4_CAP             # loop B of the float4 kernel iterates
    assert n > T.DET_SCALAR_CAP                     # the scalar kernel's loop iterates
    assert T.det_takes_float4_path(n, code, 0) and not T.det_takes_float4_path(n, code, 8)
    fg = labels[:, 1] > 0.5
    ignored = labels.sum(1) == 0
    assert 0.04 * n < int(fg.sum()) < 0.06 * n and 0.015 * n < int(ignored.sum()) < 0.025 * n
    assert bool(fg[T.DET_SCALAR_CAP:].any()) and bool(ignored[T.DET_SCALAR_CAP:].any())
    assert 0.008 * n < sat.numel() < 0.012 * n
    gaps = (cls[sat, 1] - cls[sat, 0]).abs()
    for gp in (70.0, 104.0, 120.0, 1e4):            # the drawn gaps survive float32 on top of a randn * 3 logit
        assert bool(((gaps - gp).abs() <= 1e-3 * gp).any())
    wrong = (cls[:, 1] - cls[:, 0]) * torch.where(fg, -1.0, 1.0)
    assert int(((wrong > 69.1) & ~ignored).sum()) > 500          # anchors the clamped form got wrong


def test_kd_cases_and_reference():
    for c in (1, 8, 32, 100, 512):
        s, t = T.kd_case(12, c, seed=c)
        term, d = T.kd_ref(s, t, 1e5)
        assert math.isfinite(term) and term >= 0 and bool(torch.isfinite(d).all())
        if c > 1:
            assert float(s[0].max() - s[0].sort().values[-2]) > 180 and float(t[1].max() - t[1].sort().values[-2]) > 180
            assert int((torch.softmax(t[1], 0) == 0).sum()) == c - 1      # float32 teacher probabilities underflow to 0
            # xlogy semantics: those terms are 0, the gradient is still (softmax(s) - softmax(t)) * scale
            want = (torch.softmax(s[1].double(), 0) - torch.softmax(t[1].double(), 0)) * 1e5 / (12 * c)
            assert float((d[1] - want).abs().max()) <= 1e-12 * float(want.abs().max())
        assert float(s[4].max() - s[4].min()) == 0 and float(t[5].max() - t[5].min()) == 0
        half, _ = T.kd_ref(s, t, 1e5, norm_rows=24)
        assert abs(half - term / 2) <= 1e-12 * term + 1e-300
    assert 33800 > T.KD_ROWS_CAP


def test_seg_cases():
    assert math.prod(T.SEG_PIXELS) == 600000 > T.SEG_CE_CAP > T.SEG_COUNT_CAP
    for classes in (1, 5, 8, 19):
        z, y = T.seg_case(classes, shape=(1, 40, 100))
        assert tuple(z.shape) == (1, 40, 100, classes) and y.dtype == torch.int64
        frac = float((y == -100).float().mean())
        assert 0.25 < frac < 0.35
        assert bool(((y >= 0) & (y < classes) | (y == -100)).all())
        gap = z.view(-1, classes).max(1).values - z.view(-1, classes).min(1).values
        if classes > 1:
            assert int((gap > 9000).sum()) >= 8
        loss, grad = T.seg_ref(z, y)
        assert math.isfinite(loss) and bool((grad[y == -100] == 0).all())


def test_resample_cases_exceed_the_cap_per_batch_and_not_per_image():
    """the shapes tests/test_gpu_resample_fp64.py launches whole and image by image; items as the launch code counts them"""
    from tests.test_gpu_resample_fp64 import BIG
    items = {
        "maxpool2": lambda n, h, w, c: n * (h // 2) * (w // 2) * (c // 4),             # seg_ops.hip :: dn_maxpool2_nhwc
        "maxpool2_backward": lambda n, h, w, c: n * (h // 2) * (w // 2) * (c // 4),    # dn_maxpool2_nhwc_backward
        "upsample2_bilinear": lambda n, h, w, c: n * (2 * h) * (2 * w) * (c // 4),     # dn_upsample2_bilinear_nhwc
        "upsample2_bilinear_backward": lambda n, h, w, c: n * h * w * (c // 4),        # dn_upsample2_bilinear_nhwc_backward
        "sp_maxpool2": lambda n, h, w, c: n * ((c + 15) // 16) * 2 * (h // 2) * (w // 2),     # dn_sp_maxpool2
        "sp_upsample2_bilinear": lambda n, h, w, c: n * ((c + 15) // 16) * 2 * (2 * h) * (2 * w),   # dn_sp_upsample2_bilinear
    }
    assert set(BIG) == set(items)
    for name, (n, h, w, c) in BIG.items():
        assert items[name](n, h, w, c) > T.RESAMPLE_CAP, name
        assert items[name](1, h, w, c) < T.RESAMPLE_CAP, name
    for h, w in ((1, 1), (1, 33), (64, 1), (31, 7), (64, 33)):
        assert (h, w) in T.UPSAMPLE_SIZES
    assert len(T.UPSAMPLE_SIZES) == 28


def test_elementwise_cases_exceed_the_cap():
    from tests.test_gpu_elementwise_fp64 import BIG
    assert set(BIG) == {"upsample2_sum", "add_rows", "pair_add_ego", "pair_sum_ego"}
    for name, shape in BIG.items():
        assert math.prod(shape) > T.ELEMENTWISE_CAP, name        # elements of the tensor the kernel's loop runs over


def test_pool_special_map_and_the_documented_rule():
    wins = dict(T.pool_special_windows())
    for name, s in T.POOL_SPECIALS.items():
        for pos in range(4):
            v = wins["%s@%d" % (name, pos)][pos]
            assert (math.isnan(v) and math.isnan(s)) or v == s
    x = T.pool_special_map(8)
    n, h, w, c = x.shape
    win = x.view(n, h // 2, 2, w // 2, 2, c).permute(0, 1, 3, 5, 2, 4).reshape(-1, c, 4)
    for ch in range(c):                 # every channel (so every lane of a float4) meets every special at every position
        for pos in range(4):
            col = win[:, ch, pos]
            assert bool(torch.isnan(col).any()) and bool((col == float("inf")).any()) and bool((col == float("-inf")).any())
            assert bool(((col == 0) & torch.signbit(col)).any()) and bool(((col == 0) & ~torch.signbit(col)).any())
        assert bool((win[:, ch].max(1).values == win[:, ch].min(1).values).any())       # all-equal windows
    # ATen on the CPU follows the documented rule, values and routing, bit for bit
    y_rule, arg = T.maxpool_rule(x)
    dy = torch.randn(y_rule.shape, generator=torch.Generator().manual_seed(1))
    y, dx = T.maxpool_aten(x, dy)
    assert torch.equal(T.bits(y), T.bits(y_rule))
    want = torch.zeros(n, h // 2, w // 2, c, 4)
    want.scatter_(-1, arg.unsqueeze(-1), dy.unsqueeze(-1))
    want = want.view(n, h // 2, w // 2, c, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(n, h, w, c)
    assert torch.equal(T.bits(dx), T.bits(want))
    assert bool((arg == 3).any()) and bool((arg == 0).any())


def test_upsample_reference_conserves_the_gradient():
    for h, w in ((1, 1), (3, 7), (5, 2)):
        x = torch.randn(2, h, w, 4)
        y, dx = T.upsample_ref(x, torch.ones(2, 2 * h, 2 * w, 4))
        assert tuple(y.shape) == (2, 2 * h, 2 * w, 4)
        assert float((dx.sum((1, 2)) - 4 * h * w).abs().max()) <= 1e-12 * 4 * h * w


@pytest.mark.parametrize("c", [64, 512])
def test_fuse_case_and_reference(c):
    z4, maps, dfused = T.fuse_case(c)
    assert sorted(len(l) for l in T.FUSE_LISTS) == [1, 2, 6]
    used = [m for l in T.FUSE_LISTS for _, m in l]
    assert len(set(used)) == len(used) and set(range(T.FUSE_MAPS)) - set(used) == {9}
    pairs = sorted(p for l in T.FUSE_LISTS for p, _ in l if p >= 0)
    assert pairs == list(range(8)) == list(range(z4.shape[0]))
    assert all(len(l) == 1 for l in T.FUSE_LISTS if any(p < 0 for p, _ in l))
    assert (len(T.FUSE_LISTS) * T.FUSE_HW[0] * T.FUSE_HW[1]) % 4 != 0
    assert bool((z4 == 0).any()) and bool((z4 == 80).any()) and bool((z4 < 0).any())
    outs, wts, dmaps, dz4 = T.fuse_combine_ref(z4, maps, T.FUSE_LISTS, T.FUSE_EGO_OUT, dfused)
    assert bool((dz4[z4 <= 0] == 0).all()) and float(dmaps[9].abs().max()) == 0
    assert torch.equal(outs[0], maps[0].double())                                  # a list of one: the map itself
    for wk in wts:
        assert float((wk.sum(0) - 1).abs().max()) <= 1e-12
    assert bool(torch.isfinite(dz4).all()) and float(dz4.abs().max()) > 0
