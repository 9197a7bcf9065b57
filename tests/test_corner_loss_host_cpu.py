"""The corner localisation loss without a GPU: train_ops.host_corner_loss (the contract of dn_det_loss_corner and the
reference of tests/test_gpu_corner_loss.py) against a hand-written per-anchor loop, its sub-gradient at distance 0, the
freedom of the rotation's sign convention, the case generators' distance bound, the fp32 statement's own error against
float64 (half the GPU tolerance), and the argument checks of the op, of CoDetModule and of the training tool."""
import importlib.util
import math
import os
import sys

import pytest
import torch

from tests import corner_loss_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _corners_of(a, t, flip=False):
    """the four corners of codes t against anchor row a by python floats; flip: the other sign convention of the rotation
    (x = dx cos + dy sin, y = -dx sin + dy cos)"""
    cx, cy = a[0] + t[0] * a[2], a[1] + t[1] * a[3]
    w, h = a[2] * math.exp(t[2]), a[3] * math.exp(t[3])
    s, co = a[4] * t[5] + a[5] * t[4], a[5] * t[5] - a[4] * t[4]
    if flip:
        s = -s
    return [(dx * co - dy * s + cx, dx * s + dy * co + cy)
            for dx, dy in ((-w / 2, -h / 2), (w / 2, -h / 2), (w / 2, h / 2), (-w / 2, h / 2))]


def _loop_loss(c, flip=False):
    """sum_i mask_i sum_k |pc_ik - tc_ik| / norm, one anchor at a time"""
    loc, tgt, mask, anchors = (c[k].double().tolist() for k in ("loc", "targets", "mask", "anchors"))
    total = 0.0
    for i, mk in enumerate(mask):
        if mk == 0:
            continue
        a = anchors[i % len(anchors)]
        total += mk * sum(math.hypot(p[0] - q[0], p[1] - q[1])
                          for p, q in zip(_corners_of(a, loc[i], flip), _corners_of(a, tgt[i], flip)))
    return total / c["norm"]


@pytest.mark.parametrize("name", ["n1", "n7", "n255_3img", "n258_2img", "n256_ones"])
def test_host_statement_equals_the_per_anchor_loop(name):
    c = C.case(name)
    got, _ = C.ref64(name)
    want = _loop_loss(c)
    assert want > 0 and abs(got - want) <= 1e-13 * want, (got, want)


def test_loop_corners_are_the_postprocess_corners():
    """order and rotation of postprocess._corners (which normalises the pair: compared on the targets' unit pairs)"""
    from disconet_amd.postprocess import _corners
    c = C.case("n7")
    a, t = c["anchors"].double(), c["targets"].double()
    box = torch.stack([a[:, 0] + t[:, 0] * a[:, 2], a[:, 1] + t[:, 1] * a[:, 3], a[:, 2] * torch.exp(t[:, 2]),
                       a[:, 3] * torch.exp(t[:, 3]), a[:, 4] * t[:, 5] + a[:, 5] * t[:, 4],
                       a[:, 5] * t[:, 5] - a[:, 4] * t[:, 4]], 1)
    want = torch.from_numpy(_corners(box.numpy()))
    got = torch.tensor([_corners_of(a[i].tolist(), t[i].tolist()) for i in range(7)], dtype=torch.float64)
    assert float((got - want).abs().max()) < 1e-6          # (the targets' pairs are unit to fp32 rounding)
    assert float((torch.tensor([_corners_of(a[i].tolist(), t[i].tolist(), True) for i in range(7)]) - want).abs().max()) > 0.1


def test_swapping_the_rotation_sign_leaves_the_value_unchanged():
    """The other sign convention (x = dx cos + dy sin, y = -dx sin + dy cos: the pair read clockwise) is the description of
    the same boxes in the frame with y pointing the other way: with the centres' y mirrored along with it (anchor y and
    code 1 negated, in the prediction and the target alike) every corner is the mirror image of a corner of the original
    pair of boxes -- (dx, dy) lands where (dx, -dy) was, for both boxes -- so the sum of the four distances is the same
    number.  That is why the convention (counter-clockwise, postprocess._corners') is free as far as the loss goes.
    (Negating sin alone, in an unmirrored frame, is NOT a change of convention: it moves each box's corners about its own
    centre while the offset between the centres stays, and the value changes -- asserted too.)"""
    for name in ("n7", "n257", "n4098_3img"):
        c = C.case(name)
        m = dict(c)
        for k in ("loc", "targets", "anchors"):
            m[k] = c[k].clone()
            m[k][:, 1] = -m[k][:, 1]
        a, b = _loop_loss(c), _loop_loss(m, flip=True)
        assert abs(a - b) <= 1e-12 * a, (name, a, b)
        assert abs(C.ref64(name)[0] - b) <= 1e-12 * a
        assert abs(_loop_loss(c, flip=True) - a) > 1e-4 * a


def test_zero_distance_rows_give_zero_gradient_and_no_nan():
    for name, dtype in (("n257", torch.float64), ("n258_2img", torch.float32), ("long", torch.float64)):
        c = C.case(name)
        assert len(c["exact"]) > 0 and torch.equal(c["loc"][c["exact"]], c["targets"][c["exact"]])
        loss, g = C.corner_ref(c, dtype)
        assert math.isfinite(loss) and bool(torch.isfinite(g).all())
        assert float(g[c["exact"]].abs().max()) == 0.0
        assert float(g[c["mask"] == 0].abs().max() if bool((c["mask"] == 0).any()) else 0.0) == 0.0
        assert float(g.abs().max()) > 0
    # all four corners coincide for ONE anchor among others, and a batch of nothing but such anchors
    c = dict(C.case("n7"))
    c["loc"] = c["targets"].clone()
    c["mask"] = torch.ones(7)
    loss, g = C.corner_ref(c)
    assert loss == 0.0 and float(g.abs().max()) == 0.0


def test_unmasked_rows_are_never_touched():
    """NaN / inf in the loc / targets of unmasked anchors, and in anchor rows no masked anchor uses: value and gradient
    unchanged (boolean indexing, as upstream)"""
    c = dict(C.case("n4099"))
    loss0, g0 = C.corner_ref(c)
    off = c["mask"] == 0
    assert bool(off.any())
    for k, bad in (("loc", float("nan")), ("targets", float("inf")), ("anchors", float("nan"))):
        c[k] = c[k].clone()
        c[k][off] = bad                                                      # (per_image == n here: anchor row i is anchor i's)
    loss1, g1 = C.corner_ref(c)
    assert loss1 == loss0 and torch.equal(g1, g0)
    m0 = dict(C.case("n256_zeros"))
    loss, g = C.corner_ref(m0)
    assert loss == 0.0 and float(g.abs().max()) == 0.0


def test_generated_cases_respect_the_distance_bound_and_mix_the_anchors():
    for name in list(C.SMALL_CASES) + ["long"]:
        c = C.case(name)
        n, per = c["loc"].shape[0], c["anchors"].shape[0]
        m = c["mask"] != 0
        rows = c["anchors"][torch.arange(n) % per]
        d = C.corner_distances64(c["loc"], c["targets"], rows)[m]
        assert bool(((d == 0) | (d >= C.MIN_DIST)).all()), name
        pair = c["targets"][:, 4:].double()
        assert float((pair.norm(dim=1) - 1).abs().max()) < 1e-6
    c = C.case("long")
    assert sorted(set(c["anchors"][:, 2].tolist())) == [2.0, 3.0]                # both sizes
    assert len(set((c["anchors"][:, 4] * 1000).round().tolist())) == 3          # the three yaws
    assert float(c["anchors"][:, 0].abs().max()) > 31.0
    assert 0.005 < float(c["mask"].mean()) < 0.02
    assert C.takes_float4_path(C.LONG_N) and not C.takes_float4_path(4099) and not C.takes_float4_path(4098, 16, 4)


def test_fp32_host_statement_stays_within_half_the_tolerance():
    """the fp32 torch statement against float64 on every generated case: value within half of LOSS_RTOL, gradient within half
    of GRAD_TOL of the largest |gradient| -- what entitles the GPU test to hold the kernel to the full tolerances.  (If this
    fails for a new case, raise corner_loss_cases.MIN_DIST, not the tolerance.)"""
    worst = 0.0
    for name in list(C.SMALL_CASES) + ["long"]:
        c = C.case(name)
        l64, g64 = C.ref64(name)
        l32, g32 = C.corner_ref(c, torch.float32)
        gmax = float(g64.abs().max())
        if gmax == 0.0:
            assert l32 == 0.0 and float(g32.abs().max()) == 0.0
            continue
        e = float((g32 - g64).abs().max()) / gmax
        print("%-12s loss rel err %.3g  grad err / max |grad| %.3g  (max |grad| %.4g)" % (name, abs(l32 - l64) / l64, e, gmax))
        worst = max(worst, e)
        assert abs(l32 - l64) <= 0.5 * C.LOSS_RTOL * l64, name
        assert e <= 0.5 * C.GRAD_TOL, (name, e)
    assert worst > 0


def test_op_argument_checks():
    from disconet_amd import train_ops
    c = C.case("n7")
    args = [c[k] for k in ("cls", "labels", "loc", "targets", "mask", "anchors")]
    with pytest.raises(ValueError, match="GPU"):
        train_ops.det_loss_corner(*args, norm=1.0)
    with pytest.raises(ValueError, match="whole number of images"):
        train_ops.host_corner_loss(c["loc"], c["targets"], c["mask"], c["anchors"][:3], 1.0)
    with pytest.raises(ValueError, match="anchors must be"):
        train_ops.host_corner_loss(c["loc"], c["targets"], c["mask"], c["anchors"][:, :5], 1.0)
    # [H, W, A, 6] is taken as its rows
    a4 = c["anchors"].reshape(1, 7, 1, 6)
    assert float(train_ops.host_corner_loss(c["loc"], c["targets"], c["mask"], a4, 1.0)) == \
        float(train_ops.host_corner_loss(c["loc"], c["targets"], c["mask"], c["anchors"], 1.0))


def test_library_exports_the_entry_point():
    from disconet_amd import _lib
    lib = _lib.load()
    assert lib.dn_version() >= 150
    assert hasattr(lib, "dn_det_loss_corner")
    # argument errors are reported before anything is launched
    assert lib.dn_det_loss_corner(None, None, None, None, None, None, 1, 1, 0.25, 2.0, 1.0, None, None, None, None) != 0


class _Cfg:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def test_codet_module_reads_the_loss_type_before_it_builds_anything():
    """the checks run before the engine is built: no model and no GPU are needed to see them"""
    from disconet_amd import CoDetModule, Config
    with pytest.raises(ValueError, match="'faf_loss' / 'corner_loss'"):
        CoDetModule(None, config=Config(loss_type="smooth"))
    with pytest.raises(NotImplementedError, match="code_type"):
        CoDetModule(None, config=Config(loss_type="corner_loss", code_type="corner_1"))
    assert Config().loss_type == "faf_loss"
    # data["anchors"]: required, [H, W, A, 6] or that with a leading image dimension of copies
    loc = torch.zeros(2, 4, 4, 6, 1, 6)
    with pytest.raises(KeyError, match="anchors"):
        CoDetModule._corner_anchors({}, loc)
    a = torch.arange(4 * 4 * 6 * 6, dtype=torch.float64).reshape(4, 4, 6, 6)
    rows = CoDetModule._corner_anchors({"anchors": a}, loc)
    assert rows.shape == (96, 6) and rows.dtype == torch.float32 and torch.equal(rows, a.reshape(96, 6).float())
    assert torch.equal(CoDetModule._corner_anchors({"anchors": torch.stack([a, a])}, loc), rows)
    with pytest.raises(ValueError, match="anchor rows"):
        CoDetModule._corner_anchors({"anchors": a[:3]}, loc)


def _tool():
    here = os.path.join(ROOT, "tools", "det")
    if here not in sys.path:
        sys.path.insert(0, here)
    spec = importlib.util.spec_from_file_location("train_codet_corner", os.path.join(here, "train_codet.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_train_tool_loss_type_flag():
    t = _tool()
    assert t.parse_args(["--com", "disco"]).loss_type == "faf_loss"
    assert t.parse_args(["--loss_type", "corner_loss"]).loss_type == "corner_loss"
    with pytest.raises(SystemExit):
        t.parse_args(["--loss_type", "nonsense"])
    # the anchors ride in data["anchors"] when the tool hands them in, and nothing else changes
    args = t.parse_args(["--batch", "1", "--num_agent", "2"])
    anchors = torch.zeros(32, 32, 6, 6)
    d0 = t.step_data(args, 2, 32, epoch=1, it=0, device="cpu")
    d1 = t.step_data(args, 2, 32, epoch=1, it=0, anchors=anchors, device="cpu")
    assert sorted(d1) == sorted(list(d0) + ["anchors"]) and d1["anchors"] is anchors
    assert all(torch.equal(d0[k], d1[k]) for k in d0)
