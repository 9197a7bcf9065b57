"""dn_det_loss_corner (train_ops.det_loss_corner: focal + corner localisation loss, both kernel forms) against
train_ops.host_corner_loss in float64 under autograd on the same fp32 inputs, and CoDetModule with
Config(loss_type="corner_loss") end to end.

Tolerances are dn_det_loss' (tests/test_gpu_det_loss_fp64.py): 1e-5 relative on each loss, 2e-5 of the largest
|gradient| on dloc.  The cases (tests/corner_loss_cases.py) keep every non-zero corner distance of a masked anchor above
5 mm, where the fp32 torch statement itself stays within half of that (tests/test_corner_loss_host_cpu.py)."""
import functools

import pytest
import torch

from tests import corner_loss_cases as C
from tests import train_small_ops as T

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _run(c, unaligned=False, **over):
    """-> (losses [2] float64 cpu, dcls cpu, dloc cpu, took the float4 path?)"""
    from disconet_amd import train_ops
    t = {k: over.get(k, c[k]).to(DEV) for k in ("cls", "labels", "loc", "targets", "mask", "anchors")}
    if unaligned:
        t["cls"], t["loc"] = C.offset_copy(t["cls"]), C.offset_copy(t["loc"])
    v4 = C.takes_float4_path(t["loc"].shape[0], *(t[k].data_ptr() for k in ("cls", "labels", "loc", "targets")))
    losses, dcls, dloc = train_ops.det_loss_corner(t["cls"], t["labels"], t["loc"], t["targets"], t["mask"], t["anchors"],
                                                   norm=c["norm"], alpha=C.ALPHA, gamma=C.GAMMA)
    return losses.cpu(), dcls.cpu(), dloc.cpu(), v4


@functools.lru_cache(maxsize=None)
def _cls_ref(name):
    """the focal loss of the case in float64 (oracle.train_ref.det_loss, as tests/test_gpu_det_loss_fp64.py takes it)"""
    c = C.case(name)
    return T.det_ref(c["cls"], c["labels"], c["loc"], c["targets"], c["mask"], c["norm"], C.ALPHA, C.GAMMA, 3.0)[0]


def _check(got, name, what):
    losses, dcls, dloc, _ = got
    c = C.case(name)
    l_loc, rl = C.ref64(name)
    l_cls = _cls_ref(name)
    gmax = float(rl.abs().max())
    err = float((dloc.double() - rl).abs().max())
    print("%s %s: losses got %.9g %.9g ref %.9g %.9g; dloc err %.3g of max |grad| %.4g = %.3g"
          % (name, what, float(losses[0]), float(losses[1]), l_cls, l_loc, err, gmax, err / gmax if gmax else 0.0))
    assert abs(float(losses[0]) - l_cls) <= C.LOSS_RTOL * abs(l_cls), (name, what)
    assert abs(float(losses[1]) - l_loc) <= C.LOSS_RTOL * abs(l_loc), (name, what)
    assert err <= C.GRAD_TOL * gmax, (name, what, err, gmax)
    off = c["mask"] == 0
    if bool(off.any()):
        assert bool((C.bits(dloc[off]) == 0).all()), (name, what)             # unmasked rows: all zero BITS
    if len(c["exact"]):
        assert float(dloc[c["exact"]].abs().max()) == 0.0, (name, what)       # loc == targets bitwise: exactly zero rows


@pytest.mark.parametrize("name", list(C.SMALL_CASES))
def test_value_and_gradients_match_float64_in_both_forms(name):
    """every small case as it stands (even n: the float4 streams, odd n: a lane per anchor) and from one-float-offset views
    of cls / loc (always a lane per anchor); dcls / dloc of the two runs bit for bit, and of a second call"""
    from disconet_amd import train_ops
    c = C.case(name)
    n = c["loc"].shape[0]
    a = _run(c)
    b = _run(c, unaligned=True)
    assert a[3] == (n % 2 == 0) and not b[3]
    _check(a, name, "float4" if a[3] else "scalar")
    _check(b, name, "scalar, offset views")
    assert torch.equal(C.bits(a[1]), C.bits(b[1])) and torch.equal(C.bits(a[2]), C.bits(b[2]))
    again = _run(c)
    assert torch.equal(C.bits(a[1]), C.bits(again[1])) and torch.equal(C.bits(a[2]), C.bits(again[2]))
    # the classification half is dn_det_loss': dcls bit for bit, the value to the order of the sums
    t = {k: c[k].to(DEV) for k in ("cls", "labels", "loc", "targets", "mask")}
    l0, dcls0, _ = train_ops.det_loss(t["cls"], t["labels"], t["loc"], t["targets"], t["mask"], norm=c["norm"], alpha=C.ALPHA,
                                      gamma=C.GAMMA)
    assert torch.equal(C.bits(dcls0.cpu()), C.bits(a[1]))
    assert abs(float(l0[0]) - float(a[0][0])) <= 1e-12 * abs(float(l0[0]))


def test_mask_all_zero_and_all_one():
    for name in ("n256_zeros", "n255_zeros"):
        losses, dcls, dloc, _ = _run(C.case(name))
        assert float(losses[1]) == 0.0 and bool((C.bits(dloc) == 0).all())
        assert float(losses[0]) > 0 and float(dcls.abs().max()) > 0
    c = C.case("n256_ones")
    losses, _, dloc, v4 = _run(c)
    assert v4 and bool((dloc.abs().max(1).values > 0).all())


def test_long_input_both_kernels():
    """700 002 anchors in three images, 1 % masked: 1 050 003 float4s of dloc against the float4 kernel's 1 048 576 threads and
    700 002 anchors against the per-anchor kernel's 524 288 -- both grid-stride loops iterate"""
    c = C.case("long")
    a = _run(c)
    b = _run(c, unaligned=True)
    assert a[3] and not b[3]
    _check(a, "long", "float4")
    _check(b, "long", "scalar")
    assert torch.equal(C.bits(a[1]), C.bits(b[1])) and torch.equal(C.bits(a[2]), C.bits(b[2]))
    assert float((a[0] - b[0]).abs().max()) <= 1e-12 * float(a[0].abs().max())


@pytest.mark.parametrize("name", ["n4099", "n4098_3img"])
def test_non_finite_values_of_unmasked_anchors_reach_nothing(name):
    """NaN / inf in loc and targets of unmasked anchors (and NaN in the anchor rows that no masked anchor uses): every output
    finite and bit for bit the clean run's -- those rows are not read"""
    c = C.case(name)
    n, per = c["loc"].shape[0], c["anchors"].shape[0]
    off = c["mask"] == 0
    loc, targets, anchors = c["loc"].clone(), c["targets"].clone(), c["anchors"].clone()
    loc[off] = float("nan")
    targets[off] = float("inf")
    targets[off.nonzero().flatten()[::2]] = float("nan")
    unused = torch.ones(per, dtype=torch.bool)
    unused[(~off).nonzero().flatten() % per] = False
    assert bool(unused.any())
    anchors[unused] = float("nan")
    for unaligned in (False, True):
        clean = _run(c, unaligned)
        dirty = _run(c, unaligned, loc=loc, targets=targets, anchors=anchors)
        assert clean[3] == dirty[3] == (n % 2 == 0 and not unaligned)
        assert all(bool(torch.isfinite(x).all()) for x in dirty[:3])
        assert torch.equal(C.bits(clean[1]), C.bits(dirty[1])) and torch.equal(C.bits(clean[2]), C.bits(dirty[2]))
        assert abs(float(clean[0][1]) - float(dirty[0][1])) <= 1e-12 * float(clean[0][1])
    # a non-finite value under mask 1 is NOT hidden
    loc = c["loc"].clone()
    loc[int((~off).nonzero()[0]), 2] = float("nan")
    losses, _, dloc, _ = _run(c, loc=loc)
    assert not bool(torch.isfinite(losses[1])) and not bool(torch.isfinite(dloc).all())


def test_op_argument_checks_on_the_device():
    from disconet_amd import train_ops
    c = C.case("n7")
    t = [c[k].to(DEV) for k in ("cls", "labels", "loc", "targets", "mask")]
    with pytest.raises(ValueError, match="whole number of images"):
        train_ops.det_loss_corner(*t, c["anchors"][:3].to(DEV), norm=1.0)
    with pytest.raises(ValueError, match="GPU"):
        train_ops.det_loss_corner(*t, c["anchors"], norm=1.0)
    # [H, W, A, 6] anchors are taken as their rows
    a = train_ops.det_loss_corner(*t, c["anchors"].to(DEV), norm=1.0)
    b = train_ops.det_loss_corner(*t, c["anchors"].reshape(1, 7, 1, 6).to(DEV), norm=1.0)
    assert torch.equal(a[2], b[2])


def test_decode_boxes_keeps_its_expression():
    """dn_decode_boxes after its six box lines moved into the helper the corner loss shares: postprocess.decode's documented
    expression evaluated in fp32 on the host, to a few ulps (the device fuses multiply-adds and has its own expf)"""
    from disconet_amd import Config, postprocess
    g = torch.Generator().manual_seed(21)
    anchors = postprocess.make_anchors(Config(map_hw=8), device="cpu")                 # [8, 8, 6, 6]
    apl = 8 * 8 * 6
    cls = torch.randn(3, apl, 2, generator=g) * 3
    loc = torch.randn(3, 8, 8, 6, 1, 6, generator=g) * 0.5
    scores, boxes = postprocess.decode({"cls": cls.to(DEV), "loc": loc.to(DEV)}, anchors.to(DEV))
    a, t = anchors.reshape(1, apl, 6), loc.reshape(3, apl, 6)
    want = torch.stack([a[..., 0] + t[..., 0] * a[..., 2], a[..., 1] + t[..., 1] * a[..., 3], a[..., 2] * torch.exp(t[..., 2]),
                        a[..., 3] * torch.exp(t[..., 3]), a[..., 4] * t[..., 5] + a[..., 5] * t[..., 4],
                        a[..., 5] * t[..., 5] - a[..., 4] * t[..., 4]], -1)
    assert want.dtype == torch.float32
    assert torch.allclose(boxes.cpu(), want, rtol=2e-6, atol=2e-6)
    assert torch.allclose(scores.cpu(), torch.softmax(cls, -1)[..., 1], rtol=2e-6, atol=1e-7)


# ---- end to end: CoDetModule(config=Config(loss_type="corner_loss")) at the smallest configuration of test_gpu_train_step.py ----
HW, AGENTS, BATCH = 128, 2, 1


def _model():
    from disconet_amd import Config, DiscoNet
    torch.manual_seed(0)
    model = DiscoNet(Config(map_hw=HW), kd_flag=0, num_agent=AGENTS)
    for m in model.modules():      # O(1) activations and gradients (the parity tests' init)
        if isinstance(m, (torch.nn.Conv2d, torch.nn.Conv3d)):
            torch.nn.init.kaiming_normal_(m.weight, nonlinearity="relu")
    return model.cuda()


def _data():
    from disconet_amd import Config, postprocess
    from disconet_amd.synthetic import make_scene_batch, make_train_targets
    bevs, trans, na = make_scene_batch(BATCH, AGENTS, HW, jitter_seed=101)
    labels, targets, mask = make_train_targets(bevs.shape[0], HW, p_fg=0.02)
    return {"bev_seq": bevs.cuda(), "trans_matrices": trans.cuda(), "num_agent": na.cuda(), "labels": labels.cuda(),
            "reg_targets": targets.cuda(), "reg_loss_mask": mask.cuda(), "anchors": postprocess.make_anchors(Config(map_hw=HW))}


def test_step_trains_with_the_corner_loss():
    """loc_loss is the corner loss of the step's own predictions, and the step's gradients are what engine.backward makes of
    the standalone op's dcls / dloc -- bit for bit.  (Before Config.loss_type was read, loc_loss was the smooth-L1 value.)"""
    from disconet_amd import CoDetModule, Config, train_ops
    data = _data()
    mod = CoDetModule(_model(), config=Config(map_hw=HW, loss_type="corner_loss"), lr=1e-3)
    out = mod.step(data, BATCH, update=False)
    assert sorted(out) == ["cls_loss", "loc_loss", "loss"]
    res = mod.engine.last_result
    n_img = data["bev_seq"].shape[0]
    anchors = data["anchors"].reshape(-1, 6)
    want = float(train_ops.host_corner_loss(res["loc"].reshape(-1, 6).double().cpu(), data["reg_targets"].reshape(-1, 6).double().cpu(),
                                            data["reg_loss_mask"].reshape(-1).double().cpu(), anchors.double().cpu(), n_img))
    print("loc_loss %.9g host_corner_loss %.9g" % (out["loc_loss"], want))
    assert abs(out["loc_loss"] - want) <= 1e-5 * want
    assert abs(out["loss"] - out["cls_loss"] - out["loc_loss"]) <= 1e-12 * out["loss"]
    g_step = mod.engine.flat_g.clone()

    other = CoDetModule(_model(), lr=1e-3)                 # the same seeded weights in a fresh engine: the same first backward
    with torch.no_grad():
        r2 = other.engine.forward(data["bev_seq"], data["trans_matrices"], data["num_agent"], BATCH)
    assert torch.equal(r2["loc"], res["loc"])
    f32 = lambda t, shape: t.float().reshape(shape).contiguous()
    losses, dcls, dloc = train_ops.det_loss_corner(r2["cls"].reshape(-1, 2), f32(data["labels"], (-1, 2)), r2["loc"].reshape(-1, 6),
                                                   f32(data["reg_targets"], (-1, 6)), f32(data["reg_loss_mask"], (-1,)), anchors,
                                                   norm=n_img)
    other.engine.backward(dcls, dloc)
    assert torch.equal(C.bits(other.engine.flat_g), C.bits(g_step))
    assert abs(float(losses[1]) - out["loc_loss"]) <= 1e-12 * out["loc_loss"]
    # the anchors may come with a leading image dimension of identical copies (upstream's loader): the first image's are used
    stacked = dict(data, anchors=torch.stack([data["anchors"]] * n_img))
    third = CoDetModule(_model(), config=Config(map_hw=HW, loss_type="corner_loss"), lr=1e-3)
    third.step(stacked, BATCH, update=False)
    assert torch.equal(C.bits(third.engine.flat_g), C.bits(g_step))
    with pytest.raises(KeyError, match="anchors"):
        third.step({k: v for k, v in data.items() if k != "anchors"}, BATCH, update=False)


def test_default_loss_path_is_untouched():
    """loss_type="faf_loss" and config=None: the same gradients bit for bit, the smooth-L1 value as loc_loss"""
    from disconet_amd import CoDetModule, Config, train_ops
    data = _data()
    got = {}
    for key, cfg in (("faf", Config(map_hw=HW, loss_type="faf_loss")), ("none", None)):
        mod = CoDetModule(_model(), config=cfg, lr=1e-3)                  # (seeded: the same weights every time)
        out = mod.step(data, BATCH, update=False)
        got[key] = (out, mod.engine.flat_g.clone(), mod.engine.last_result)
    assert torch.equal(C.bits(got["faf"][1]), C.bits(got["none"][1]))
    for k in ("loss", "cls_loss", "loc_loss"):                            # (the values leave through f64 atomics: last bits)
        assert abs(got["faf"][0][k] - got["none"][0][k]) <= 1e-12 * got["none"][0][k], k
    res = got["none"][2]
    f32 = lambda t, shape: t.float().reshape(shape).contiguous()
    losses, _, _ = train_ops.det_loss(res["cls"].reshape(-1, 2), f32(data["labels"], (-1, 2)), res["loc"].reshape(-1, 6),
                                      f32(data["reg_targets"], (-1, 6)), f32(data["reg_loss_mask"], (-1,)), norm=data["bev_seq"].shape[0])
    assert abs(float(losses[1]) - got["none"][0]["loc_loss"]) <= 1e-12 * float(losses[1])


def test_train_tool_passes_the_loss_type_on(monkeypatch, capsys):
    """tools/det/train_codet.py --loss_type corner_loss, in this process: every step goes through det_loss_corner (with the
    anchors the tool made once) and none through det_loss"""
    import importlib.util
    import os
    from disconet_amd import train_ops
    here = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "det")
    monkeypatch.syspath_prepend(here)
    spec = importlib.util.spec_from_file_location("train_codet_corner_gpu", os.path.join(here, "train_codet.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    calls = {"corner": 0, "faf": 0}
    real_corner, real_faf = train_ops.det_loss_corner, train_ops.det_loss

    def corner(*a, **kw):
        calls["corner"] += 1
        assert a[5].shape == (256 * 256 * 6, 6)
        return real_corner(*a, **kw)

    def faf(*a, **kw):
        calls["faf"] += 1
        return real_faf(*a, **kw)

    monkeypatch.setattr(train_ops, "det_loss_corner", corner)
    monkeypatch.setattr(train_ops, "det_loss", faf)
    tool.main(["--com", "disco", "--loss_type", "corner_loss", "--targets", "boxes", "--num_agent", "2", "--batch", "1",
               "--nepoch", "1", "--steps_per_epoch", "2"])
    assert calls == {"corner": 2, "faf": 0}
    out = capsys.readouterr().out
    assert "loc_loss" in out and "nan" not in out.lower(), out


def test_twenty_adam_steps_lower_the_corner_loss_on_box_targets():
    """--targets boxes-style data: targets.assign_targets on one fixed make_box_scene_batch"""
    from disconet_amd import CoDetModule, Config, postprocess, targets
    from disconet_amd.synthetic import make_box_scene_batch
    cfg = Config(map_hw=HW, loss_type="corner_loss")
    scene = make_box_scene_batch(BATCH, AGENTS, HW, seed=0, boxes_per_scene=24, device=DEV)
    anchors = postprocess.make_anchors(cfg)
    data = {k: scene[k] for k in ("bev_seq", "trans_matrices", "num_agent")}
    data.update(targets.assign_targets(anchors, scene["gt_boxes"], scene["gt_count"]))
    data["anchors"] = anchors
    assert float(data["reg_loss_mask"].sum()) > 0
    mod = CoDetModule(_model(), config=cfg, lr=1e-3)
    curve = [mod.step(data, BATCH)["loc_loss"] for _ in range(20)]
    print("loc_loss", ["%.4g" % v for v in curve])
    assert all(v == v and v < float("inf") for v in curve)
    assert curve[-1] < curve[0]
