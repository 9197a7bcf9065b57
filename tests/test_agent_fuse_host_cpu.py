"""Host side of `--com agent` (disconet_amd.fusion_modes.AgentWeightedFusion): the C ABI's new symbols and refusals, the
contract in plain torch (host_agent_fuse) against the twins of tests/agent_fusion_ref.py, the model's parameters, the mode
tuples and the tools' command lines.  No GPU.

host_agent_fuse sums a_k in the contract's order (tiles of 32 pixels, a tree inside a tile, the tiles ascending) and the fp32
twin through torch's Conv2d(1, 1, (h, w)): two fp32 orders of one sum, so the two agree within the bounds the GPU tests use
(weights: FACTOR x the fp32 twin's own distance from float64; fused maps: TOL + that x sum |map_k|), not bit for bit."""
import ctypes
import importlib.util
import os
import re
from unittest import mock

import pytest
import torch

from tests import agent_fusion_ref as ar
from tests.conftest import ROOT


def test_library_has_the_entry_points_with_the_bound_signatures():
    from disconet_amd import _lib
    from disconet_amd.csrc import build
    lib = _lib.load()
    assert lib.dn_version() >= 149
    assert "agent_fuse.hip" in build.SOURCES and "disconet_amd/csrc/agent_device.h" in build.tree_files()
    text = {h: re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", h)).read(), flags=re.S)
            for h in ("disconet_hip.h", "disconet_train.h")}
    for name, header, restype, n_args in (("dn_agent_fuse", "disconet_hip.h", ctypes.c_int, 19),
                                          ("dn_agent_fuse_workspace_bytes", "disconet_hip.h", ctypes.c_size_t, 4),
                                          ("dn_agent_combine_lists", "disconet_train.h", ctypes.c_int, 14),
                                          ("dn_agent_combine_lists_backward", "disconet_train.h", ctypes.c_int, 11)):
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, text[header])
        assert decl and len(decl.group(1).split(",")) == n_args, name
        want, argtypes = _lib.SIGNATURES[name]
        assert want is restype and len(argtypes) == n_args
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes)


def test_workspace_size_and_refusals_before_any_launch():
    """every refusal is DN_ERR_ARG with a message, decided on the host: no GPU is needed to be refused"""
    from disconet_amd import _lib
    lib = _lib.load()
    assert lib.dn_agent_fuse_workspace_bytes(2, 5, 5, 1024) == 2 * 5 * 5 * 32 * 4
    assert lib.dn_agent_fuse_workspace_bytes(1, 3, 2, 30) == (1 * 2 * 3 * 1 * 4 + 15) // 16 * 16
    assert lib.dn_agent_fuse_workspace_bytes(0, 3, 3, 64) == 0
    p = _lib.FuseMlpParams()
    x = 4096      # a non-null, 16-byte aligned address that is never dereferenced: every call below is refused first

    def call(feat=x, warped=x, fm=0, na=x, params=p, w5=x, b5=x, B=1, A=3, hw=64, c=64, v2i=0, e0=0, ec=3, ws=x, wsb=1 << 20,
             fused=x, weights=None):
        return lib.dn_agent_fuse(feat, warped, fm, na, ctypes.byref(params), w5, b5, B, A, hw, c, v2i, e0, ec, ws, wsb, fused,
                                 weights, None)
    for kw, msg in ((dict(feat=None), b"null"), (dict(w5=None), b"null"), (dict(b5=None), b"null"), (dict(fused=None), b"null"),
                    (dict(ws=None), b"null"), (dict(na=None), b"null"), (dict(warped=None), b"warped is null"),
                    (dict(e0=2, ec=2), b"ego range"), (dict(ec=0), b"ego range"), (dict(c=96), b"channels unsupported"),
                    (dict(c=512), b"channels unsupported"), (dict(A=9, ec=9), b"at most 8 agents"),
                    (dict(wsb=16), b"workspace"), (dict(fm=1, hw=30), b"multiple of 32"), (dict(fused=x + 4), b"16-byte"),
                    (dict(B=0), b"empty")):
        assert call(**kw) == -1, kw                       # DN_ERR_ARG
        assert msg in lib.dn_last_error(), (kw, lib.dn_last_error())
    assert call() == -1 and b"null MLP parameter" in lib.dn_last_error()      # (the packed weight net is checked too)
    assert lib.dn_agent_combine_lists(None, x, x, x, x, x, x, x, 1, 64, 64, x, x, None) == -1
    assert lib.dn_agent_combine_lists(x, x, x, x, x, x, x, x, 1, 64, 6, x, x, None) == -1
    assert lib.dn_agent_combine_lists_backward(x, 64, None, x, x, x, 1, 64, 64, x, None) == -1
    assert lib.dn_agent_combine_lists_backward(x, 62, x, x, x, x, 1, 64, 64, x, None) == -1


@pytest.mark.parametrize("shape", [ar.SHAPES[0], ar.SHAPES[1], ar.SHAPES[4], ar.SHAPES[5]], ids=str)
def test_host_agent_fuse_is_the_twins_loop_within_the_bounds(shape):
    """two tiles, a non-square conv1_5 with only_v2i and a padded ego, agents == 1, h * w = 30"""
    from disconet_amd.fusion_modes import host_agent_fuse
    A, B, h, w, C, _, v2i = shape
    net, feat, trans, live, ref = ar.make_case(shape)
    assert A == 1 or (ref.tells_agent_from_mean() and ref.E_w > 0)
    fused, weights = host_agent_fuse(ar.nhwc(feat), trans, live, B, A, net, v2i, want_weights=True)
    for dt, slack in ((torch.float64, 1.0), (torch.float32, 2.0)):      # (against the fp32 twin: both sit within the bound of float64)
        err_w = (weights.double() - ref.weights[dt].double()).abs().max().item()
        err_f = (fused.double() - ar.nhwc(ref.fused[dt]).double()).abs().max().item()
        assert err_w <= slack * ref.weight_bound(), (dt, err_w, ref.weight_bound())
        assert err_f <= slack * ref.fused_bound(), (dt, err_f, ref.fused_bound())
    x = ar.nhwc(feat)
    for b, i, js in ar.lists_of(live, A, B, v2i):
        n_live = max(0, min(live[b], A))
        if i >= n_live:                                   # a padded ego: the same bits, no weight
            assert torch.equal(fused[i * B + b], x[i * B + b]) and float(weights[b, i].abs().max()) == 0.0
        elif not js:                                      # a list of one entry: weight 1, the ego's own bits
            assert torch.equal(fused[i * B + b], x[i * B + b]) and weights[b, i].tolist() == [1.0] + [0.0] * (A - 1)
        else:
            assert abs(float(weights[b, i].sum()) - 1.0) < 1e-6 and float(weights[b, i, 1 + len(js):].abs().max() if 1 + len(js) < A else 0) == 0.0
    # an ego sub-range is the slice of the full result
    if A >= 3:
        part = host_agent_fuse(ar.nhwc(feat), trans, live, B, A, net, v2i, ego_first=1, ego_count=2)
        assert torch.equal(part, fused[B:3 * B])
    with pytest.raises(ValueError, match="ego range"):
        host_agent_fuse(ar.nhwc(feat), trans, live, B, A, net, v2i, ego_first=A, ego_count=1)


def test_the_scalar_and_the_sums_are_what_the_contract_says():
    """agent_scalar: tiles of 32 with zeros past the end, the tree l + 16, + 8, ... inside a tile, the tiles ascending -- spelled
    out element by element here; the softmax sums in list order; the weighted sum rounds every product"""
    from disconet_amd.fusion_modes import agent_scalar, agent_softmax, weighted_sum
    g = torch.Generator().manual_seed(4)
    for hw in (30, 64, 100):
        s, w5, b5 = torch.rand(hw, generator=g), torch.rand(hw, generator=g) + 0.5, torch.tensor([0.25])
        prod = (s * w5).tolist() + [0.0] * ((hw + 31) // 32 * 32 - hw)
        f32 = lambda v: torch.tensor(v, dtype=torch.float32)
        sums = []
        for t in range(len(prod) // 32):
            v = [f32(p) for p in prod[32 * t:32 * t + 32]]
            for d in (16, 8, 4, 2, 1):
                v = [v[k] + v[k + d] for k in range(d)]
            sums.append(v[0])
        acc = sums[0]
        for t in sums[1:]:
            acc = acc + t
        assert float(agent_scalar(s, w5, b5)) == float(torch.clamp(acc + b5[0], min=0.0))
    assert float(agent_scalar(torch.ones(40), torch.ones(40), torch.tensor([-50.0]))) == 0.0      # the ReLU
    a = torch.tensor([3.0, 1.0, 2.5, 3.0])
    e = torch.exp(a - 3.0)
    assert torch.equal(agent_softmax(a), e / (((e[0] + e[1]) + e[2]) + e[3]))
    assert agent_softmax(torch.tensor([7.5])).tolist() == [1.0]
    maps = [torch.randn(4, 3, 3, generator=g) for _ in range(3)]
    w = torch.tensor([0.2, 0.5, 0.3])
    assert torch.equal(weighted_sum(maps, w), (w[0] * maps[0] + w[1] * maps[1]) + w[2] * maps[2])


def test_model_parameters_mode_tuples_and_build_model():
    from disconet_amd import (ALL_DET_COM_MODES, COM_MODES, DET_COM_MODES, PARAM_COM_MODES, AgentWeightedFusion, Config, Detector,
                              DiscoNet, build_model)
    assert COM_MODES == ("disco", "sum", "mean", "max")                                  # the two pinned tuples: unchanged
    assert DET_COM_MODES == ("disco", "sum", "mean", "max", "lowerbound", "late")
    assert PARAM_COM_MODES == ("agent",) and ALL_DET_COM_MODES == DET_COM_MODES + PARAM_COM_MODES
    disco = DiscoNet(Config())
    m = build_model("agent", Config(), layer=3, in_channels=13, kd_flag=True, num_agent=5, compress_level=0, only_v2i=False)
    assert type(m) is AgentWeightedFusion and m.com == "agent" and not hasattr(m, "pixel_weighted_fusion")
    own = {k: tuple(v.shape) for k, v in m.state_dict().items() if k.startswith("agent_weighted_fusion.")}
    want = {k.replace("pixel_weighted_fusion.", "agent_weighted_fusion."): tuple(v.shape) for k, v in disco.state_dict().items()
            if k.startswith("pixel_weighted_fusion.")}
    want.update({"agent_weighted_fusion.conv1_5.weight": (1, 1, 32, 32), "agent_weighted_fusion.conv1_5.bias": (1,)})
    assert own == want                                                                    # upstream's names and shapes
    assert {k for k in m.state_dict() if k not in own} == {k for k in disco.state_dict() if not k.startswith("pixel_weighted_fusion.")}
    with pytest.raises(RuntimeError, match="Unexpected key"):
        m.load_state_dict(disco.state_dict())
    m.load_state_dict({"module." + k: v for k, v in m.state_dict().items()})
    twin = ar.build_agent_ref(128, 3)
    small = build_model("agent", Config(map_hw=128), num_agent=3)
    assert tuple(small.agent_weighted_fusion.conv1_5.weight.shape) == (1, 1, 16, 16)      # the exchanged map's own size
    small.load_state_dict(twin.state_dict())
    layer2 = build_model("agent", Config(map_hw=128), layer=2, num_agent=2)
    assert tuple(layer2.agent_weighted_fusion.conv1_5.weight.shape) == (1, 1, 32, 32)
    assert tuple(layer2.agent_weighted_fusion.conv1_1.weight.shape) == (128, 256, 1, 1)
    from disconet_amd.fusion_modes import AgentTrainEngine
    assert m._train_engine_class() is AgentTrainEngine and AgentTrainEngine._KD_OK is False
    with pytest.raises(ValueError, match=r"disco, sum, mean, max, lowerbound, late, agent \(got 'v2v'\)"):
        build_model("v2v", Config())
    det = Detector("agent", Config(map_hw=128), 2, 1, device="cpu")
    assert type(det.model) is AgentWeightedFusion and not det.model.training and det.com == "agent"


def _tool(rel):
    spec = importlib.util.spec_from_file_location("tool_" + rel.replace("/", "_").replace(".py", ""), os.path.join(ROOT, "tools", rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class _Reached(Exception):
    pass


@pytest.mark.parametrize("rel", ["det/train_codet.py", "det/detect_codet.py", "det/eval_codet.py",
                                 "track/sort_codet.py", "track/eval_sort.py"])
def test_det_and_track_tools_take_agent_and_still_refuse_v2v(rel, monkeypatch):
    mod = _tool(rel)
    with pytest.raises(SystemExit, match=r"disco \| sum \| mean \| max.*agent"):
        mod.main(["--com", "v2v"])
    asked = []

    def build_model(com, config, **kw):
        asked.append((com, kw["num_agent"]))
        raise _Reached()
    monkeypatch.setattr(torch.cuda, "set_device", lambda *a, **kw: None)
    if rel == "det/train_codet.py":
        monkeypatch.setattr(mod, "build_model", build_model)
    else:
        from disconet_amd import detector
        monkeypatch.setattr(detector, "build_model", build_model)
    extra = []
    if rel.startswith("track/"):
        monkeypatch.setattr(mod, "tracking", mock.MagicMock())
        extra = ["--source", "net"]
    with pytest.raises(_Reached):
        mod.main(["--com", "agent", "--num_agent", "3"] + extra)
    assert asked == [("agent", 3)]


def test_require_com_and_test_codet():
    import argparse
    common = _tool("det/codet_common.py")
    from disconet_amd import ALL_DET_COM_MODES
    common.require_com(argparse.Namespace(com="agent"), ALL_DET_COM_MODES)
    with pytest.raises(SystemExit):
        common.require_com(argparse.Namespace(com="v2v"), ALL_DET_COM_MODES)
    with pytest.raises(SystemExit, match="only --com disco is built"):
        _tool("det/test_codet.py").main(["--com", "agent"])
