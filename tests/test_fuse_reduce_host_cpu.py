"""Host side of the parameter-free collaboration baselines `--com sum | mean | max` (disconet_amd.fusion_modes): the C ABI's
new symbols, the contract in plain torch (host_fuse_reduce) against the twins of tests/reduce_fusion_ref.py, the model
classes' parameters and the tools' command lines.  No GPU."""
import ctypes
import importlib.util
import os
import re
from unittest import mock

import pytest
import torch

from tests import fusion_fp64 as f64
from tests import reduce_fusion_ref as rf
from tests.conftest import ROOT

MODES = rf.MODES


def test_library_has_the_entry_points_with_the_bound_signatures():
    from disconet_amd import _lib
    from disconet_amd.csrc import build
    lib = _lib.load()
    assert lib.dn_version() >= 147
    assert "fuse_reduce.hip" in build.SOURCES
    text = {h: re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", h)).read(), flags=re.S)
            for h in ("disconet_hip.h", "disconet_train.h")}
    for name, header, n_args in (("dn_fuse_reduce", "disconet_hip.h", 14), ("dn_fuse_reduce_lists", "disconet_train.h", 10),
                                 ("dn_fuse_reduce_lists_backward", "disconet_train.h", 13)):
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, text[header])
        assert decl and len(decl.group(1).split(",")) == n_args, name
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is ctypes.c_int and len(argtypes) == n_args
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == list(argtypes)
    for k, v in (("DN_FUSE_SUM", 0), ("DN_FUSE_MEAN", 1), ("DN_FUSE_MAX", 2)):
        assert re.search(r"#define %s %d\b" % (k, v), text["disconet_hip.h"])
    from disconet_amd import ops
    assert ops.FUSE_MODES == {"sum": 0, "mean": 1, "max": 2}


def _case(A, B, h, w, c, seed):
    poses, _ = f64.sweep(h, w)
    g = torch.Generator().manual_seed(seed)
    trans = poses[torch.randperm(poses.shape[0], generator=g)[:B * A * A]].reshape(B, A, A, 4, 4).contiguous()
    return f64.sweep_maps(A * B, c, h, w, seed=seed), trans


@pytest.mark.parametrize("A,B,live,only_v2i,ego", [(4, 2, [3, 2], False, (0, None)), (4, 2, [4, 3], True, (0, None)),
                                                   (3, 2, [0, 7], False, (0, None)), (5, 1, [5], False, (1, 2))])
def test_host_fuse_reduce_is_the_twins_fp32_loop_and_within_the_bounds_of_float64(A, B, live, only_v2i, ego):
    """padded egos, only_v2i, counts of 0 and above A (clamped), an ego sub-range"""
    from disconet_amd.fusion_modes import host_fuse_reduce
    maps, trans = _case(A, B, 12, 16, 8, seed=A * 10 + B)
    ref = rf.Loop(maps, trans, live, A, B, only_v2i, ego[0], ego[1])
    assert ref.E_w > 0 and ref.nonzero >= 0.6 * ref.n_warps
    feat = rf.nhwc(maps)
    for m in MODES:
        got = host_fuse_reduce(feat, trans, live, B, A, m, only_v2i, ego[0], ego[1])
        assert torch.equal(got, rf.nhwc(ref.fused[torch.float32][m])), m
        err = (got.double() - rf.nhwc(ref.fused[torch.float64][m])).abs().max().item()
        assert err <= ref.bound(m), (m, err, ref.bound(m))
        E = A if ego[1] is None else ego[1]
        for b, i, js in rf.lists_of(live, A, B, only_v2i, ego[0], E):
            if not js:
                assert torch.equal(got[(i - ego[0]) * B + b], feat[i * B + b])       # a padded ego: the same bits
    if live == [0, 7]:
        assert ref.longest == A and ref.n_warps == A * (A - 1)                       # scene 0 empty, scene 1 clamped to A


def test_the_three_reductions_are_what_the_contract_says():
    """torch.stack(list).sum(0) is the sequential fp32 adds for 2..8 maps of a feature map's size (a stack of a few hundred
    elements per map is summed in another order by torch's CPU kernel: 64 x 16 x 16 and 256 x 32 x 32 here), .mean(0) is
    that sum / k, torch.max(dim=0) takes the first index among ties and the first NaN"""
    from disconet_amd.fusion_modes import reduce_list
    g = torch.Generator().manual_seed(1)
    for k in range(2, 9):
        shape = (64, 16, 16) if k % 2 else (256, 32, 32)
        maps = [torch.randn(*shape, generator=g) * 10.0 ** (i % 4 - 2) for i in range(k)]
        seq = maps[0].clone()
        for t in maps[1:]:
            seq = seq + t
        assert torch.equal(reduce_list(maps, "sum"), seq)
        assert torch.equal(reduce_list(maps, "mean"), seq / float(k))
    a = torch.tensor([1.0, 2.0, float("nan"), 0.0, -0.0, 5.0])
    b = torch.tensor([1.0, 3.0, 7.0, -0.0, 0.0, float("nan")])
    c = torch.tensor([2.0, 3.0, float("nan"), 0.0, 0.0, float("nan")])
    val, idx = torch.max(torch.stack([a, b, c]), dim=0)
    assert idx.tolist() == [2, 1, 0, 0, 0, 1]
    assert torch.equal(torch.isnan(val), torch.tensor([False, False, True, False, False, True]))
    assert torch.equal(torch.nan_to_num(reduce_list([a, b, c], "max"), nan=-1.0), torch.tensor([2.0, 3.0, -1.0, 0.0, 0.0, -1.0]))
    with pytest.raises(ValueError):
        reduce_list([a, b], "v2v")


def test_host_fuse_reduce_on_ties_and_nan():
    """post-ReLU maps (many exact zeros) under whole-pixel poses on a 32 x 32 map, where torch's fp32 warp copies: max is
    the elementwise maximum of the shifted maps, a NaN of a neighbour arrives where the pose carries it"""
    from disconet_amd.fusion_modes import host_fuse_reduce
    A, h, w, c = 2, 32, 32, 4
    g = torch.Generator().manual_seed(2)
    feat = torch.randn(A, h, w, c, generator=g).clamp_(min=0)
    feat[1, 10, 12, 1] = float("nan")
    trans = torch.eye(4).repeat(1, A, A, 1, 1)
    trans[0, 0, 1] = torch.from_numpy(f64.pose(0.0, 0.0, 0.0))
    got = host_fuse_reduce(feat, trans, [2], 1, A, "max")
    assert bool(torch.isnan(got[0, 10, 12, 1])) and int((got[0] == 0).sum()) > 100
    clean = torch.nan_to_num(feat[1], nan=0.0)
    sel = ~torch.isnan(got[0])
    assert torch.equal(got[0][sel], torch.maximum(feat[0], clean)[sel])


def test_models_own_no_attention_parameters():
    from disconet_amd import COM_MODES, Config, DiscoNet, MaxFusion, MeanFusion, SumFusion, build_model
    assert COM_MODES == ("disco", "sum", "mean", "max")
    disco = DiscoNet(Config())
    want = {k for k in disco.state_dict() if not k.startswith("pixel_weighted_fusion.")}
    assert len(want) < len(disco.state_dict())
    for com, cls in (("sum", SumFusion), ("mean", MeanFusion), ("max", MaxFusion)):
        m = build_model(com, Config(), layer=3, in_channels=13, kd_flag=True, num_agent=5, compress_level=0, only_v2i=False)
        assert type(m) is cls and m.com == com and not hasattr(m, "pixel_weighted_fusion")
        assert set(m.state_dict()) == want
        with pytest.raises(RuntimeError, match="Unexpected key"):
            m.load_state_dict(disco.state_dict())
        m.load_state_dict({"module." + k: v for k, v in disco.state_dict().items() if k in want})
        assert m._fusion_plan(0) == {}
    assert type(build_model("disco", Config(), num_agent=3)) is DiscoNet
    assert set(build_model("disco", Config()).state_dict()) == set(disco.state_dict())
    with pytest.raises(ValueError, match="v2v"):
        build_model("v2v", Config())


class _Reached(Exception):
    pass


def _tool(rel):
    spec = importlib.util.spec_from_file_location("tool_" + rel.replace("/", "_").replace(".py", ""), os.path.join(ROOT, "tools", rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("rel", ["det/train_codet.py", "det/detect_codet.py", "det/eval_codet.py",
                                 "track/sort_codet.py", "track/eval_sort.py"])
def test_det_and_track_tools_take_the_four_modes(rel, monkeypatch):
    mod = _tool(rel)
    with pytest.raises(SystemExit, match=r"disco \| sum \| mean \| max"):
        mod.main(["--com", "v2v"])

    asked = []

    def build_model(com, config, **kw):                  # what the tool builds its detector with: the mode must arrive here
        asked.append((com, kw["num_agent"]))
        raise _Reached()
    monkeypatch.setattr(torch.cuda, "set_device", lambda *a, **kw: None)
    if rel == "det/train_codet.py":                      # the training tool builds the model itself, ...
        monkeypatch.setattr(mod, "build_model", build_model)
    else:                                                # ... the others through Detector, the one construction site
        from disconet_amd import detector
        assert not hasattr(mod, "build_model")
        monkeypatch.setattr(detector, "build_model", build_model)
    extra = []
    if rel.startswith("track/"):                         # (the tracker and the metrics are built first, on the GPU: stand-ins)
        monkeypatch.setattr(mod, "tracking", mock.MagicMock())
        extra = ["--source", "net"]
    for com in ("max", "sum", "mean", "disco"):
        with pytest.raises(_Reached):
            mod.main(["--com", com, "--num_agent", "3"] + extra)
    assert asked == [(com, 3) for com in ("max", "sum", "mean", "disco")]


@pytest.mark.parametrize("rel", ["seg/train_seg.py", "seg/test_seg.py", "seg/eval_seg.py"])
def test_seg_tools_still_refuse_everything_but_disco(rel):
    mod = _tool(rel)
    for com in ("max", "sum", "mean", "v2v"):
        with pytest.raises(SystemExit, match="only --com disco is built"):
            mod.main(["--com", com])
