"""The selective feature exchange without a GPU: the library's entry points and sizes, the numpy statement
(disconet_amd.exchange.host_select / host_encode_cells / host_decode_cells) against independent routes, malformed wires,
and the plumbing through Detector, DiscoNet and the tools' command lines.

The independent routes share only the contract's words (include/disconet_hip.h, "Selective exchange") with exchange.py:
the selection is a Python sorted() on (-max |v| as float64, index) for finite inputs (exchange.py orders bit patterns), and
the decoded map is where(selected, the DENSE host round trip, +0.0) (exchange.py gathers rows, encodes the [1, K, c] image
and scatters its decode)."""
import argparse
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

from tests import exchange_cells_cases as cc
from tests.conftest import ROOT

from disconet_amd import exchange as ex

FORMATS = ("f32", "f16", "mxfp8", "mxfp4")
SIZES = {((32, 32, 256), 128): (131344, 65808, 34064, 17680), ((3, 5, 64), 7): (1824, 928, 496, 272)}
SHAPE_K = [((2, 3, 5, 64), 1), ((2, 3, 5, 64), 7), ((2, 3, 5, 64), 15), ((3, 8, 8, 32), 20), ((1, 1, 1, 32), 1)]


def _bits_equal(got, want):
    """equal in every bit; where `want` is a NaN only the position is compared (the contract fixes no NaN payload)"""
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]))


def _selected_mask(x, cells):
    index, count = ex.host_select(x, cells)
    n, h, w, _ = x.shape
    mask = np.zeros((n, h * w), bool)
    for i in range(n):
        mask[i, index[i, :count[i]]] = True
    return mask


def _dense_roundtrip(x, fmt):
    n, h, w, c = x.shape
    return x if fmt == "f32" else ex.host_decode(ex.host_encode(x, fmt), fmt, h, w, c)


def test_library_exports_the_entry_points():
    from disconet_amd import _lib, ops
    lib = _lib.load()
    for name in ("dn_exchange_cells_message_bytes", "dn_exchange_cells_workspace_bytes", "dn_exchange_encode_cells",
                 "dn_exchange_decode_cells"):
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None
    assert lib.dn_version() >= 156
    for name in ("exchange_cells_message_bytes", "exchange_encode_cells", "exchange_decode_cells"):
        assert callable(getattr(ops, name))
    for name in ("host_select", "host_encode_cells", "host_decode_cells", "cells_message_bytes", "sent_bytes"):
        assert callable(getattr(ex, name))
    assert ops.EXCHANGE_FORMATS == ex.FORMATS == {"f32": 0, "f16": 1, "mxfp8": 2, "mxfp4": 3}      # no new format


def test_message_sizes_library_and_numpy_agree():
    from disconet_amd import _lib, ops
    for ((h, w, c), k), want in SIZES.items():
        assert tuple(ex.cells_message_bytes(f, h, w, c, k) for f in FORMATS) == want
        assert tuple(ops.exchange_cells_message_bytes(f, h, w, c, k) for f in FORMATS) == want
    for h, w, c in ((1, 1, 32), (3, 5, 64), (7, 9, 96), (32, 32, 256), (128, 128, 32)):
        P = h * w
        for k in sorted({1, 2, 7, 8, 9, P // 2 + 1, P - 1, P} & set(range(1, P + 1))):
            for f in FORMATS:
                nbytes = ex.cells_message_bytes(f, h, w, c, k)
                assert nbytes == ops.exchange_cells_message_bytes(f, h, w, c, k) and nbytes % 16 == 0
                assert nbytes == 16 + (2 * k + 15) // 16 * 16 + ex.message_bytes(f, 1, k, c)
    # what the library and the numpy statement refuse: P past the LDS limit, K outside [1, P], c no multiple of 32
    for h, w, c, k in ((128, 129, 32, 5), (1, 16385, 32, 5), (3, 5, 64, 0), (3, 5, 64, 16), (3, 5, 48, 4), (3, 5, 64, -1)):
        with pytest.raises(_lib.DnError):
            ops.exchange_cells_message_bytes("mxfp8", h, w, c, k)
        with pytest.raises(ValueError):
            ex.cells_message_bytes("mxfp8", h, w, c, k)
    with pytest.raises(_lib.DnError):
        ops.exchange_cells_message_bytes(9, 3, 5, 64, 4)
    lib = _lib.load()
    assert lib.dn_exchange_cells_workspace_bytes(3, 32, 32) >= 3 * 1024 * 4
    assert lib.dn_exchange_cells_workspace_bytes(1, 128, 129) < 0 and lib.dn_exchange_cells_workspace_bytes(0, 4, 4) < 0


def test_sent_bytes():
    # 16 + 2 count + count c bits / 8 (+ count c / 32 scale bytes for MX); at count = K = 128 of 256 channels the index list
    # needs no padding and neither do the scales, so it equals the capacity message
    for f, want in zip(FORMATS, SIZES[((32, 32, 256), 128)]):
        assert ex.sent_bytes(f, 256, 128) == want
    assert ex.sent_bytes("f32", 64, 0) == ex.sent_bytes("mxfp4", 64, 0) == 16
    assert ex.sent_bytes("f16", 64, 7) == 16 + 14 + 7 * 128
    assert ex.sent_bytes("mxfp8", 64, 7) == 16 + 14 + 7 * 64 + 14
    assert ex.sent_bytes("mxfp4", 64, 7) == 16 + 14 + 7 * 32 + 14
    assert ex.sent_bytes("mxfp4", 256, 2.5) == 16 + 2.5 * (2 + 128 + 8)


@pytest.mark.parametrize("shape,cells", SHAPE_K, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else "K%d" % v)
def test_select_equals_a_python_sort(shape, cells):
    for name, x in cc.named_inputs(*shape, cells, seed=sum(shape)).items():
        if not np.isfinite(x).all():
            continue
        index, count = ex.host_select(x, cells)
        assert index.shape == (shape[0], cells) and index.dtype == np.uint16 and count.dtype == np.int32
        n, P = shape[0], shape[1] * shape[2]
        for i in range(n):
            mag = np.abs(x[i].reshape(P, -1).astype(np.float64)).max(axis=1)
            order = sorted(range(P), key=lambda p: (-mag[p], p))
            want = sorted(p for p in order[:cells] if mag[p] > 0)
            assert count[i] == len(want) == min(cells, int((mag > 0).sum())), name
            assert index[i, :count[i]].tolist() == want, name
            assert (index[i, count[i]:] == 0xFFFF).all(), name


def test_ties_go_to_the_lower_index():
    x = cc.equal_scores(2, 3, 5, 64, seed=1)
    for k in (1, 4, 15):
        index, count = ex.host_select(x, k)
        assert count.tolist() == [k, k] and (index == np.arange(k)).all()
    x = cc.tie_run(1, 8, 8, 32, 20, seed=2)
    score = np.abs(x.reshape(64, 32)).max(axis=1)
    index, count = ex.host_select(x, 20)
    chosen = set(index[0].tolist())
    run = np.nonzero(score == 2.0)[0]
    taken = [p for p in run if p in chosen]
    assert count[0] == 20 and 0 < len(taken) < len(run)                  # the run straddles the boundary
    assert taken == run[:len(taken)].tolist()                            # ... and its lowest indices went
    assert all(p in chosen for p in np.nonzero(score > 2.0)[0])


def test_zero_cells_are_never_sent_and_the_tail_is_padded():
    for fmt in FORMATS:
        x = cc.negative_zero_only(2, 3, 5, 64)
        wire = ex.host_encode_cells(x, fmt, 7)
        assert wire[:, :4].view("<u4").reshape(-1).tolist() == [0, 0]
        assert (wire[:, 4:16] == 0).all() and (wire[:, 16:30] == 0xFF).all() and (wire[:, 30:] == 0).all()
        assert (ex.host_decode_cells(wire, fmt, 3, 5, 64, 7).view(np.uint32) == 0).all()      # +0.0, not -0.0
    x = cc.short_count(3, 3, 5, 64, 7, seed=3)
    index, count = ex.host_select(x, 7)
    assert count.tolist() == [3, 3, 0]
    score = ex.host_scores(x)
    for i in range(3):
        assert (score[i, index[i, :count[i]]] > 0).all() and (index[i, count[i]:] == 0xFFFF).all()
    wire = ex.host_encode_cells(x, "f32", 7)
    body = wire[:, 32:].view(np.uint32).reshape(3, 7, 64)
    for i in range(3):
        assert (body[i, count[i]:] == 0).all()                           # rows at and beyond count: +0.0 in every channel
        assert np.array_equal(body[i, :count[i]], x[i].reshape(15, 64)[index[i, :count[i]]].view(np.uint32))


def test_non_finite_cells_are_selected_first():
    x = cc.non_finite(4, 3, 5, 64, seed=4)
    bad = ~np.isfinite(x).all(axis=3).reshape(4, 15)
    assert (bad.sum(axis=1) == 2).all()
    for k in (2, 3, 7):
        assert (_selected_mask(x, k) & bad).sum() == 8
    index, count = ex.host_select(x, 1)
    assert count.tolist() == [1] * 4 and all(bad[i, index[i, 0]] for i in range(4))
    nan_cell = np.isnan(x).any(axis=3).reshape(4, 15)
    assert all(nan_cell[i, index[i, 0]] for i in range(4))               # a NaN's bit pattern lies above Inf's


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("shape,cells", SHAPE_K, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else "K%d" % v)
def test_decoded_map_is_the_dense_roundtrip_where_selected(shape, cells, fmt):
    n, h, w, c = shape
    for name, x in cc.named_inputs(*shape, cells, seed=sum(shape) + cells).items():
        wire = ex.host_encode_cells(x, fmt, cells)
        assert wire.shape == (n, ex.cells_message_bytes(fmt, h, w, c, cells)) and wire.dtype == np.uint8
        got = ex.host_decode_cells(wire, fmt, h, w, c, cells)
        mask = _selected_mask(x, cells).reshape(n, h, w, 1)
        want = np.where(mask, _dense_roundtrip(x, fmt), np.float32(0.0)).astype(np.float32)
        assert _bits_equal(got, want), name


@pytest.mark.parametrize("fmt", FORMATS)
def test_every_cell_of_capacity_is_the_dense_roundtrip_of_non_zero_cells(fmt):
    n, h, w, c = 2, 3, 5, 64
    for name, x in cc.named_inputs(n, h, w, c, h * w, seed=9).items():
        got = ex.host_decode_cells(ex.host_encode_cells(x, fmt, h * w), fmt, h, w, c, h * w)
        live = (ex.host_scores(x) > 0).reshape(n, h, w, 1)
        want = np.where(live, _dense_roundtrip(x, fmt), np.float32(0.0)).astype(np.float32)
        assert _bits_equal(got, want), name
        assert (ex.host_select(x, h * w)[1] == live.reshape(n, -1).sum(axis=1)).all()


@pytest.mark.parametrize("fmt", FORMATS)
def test_malformed_wires(fmt):
    x, wire, over, past, (h, w, c, cells) = cc.malformed_wires(fmt)
    good = ex.host_decode_cells(wire, fmt, h, w, c, cells)
    assert _bits_equal(ex.host_decode_cells(over, fmt, h, w, c, cells), good)          # the count is clamped to K
    skipped = ex.host_decode_cells(past, fmt, h, w, c, cells)
    want = good.copy()
    want.reshape(2, h * w, c)[:, cells - 1] = 0                                        # (equal scores: cells 0 .. K - 1 went)
    assert _bits_equal(skipped, want) and not _bits_equal(skipped, good)
    with pytest.raises(ValueError):
        ex.host_decode_cells(wire[:, :-16], fmt, h, w, c, cells)


# ---------------------------------------------------------------------------------------------
# plumbing
# ---------------------------------------------------------------------------------------------
def _tiny_config():
    from disconet_amd import Config
    return Config(map_hw=32)                 # the exchanged level-3 map is 4 x 4: P = 16


def test_detector_takes_cells_for_disco_only():
    from disconet_amd import Detector
    cfg = _tiny_config()
    det = Detector("disco", cfg, 3, 1, device="cpu")
    assert det.model.exchange_cells == 0 and det.model.exchange == "f32" and det.model.exchange_sent is None
    det = Detector("disco", cfg, 3, 1, exchange_cells=5, device="cpu")
    assert det.model.exchange_cells == 5 and det.model.exchange == "f32"
    det = Detector("disco", cfg, 3, 1, exchange="mxfp4", exchange_cells=16, device="cpu")
    assert det.model.exchange_cells == 16 and det.model.exchange == "mxfp4"
    for com in ("sum", "lowerbound", "late", "agent"):
        with pytest.raises(ValueError, match="exchange_cells = 5.*" + com):
            Detector(com, cfg, 3, 1, exchange_cells=5, device="cpu")
        assert Detector(com, cfg, 3, 1, exchange_cells=0, device="cpu").model.exchange_cells == 0
    for bad in (17, -1):
        with pytest.raises(ValueError, match=r"exchange_cells = %d.*P = 16" % bad):
            Detector("disco", cfg, 3, 1, exchange_cells=bad, device="cpu")


def test_model_refuses_training_values_outside_the_map_and_baselines():
    from disconet_amd import DiscoNet, SumFusion
    cfg = _tiny_config()
    args = (torch.zeros(3, 1, 32, 32, 13), torch.zeros(1, 3, 3, 4, 4), torch.full((1, 3), 3))
    model = DiscoNet(cfg, kd_flag=0, num_agent=3)
    assert model.exchange_cells == 0 and model.exchange_sent is None
    model.exchange_cells = 4
    model.train()
    with pytest.raises(NotImplementedError, match="exchange_cells = 4"):
        model(*args, 1)
    model.eval()
    for bad in (17, -3, 2.5):
        model.exchange_cells = bad
        with pytest.raises(ValueError, match="exchange_cells = %s.*P = 16" % bad):
            model(*args, 1)
    base = SumFusion(cfg, kd_flag=0, num_agent=3).eval()
    base.exchange_cells = 4
    with pytest.raises(ValueError, match="SumFusion.exchange_cells = 4"):
        base(*args, 1)
    # cells = 0 leaves the format's rules as they were
    model.exchange_cells = 0
    model.exchange = "f16"
    model.train()
    with pytest.raises(NotImplementedError, match="DiscoNet.exchange = 'f16'"):
        model(*args, 1)
    model.eval()
    model.exchange = "int8"
    with pytest.raises(ValueError, match="int8"):
        model(*args, 1)
    with pytest.raises(ValueError, match="int8"):
        ex.roundtrip(torch.zeros(1, 2, 2, 32), "int8", cells=2)
    t = torch.zeros(1, 2, 2, 32)
    assert ex.roundtrip(t, "f32") is t and ex.roundtrip(t, "f32", cells=0, sent=None) is t


def _tool(folder, name):
    for d in (os.path.join(ROOT, "tools", "det"), os.path.join(ROOT, "tools", "track")):
        if d not in sys.path:
            sys.path.insert(0, d)
    spec = importlib.util.spec_from_file_location("exchange_cells_cli_" + name, os.path.join(ROOT, "tools", folder, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("folder,name,parse", [
    ("det", "detect_codet", lambda m, a: m.build_detect_parser().parse_args(a)),
    ("det", "eval_codet", lambda m, a: m.build_eval_parser().parse_args(a)),
    ("det", "visualize_codet", lambda m, a: m.build_vis_parser().parse_args(a)),
    ("track", "sort_codet", lambda m, a: m.parse_args(a)),
    ("track", "eval_sort", lambda m, a: m.parse_args(a + ["--source", "net"])),
])
def test_tools_parse_the_flag(folder, name, parse, capsys):
    mod = _tool(folder, name)
    args = parse(mod, ["--com", "disco"])
    assert args.exchange_cells == 0 and args.exchange == "f32"
    args = parse(mod, ["--com", "disco", "--exchange_cells", "128", "--exchange", "mxfp4"])
    assert args.exchange_cells == 128 and args.exchange == "mxfp4"
    assert parse(mod, ["--com", "disco", "--exchange_cells", "64"]).exchange == "f32"
    with pytest.raises(SystemExit):
        parse(mod, ["--com", "disco", "--exchange_cells", "many"])
    assert "many" in capsys.readouterr().err


def test_tools_lines_and_source_rule():
    common = _tool("det", "codet_common")
    from disconet_amd import Config
    cfg = Config("test", binary=True, only_det=True)
    line = common.exchange_line(argparse.Namespace(exchange="mxfp4", exchange_cells=128, layer=3), cfg)
    assert "mxfp4" in line and "128 cells" in line and "17680" in line and "1048576" in line and "32 x 32 x 256" in line
    line = common.exchange_line(argparse.Namespace(exchange="f32", exchange_cells=128, layer=3), cfg)
    assert "131344" in line
    # a namespace from before the flag, and the flag at 0: the format's line as it was
    for ns in (argparse.Namespace(exchange="mxfp8", layer=3), argparse.Namespace(exchange="mxfp8", exchange_cells=0, layer=3)):
        line = common.exchange_line(ns, cfg)
        assert "270336" in line and "cells" not in line
    assert common.exchanges(argparse.Namespace(exchange="f32", exchange_cells=4))
    assert common.exchanges(argparse.Namespace(exchange="f16")) and not common.exchanges(argparse.Namespace(exchange="f32"))

    class _Model:
        def exchange_sent_summary(self):
            return {"frames": 4, "cells_per_image": [100.0, 50.0], "mean_cells": 75.0}

    line = common.exchange_sent_line(argparse.Namespace(exchange="mxfp4", exchange_cells=128, layer=3),
                                     argparse.Namespace(model=_Model()))
    assert "75.0 cells" in line and "4 frames" in line and "capacity 128" in line
    assert "%.0f bytes" % ex.sent_bytes("mxfp4", 256, 75.0) in line
    with pytest.raises(SystemExit, match="exchange_cells 64"):
        _tool("track", "eval_sort").parse_args(["--com", "disco", "--exchange_cells", "64"])      # --source boxes: no network
    with pytest.raises(SystemExit, match="exchange_cells 64"):
        _tool("track", "sort_codet").parse_args(["--com", "disco", "--exchange_cells", "64", "--source", "lidar",
                                                 "--detections", "truth"])
