"""The feature-exchange wire format without a GPU: the library's entry points, the message layout, the numpy statement
(disconet_amd.exchange.host_encode / host_decode) against independent routes through the same scale rule, the contract's
derived consequences, and the plumbing through Detector, DiscoNet and the tools' command lines.

The independent routes share only the contract's words with exchange.py: the scale exponent comes from numpy.frexp in
float64 (exchange.py reads the exponent field of the bit pattern), the E4M3 codes from torch's CPU float8_e4m3fn cast of
the scaled, clipped value (exchange.py rounds an integer significand), the E2M1 codes from the nearest of the eight
magnitudes in float64 with ties to the even code."""
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

from tests import exchange_cases as ec
from tests.conftest import ROOT

from disconet_amd import exchange as ex

MX = ("mxfp8", "mxfp4")
EMAX = {"mxfp8": 8, "mxfp4": 2}
BOUND = {"mxfp8": 1.0 / 8, "mxfp4": 1.0 / 4}       # |x - x'| <= BOUND * max |block|: derived in include/disconet_hip.h
HALF_QUANTUM_AT_FLOOR = {"mxfp8": 2.0 ** (-9 - 127 - 1), "mxfp4": 2.0 ** (-1 - 127 - 1)}
E2M1 = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])


def _blocks():
    """every block of the cases, [N, 32]: random non-negative, random signed, the edges"""
    return np.concatenate([ec.random_blocks(4096, False, 11), ec.random_blocks(4096, True, 12), ec.edge_array()])


def _as_images(blocks):
    return blocks.reshape(len(blocks), 1, 1, ec.BLOCK)


def _split(wire, fmt, blocks):
    """(element codes [N, 32], scale bytes [N]) of the wire of N one-block images"""
    p = ex.scale_offset(fmt, 1, 1, ec.BLOCK)
    code = wire[:, :p]
    if fmt == "mxfp4":
        code = np.stack([code & 0xF, code >> 4], axis=-1).reshape(len(blocks), ec.BLOCK)
    return code, wire[:, p]


def _scale_exponent(blocks, fmt):
    """the contract's e per block, through float64 frexp; None-flag for non-finite blocks"""
    finite = np.isfinite(blocks).all(axis=1)
    m = np.where(finite, np.abs(np.where(np.isfinite(blocks), blocks, 0)).max(axis=1), 1.0).astype(np.float64)
    E = np.frexp(m)[1] - 1                                   # m = f 2^ex, f in [0.5, 1): floor(log2 m) = ex - 1
    e = np.where(m == 0, -127, np.maximum(E - EMAX[fmt], -127))
    return e, finite


def test_library_exports_the_entry_points():
    from disconet_amd import _lib
    lib = _lib.load()
    for name in ("dn_exchange_message_bytes", "dn_exchange_encode", "dn_exchange_decode"):
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None
    assert lib.dn_version() >= 155
    import disconet_amd
    assert "exchange" in disconet_amd.__all__ and disconet_amd.exchange is ex
    from disconet_amd import ops
    assert ops.EXCHANGE_FORMATS == ex.FORMATS == {"f32": 0, "f16": 1, "mxfp8": 2, "mxfp4": 3}


def test_message_bytes_and_layout():
    from disconet_amd import _lib, ops
    want = {"f32": 1048576, "f16": 524288, "mxfp8": 270336, "mxfp4": 139264}
    for fmt, nbytes in want.items():
        assert ex.message_bytes(fmt, 32, 32, 256) == nbytes == ops.exchange_message_bytes(fmt, 32, 32, 256)
    assert ex.scale_offset("mxfp8", 32, 32, 256) == 262144 and ex.scale_offset("mxfp4", 32, 32, 256) == 131072
    # scale bytes padded to a multiple of 16: 3 x 5 pixels x 2 blocks = 30 -> 32; one block -> 16
    assert ex.message_bytes("mxfp8", 3, 5, 64) == 960 + 32 and ex.message_bytes("mxfp4", 3, 5, 64) == 480 + 32
    assert ex.message_bytes("mxfp8", 1, 1, 32) == 32 + 16 and ex.message_bytes("mxfp4", 1, 1, 32) == 16 + 16
    assert ex.message_bytes("f16", 1, 1, 32) == 64
    for shape in ((1, 1, 32), (3, 5, 64), (5, 7, 256), (2, 3, 512)):
        for fmt in ex.FORMATS:
            assert ex.message_bytes(fmt, *shape) == ops.exchange_message_bytes(fmt, *shape)
            assert ex.message_bytes(fmt, *shape) % 16 == 0
    with pytest.raises(_lib.DnError):
        ops.exchange_message_bytes("mxfp8", 4, 4, 48)
    with pytest.raises(_lib.DnError):
        ops.exchange_message_bytes(7, 4, 4, 64)
    with pytest.raises(ValueError):
        ex.message_bytes("mxfp8", 4, 4, 48)
    with pytest.raises(ValueError):
        ex.message_bytes("int8", 4, 4, 64)


def test_layout_offsets_payload_scales_padding():
    """[pixel][block] scale order, pixel-major channel-order payload, the low nibble first, zero padding"""
    h, w, c = 3, 5, 64
    x = np.zeros((2, h, w, c), np.float32)
    x[1, 2, 3, 32:] = 2.0 ** 20                  # image 1, pixel 13, block 1: scale exponent 20 - emax
    x[1, 2, 3, 33] = -(2.0 ** 20)
    for fmt in MX:
        wire = ex.host_encode(x, fmt)
        assert wire.shape == (2, ex.message_bytes(fmt, h, w, c)) and not wire[0].any()
        p = ex.scale_offset(fmt, h, w, c)
        scales = wire[1, p:p + h * w * 2]
        assert scales[13 * 2 + 1] == 20 - EMAX[fmt] + 127 and np.count_nonzero(scales) == 1
        assert not wire[1, p + h * w * 2:].any() and wire.shape[1] - (p + h * w * 2) == 2
        first = (13 * c + 32) // (1 if fmt == "mxfp8" else 2)
        if fmt == "mxfp8":                       # 2^8 = 1.0 x 2^(15 - 7): code 0x78, and 0xF8 with the sign
            assert wire[1, first] == 0x78 and wire[1, first + 1] == 0xF8 and np.count_nonzero(wire[1, :p]) == 32
        else:                                    # 2^2 = 4.0: code 6; channel 32 in the low nibble, channel 33 (negative) high
            assert wire[1, first] == (0x6 | (0xE << 4)) and wire[1, first + 1] == 0x66
    half = ex.host_encode(x, "f16")
    assert half.shape == (2, h * w * c * 2)
    assert list(half[1, (13 * c + 33) * 2:(13 * c + 33) * 2 + 2]) == [0x00, 0xFC]       # -2^20 -> -Inf = 0xFC00, little endian
    assert half.view(np.float16)[1, 13 * c + 33] == -np.inf and half.view(np.float16)[1, 13 * c + 32] == np.inf


def test_mxfp8_codes_equal_the_torch_float8_route():
    blocks = _blocks()
    code, scale = _split(ex.host_encode(_as_images(blocks), "mxfp8"), "mxfp8", blocks)
    e, finite = _scale_exponent(blocks, "mxfp8")
    assert np.array_equal(scale[finite], (e[finite] + 127).astype(np.uint8)) and (scale[~finite] == 0xFF).all()
    assert not code[~finite].any() and (~finite).sum() >= 3
    y = np.ldexp(blocks[finite].astype(np.float64), -e[finite, None]).clip(-448, 448).astype(np.float32)
    ref = torch.from_numpy(y).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    assert np.array_equal(code[finite], ref)


def test_mxfp4_codes_equal_the_brute_force_route():
    blocks = _blocks()
    code, scale = _split(ex.host_encode(_as_images(blocks), "mxfp4"), "mxfp4", blocks)
    e, finite = _scale_exponent(blocks, "mxfp4")
    assert np.array_equal(scale[finite], (e[finite] + 127).astype(np.uint8)) and (scale[~finite] == 0xFF).all()
    assert not code[~finite].any()
    v = blocks[finite]
    y = np.abs(np.ldexp(v.astype(np.float64), -e[finite, None]))          # exact: a power-of-two scaling in float64
    y = np.where(y > 6.0, 6.0, y)                                         # (rounding first would clamp the same values)
    d = np.abs(y[..., None] - E2M1)
    best = d.min(axis=-1, keepdims=True)
    near = d == best                                                      # one code, or two at a tie
    idx = np.arange(8)
    even = np.where(near & (idx % 2 == 0), idx, -1).max(axis=-1)
    anyc = np.where(near, idx, -1).max(axis=-1)
    mag = np.where(near.sum(axis=-1) == 2, even, anyc)
    ref = (mag | np.where(np.signbit(v), 8, 0)).astype(np.uint8)
    assert np.array_equal(code[finite], ref)


def test_f16_equals_numpy_astype():
    blocks = _blocks()
    wire = ex.host_encode(_as_images(blocks), "f16")
    with np.errstate(over="ignore"):
        ref = blocks.astype(np.float16)
    got = wire.view(np.float16).reshape(ref.shape)
    nan = np.isnan(ref)
    assert np.array_equal(nan, np.isnan(got)) and np.array_equal(got.view(np.uint16)[~nan], ref.view(np.uint16)[~nan])
    back = ex.host_decode(wire, "f16", 1, 1, ec.BLOCK).reshape(ref.shape)
    assert np.array_equal(back[~nan], ref.astype(np.float32)[~nan])
    edge = ec.edge_blocks()["f16_edges"]
    h = ex.host_encode(edge.reshape(1, 1, 1, -1), "f16").view(np.float16)[0]
    assert h[0] == 65504 and h[1] == 65504 and h[2] == np.inf and h[3] == -65504 and h[4] == -np.inf
    q = 2.0 ** -24
    assert h[5] == 0 and h[6] == 0 and h[7] == q and h[8] == 2 * q and h[9] == 2 * q and np.signbit(h[10]) and h[10] == 0


@pytest.mark.parametrize("fmt", ["f16", "mxfp8", "mxfp4"])
def test_roundtrip_idempotent_bounded_sign_keeping(fmt):
    blocks = _blocks()
    x = _as_images(blocks)
    once = ex.host_decode(ex.host_encode(x, fmt), fmt, 1, 1, ec.BLOCK)
    twice = ex.host_decode(ex.host_encode(once, fmt), fmt, 1, 1, ec.BLOCK)
    nan = np.isnan(once)
    assert np.array_equal(nan, np.isnan(twice))
    assert np.array_equal(once.view(np.uint32)[~nan], twice.view(np.uint32)[~nan])
    got = once.reshape(blocks.shape)
    finite = np.isfinite(blocks).all(axis=1)
    if fmt == "f16":
        return
    # a non-finite block is all NaN, a finite block has no NaN and keeps every sign bit
    assert np.isnan(got[~finite]).all() and not np.isnan(got[finite]).any()
    assert np.array_equal(np.signbit(got[finite]), np.signbit(blocks[finite]))
    m = np.abs(blocks[finite]).max(axis=1, keepdims=True).astype(np.float64)
    err = np.abs(got[finite].astype(np.float64) - blocks[finite].astype(np.float64))
    # the relative bound holds where the scale rule is not at its floor; at e = -127 (m below 2^(emax - 127): fp32's own
    # subnormal range, which E8M0 cannot follow) the error is at most half the smallest quantum the format has left
    floor = HALF_QUANTUM_AT_FLOOR[fmt]
    assert (err <= np.maximum(BOUND[fmt] * m, np.where(m < 2.0 ** (EMAX[fmt] - 127), floor, 0.0))).all()
    assert (m < 2.0 ** (EMAX[fmt] - 127)).sum() >= 4                        # the subnormal and 1e-45 edge blocks
    assert (err / np.maximum(m, 1e-300)).max() > 0.9 * BOUND[fmt]           # the clamp blocks reach the bound


def test_named_edges_decode_to_hand_derived_values():
    edges = ec.edge_blocks()

    def rt(name, fmt):
        x = edges[name].reshape(1, 1, 1, -1)
        return ex.host_decode(ex.host_encode(x, fmt), fmt, 1, 1, ec.BLOCK).reshape(-1)

    # m = 512 - 1 ulp: E = 8, e = 0; 512 is past E4M3's 448 -> clamp; 463.9 -> 448, 464 is the tie of 448 | 480 -> 480
    # (the even mantissa) -> clamp 448; 5, 6, 7 are exact
    got = rt("clamp", "mxfp8")
    assert list(got[:11]) == [448, 448, 448, 448, 448, 448, 448, 5, 6, 7, -448]
    # m = 8 - 1 ulp: E = 2, e = 0: 8 -> clamp 6; 6.9, 7, 7.1 -> 8 or the tie 6 | 8 -> 8 (even code) -> clamp 6; 5 is the tie
    # of 4 | 6 -> 4 (code 6 even), 5.1 -> 6
    got = rt("clamp_fp4", "mxfp4")
    assert list(got[:8]) == [6, 6, 6, 6, 6, 4, 6, -6]
    # E4M3 ties under e = 0 (m = 256): midpoints of the binade 2^-6 go to the even mantissa
    got = rt("ties_fp8", "mxfp8")
    q = 2.0 ** -9
    assert got[0] == 256
    assert list(got[1:9] / q) == [8, 10, 10, 12, 12, 14, 14, 16]            # 8.5, 9.5, ... 15.5 quanta
    assert list(got[17:25] / q) == [0, 2, 2, 4, 4, 6, 6, 8]                 # 0.5, 1.5, ... 7.5 quanta (subnormal codes)
    assert list(got[25:27] / q) == [0, 1]                                   # just below / above half the smallest subnormal
    got = rt("ties_fp4", "mxfp4")
    assert got[0] == 4 and list(got[1:5]) == [1.0, 2.0, 2.0, 4.0]           # 1.25, 1.75, 2.5, 3.5
    assert list(got[5:9]) == [0.0, 1.0, 0.0, 0.5]                           # 0.25, 0.75, below and above 0.25
    # signs survive a magnitude that rounds to zero, and -0
    got = rt("neg_zero", "mxfp8")
    assert got[3] == 0 and np.signbit(got[3]) and np.signbit(got[0]) and not np.signbit(got[4])
    for fmt in MX:
        for name in ("one_nan", "plus_inf", "minus_inf"):
            wire = ex.host_encode(edges[name].reshape(1, 1, 1, -1), fmt)
            p = ex.scale_offset(fmt, 1, 1, ec.BLOCK)
            assert wire[0, p] == 0xFF and not wire[0, :p].any() and not wire[0, p + 1:].any()
            assert np.isnan(rt(name, fmt)).all()
        assert not rt("zeros", fmt).any() and not np.signbit(rt("zeros", fmt)).any()
        # 1e-45 alone: m is the smallest subnormal, e = -127; the element is 2^-149 / 2^-127 = 2^-22: below half a quantum
        assert not rt("tiny", fmt).any() and np.signbit(rt("tiny", fmt)[1])
        # 3e38 = 1.76 x 2^127: E = 127, the scale byte is 127 - emax + 127
        wire = ex.host_encode(edges["huge_alone"].reshape(1, 1, 1, -1), fmt)
        assert wire[0, ex.scale_offset(fmt, 1, 1, ec.BLOCK)] == 254 - EMAX[fmt]
        assert np.isfinite(rt("huge", fmt)).all()


def _tiny_config():
    from disconet_amd import Config
    return Config(map_hw=32)


def test_detector_takes_the_format_for_disco_only():
    from disconet_amd import Detector
    cfg = _tiny_config()
    assert Detector("disco", cfg, 3, 1, device="cpu").model.exchange == "f32"
    assert Detector("disco", cfg, 3, 1, exchange="mxfp4", device="cpu").model.exchange == "mxfp4"
    for com in ("sum", "lowerbound", "late", "agent"):
        with pytest.raises(ValueError, match=com):
            Detector(com, cfg, 3, 1, exchange="mxfp8", device="cpu")
        assert Detector(com, cfg, 3, 1, exchange="f32", device="cpu").model.exchange == "f32"
    with pytest.raises(ValueError, match="int8"):
        Detector("disco", cfg, 3, 1, exchange="int8", device="cpu")


def test_model_refuses_training_unknown_formats_and_baselines():
    from disconet_amd import DiscoNet, SumFusion
    cfg = _tiny_config()
    args = (torch.zeros(3, 1, 32, 32, 13), torch.zeros(1, 3, 3, 4, 4), torch.full((1, 3), 3))
    model = DiscoNet(cfg, kd_flag=0, num_agent=3)
    assert model.exchange == "f32"
    model.exchange = "f16"
    model.train()
    with pytest.raises(NotImplementedError, match="f16"):
        model(*args, 1)
    model.eval()
    model.exchange = "int8"
    with pytest.raises(ValueError, match="int8"):
        model(*args, 1)
    base = SumFusion(cfg, kd_flag=0, num_agent=3).eval()
    base.exchange = "mxfp8"
    with pytest.raises(ValueError, match="SumFusion"):
        base(*args, 1)


def _tool(folder, name):
    for d in (os.path.join(ROOT, "tools", "det"), os.path.join(ROOT, "tools", "track")):
        if d not in sys.path:
            sys.path.insert(0, d)
    spec = importlib.util.spec_from_file_location("exchange_cli_" + name, os.path.join(ROOT, "tools", folder, name + ".py"))
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
    assert parse(mod, ["--com", "disco"]).exchange == "f32"
    assert parse(mod, ["--com", "disco", "--exchange", "mxfp4"]).exchange == "mxfp4"
    with pytest.raises(SystemExit):
        parse(mod, ["--com", "disco", "--exchange", "int8"])
    assert "int8" in capsys.readouterr().err


def test_tools_message_line_and_source_rule():
    import argparse
    common = _tool("det", "codet_common")
    from disconet_amd import Config
    line = common.exchange_line(argparse.Namespace(exchange="mxfp8", layer=3), Config("test", binary=True, only_det=True))
    assert "mxfp8" in line and "270336" in line and "1048576" in line and "32 x 32 x 256" in line
    with pytest.raises(SystemExit, match="exchange"):
        _tool("track", "eval_sort").parse_args(["--com", "disco", "--exchange", "f16"])      # --source boxes: no network
