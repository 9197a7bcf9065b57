"""The feature-exchange wire format on the GPU (csrc/exchange.hip, ops.exchange_encode / exchange_decode): every byte of
the wire -- payload, scale bytes, zero padding -- and every bit of the decoded floats against the numpy statement
(disconet_amd.exchange.host_encode / host_decode) on the inputs of tests/exchange_cases.py; what the library refuses; a
captured replay; disco_fuse's `received` against the call it must equal; and the Detector with a format.

Equality is exact.  Where a value is a NaN only its position is compared (the contract fixes no NaN payload): the binary16
code of a NaN input, and the decoded floats of a non-finite MX block.

Measured (MI355X, one run, printed by test_detector_with_a_format, not asserted: there is no reference for it) -- max abs
deviation of the heads from the f32 forward, 3 agents x batch 1, 128 x 128 maps, random weights (max |cls| 0.183, max |loc|
0.241):
    f16    cls 5.960e-08  loc 7.451e-08
    mxfp8  cls 8.941e-07  loc 9.835e-07
    mxfp4  cls 1.688e-06  loc 3.472e-06
"""
import numpy as np
import pytest
import torch

from tests import exchange_cases as ec

pytestmark = pytest.mark.gpu

FORMATS = ("f16", "mxfp8", "mxfp4")
SHAPES = [(2, 1, 1, 32),            # one block per image
          (1, 3, 5, 64),
          (3, 5, 7, 256),           # 35 pixels: no multiple of any lane grouping
          (2, 2, 3, 512),
          (len(ec.edge_blocks()), 1, 1, 32)]      # every edge block as a one-block image of its own


def _assert_wire_equal(got, want, fmt):
    assert got.shape == want.shape and got.dtype == want.dtype == np.uint8
    if fmt == "f16":                 # the whole message is binary16 values
        g, w = got.view(np.float16), want.view(np.float16)
        nan = np.isnan(w)
        assert np.array_equal(np.isnan(g), nan)
        assert np.array_equal(g.view(np.uint16)[~nan], w.view(np.uint16)[~nan])
    else:
        assert np.array_equal(got, want)


def _assert_floats_equal(got, want):
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])


def _check(x, fmt):
    """device encode and decode of x [n, h, w, c] (numpy) against the host statement; returns the device wire"""
    from disconet_amd import exchange as ex, ops
    n, h, w, c = x.shape
    want_wire = ex.host_encode(x, fmt)
    wire = ops.exchange_encode(torch.from_numpy(x).cuda(), fmt)
    assert tuple(wire.shape) == (n, ex.message_bytes(fmt, h, w, c)) and wire.dtype == torch.uint8
    _assert_wire_equal(wire.cpu().numpy(), want_wire, fmt)
    # the decode of the HOST's wire: the kernel is checked on its own, not behind the encode kernel
    back = ops.exchange_decode(torch.from_numpy(want_wire).cuda(), fmt, h, w, c)
    _assert_floats_equal(back.cpu().numpy(), ex.host_decode(want_wire, fmt, h, w, c))
    return wire


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_wire_and_decoded_floats_equal_the_host_statement(shape, fmt):
    n, h, w, c = shape
    if shape[1:] == (1, 1, 32) and n > 2:
        x = ec.edge_array().reshape(shape)
    else:
        x = ec.tensor_with_edges(n, h, w, c, seed=sum(shape))
    _check(x, fmt)
    _check(np.abs(x), fmt)          # non-negative, as after a ReLU (|NaN| stays a NaN)


def test_bench_shape_last_workgroup():
    """20 x 32 x 32 x 256, the benchmark's 5 agents x batch 4: 10240 waves, the grid's last workgroup included"""
    x = ec.tensor_with_edges(20, 32, 32, 256, seed=20)
    for fmt in FORMATS:
        _check(x, fmt)


def test_roundtrip_is_the_host_roundtrip_and_f32_is_the_identity():
    from disconet_amd import exchange as ex
    x = ec.tensor_with_edges(3, 5, 7, 256, seed=5)
    t = torch.from_numpy(x).cuda()
    assert ex.roundtrip(t, "f32") is t
    for fmt in FORMATS:
        got = ex.roundtrip(t, fmt)
        assert got is not t and got.shape == t.shape
        _assert_floats_equal(got.cpu().numpy(), ex.host_decode(ex.host_encode(x, fmt), fmt, 5, 7, 256))
    with pytest.raises(ValueError, match="int8"):
        ex.roundtrip(t, "int8")


def test_refusals_launch_nothing():
    from disconet_amd import _lib, ops
    x = torch.ones(2, 3, 5, 64, device="cuda")
    nbytes = ops.exchange_message_bytes("mxfp8", 3, 5, 64)
    canary = torch.full((2 * nbytes + 16,), 0xA5, dtype=torch.uint8, device="cuda")
    with pytest.raises(_lib.DnError):                                        # short
        ops.exchange_encode(x, "mxfp8", out=canary[:2 * nbytes - 16])
    with pytest.raises(_lib.DnError, match="aligned"):                       # long enough, not 16-byte aligned
        ops.exchange_encode(x, "mxfp8", out=canary[1:1 + 2 * nbytes])
    with pytest.raises(_lib.DnError, match="48"):
        ops.exchange_encode(torch.ones(1, 2, 2, 48, device="cuda"), "mxfp8")
    with pytest.raises(_lib.DnError):
        ops.exchange_encode(x, "int8")
    with pytest.raises(_lib.DnError):
        ops.exchange_encode(x, 7)
    with pytest.raises(_lib.DnError):                                        # the identity has no launch
        ops.exchange_encode(x, "f32", out=torch.empty(2, 3 * 5 * 64 * 4, dtype=torch.uint8, device="cuda"))
    with pytest.raises(_lib.DnError):
        ops.exchange_encode(x.cpu(), "mxfp8")
    wire = ops.exchange_encode(x, "mxfp8")
    with pytest.raises(_lib.DnError):                                        # a wire of another shape's length
        ops.exchange_decode(wire[:, :-16].contiguous(), "mxfp8", 3, 5, 64)
    with pytest.raises(_lib.DnError):
        ops.exchange_decode(wire, "mxfp4", 3, 5, 64)
    with pytest.raises(_lib.DnError, match="aligned"):
        ops.exchange_decode(canary[1:1 + 2 * nbytes].view(2, nbytes), "mxfp8", 3, 5, 64)
    with pytest.raises(_lib.DnError):
        ops.exchange_decode(wire, "mxfp8", 3, 5, 48)
    torch.cuda.synchronize()
    assert bool((canary == 0xA5).all())                                      # nothing was written


@pytest.mark.parametrize("fmt", FORMATS)
def test_captured_replay_over_changed_inputs_equals_eager(fmt):
    from disconet_amd import ops
    n, h, w, c = 3, 5, 7, 256
    inputs = [torch.from_numpy(ec.tensor_with_edges(n, h, w, c, seed=s)).cuda() for s in (31, 32, 33)]
    eager = []
    for t in inputs:
        wire = ops.exchange_encode(t, fmt)
        eager.append((wire.clone(), ops.exchange_decode(wire, fmt, h, w, c).clone()))
    x = inputs[0].clone()
    wire = torch.empty_like(eager[0][0])
    back = torch.empty_like(x)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.exchange_decode(ops.exchange_encode(x, fmt, out=wire), fmt, h, w, c, out=back)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.exchange_decode(ops.exchange_encode(x, fmt, out=wire), fmt, h, w, c, out=back)
    for t, (want_wire, want_back) in zip(inputs, eager):
        x.copy_(t)
        wire.fill_(0x5A)
        back.fill_(-7.0)
        g.replay()
        torch.cuda.synchronize()
        _assert_wire_equal(wire.cpu().numpy(), want_wire.cpu().numpy(), fmt)
        _assert_floats_equal(back.cpu().numpy(), want_back.cpu().numpy())


# ---------------------------------------------------------------------------------------------
# disco_fuse(received=)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("one_launch", [True, False], ids=["fuse_mlp", "mlp_g_tail"])
@pytest.mark.parametrize("live", [None, [2]], ids=["all_live", "dead_slot"])
def test_received_equals_the_old_call_on_a_spliced_tensor(live, one_launch):
    """the warp reads the neighbours from `received`, the attention the ego's own map from `feat`: for ego i that is the
    old call on `received` with ego i's rows taken from `feat`"""
    from disconet_amd import Config, DiscoNet
    from disconet_amd.model import disco_fuse
    from disconet_amd.synthetic import make_scene_batch, randomize_bn_stats
    A, B = 3, 1
    torch.manual_seed(3)
    m = DiscoNet(Config(map_hw=128), kd_flag=0, num_agent=A).eval()
    randomize_bn_stats(m)
    m.fuse_mlp = one_launch
    m.cuda()
    P = m._get_plan()
    assert ("_fuse_mlp" in P) == one_launch
    _, trans, na = make_scene_batch(B, A, 128, live=live, jitter_seed=9)
    trans = trans.cuda().float().contiguous()
    num_agent = na[:, 0].to(torch.int32).cuda()
    gen = torch.Generator().manual_seed(4)
    feat = torch.relu(torch.randn(A * B, 16, 16, 256, generator=gen)).cuda()
    received = (feat.cpu() * (1 + 0.25 * torch.randn(A * B, 16, 16, 256, generator=gen))).cuda().contiguous()
    plain = disco_fuse(feat, trans, num_agent, B, P, A, False)
    differs = 0
    for i in range(A):
        got = disco_fuse(feat, trans, num_agent, B, P, A, False, ego_first=i, ego_count=1, received=received)
        spliced = received.clone()
        spliced[i * B:(i + 1) * B] = feat[i * B:(i + 1) * B]
        want = disco_fuse(spliced, trans, num_agent, B, P, A, False, ego_first=i, ego_count=1)
        assert got.shape == want.shape == (B, 16, 16, 256)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), "ego %d" % i
        assert torch.equal(m.fuse(feat, trans, num_agent, B, P, ego_first=i, ego_count=1, received=received), got)
        same = torch.equal(got, plain[i * B:(i + 1) * B])
        if live is not None and i >= live[0]:
            assert same                           # a dead slot lists no neighbour: nothing it reads was received
        differs += int(not same)
    assert differs >= 1                           # some ego saw its neighbours changed: the equality above is not vacuous
    with pytest.raises(ValueError):
        disco_fuse(feat, trans, num_agent, B, P, A, False, received=received[:2])


# ---------------------------------------------------------------------------------------------
# Detector(exchange=)
# ---------------------------------------------------------------------------------------------
def _detector_setup():
    from disconet_amd import Config
    from disconet_amd.synthetic import make_scene_batch
    return Config(map_hw=128), tuple(t.cuda() for t in make_scene_batch(1, 3, 128, jitter_seed=5))


def test_detector_with_a_format(monkeypatch):
    from disconet_amd import Detector, exchange as ex, ops
    cfg, inputs = _detector_setup()
    base = Detector("disco", cfg, 3, 1, pre_nms_top_k=64)
    want = {k: v.clone() for k, v in base.forward(*inputs).items()}
    ops.drain_sp_range()
    print()
    for fmt in FORMATS:
        det = Detector("disco", cfg, 3, 1, pre_nms_top_k=64, exchange=fmt)
        assert det.model.exchange == fmt
        got = det.forward(*inputs)
        again = det.forward(*inputs)                 # the range guard of the first forward raises here, if it found anything
        ops.drain_sp_range()
        for k in ("cls", "loc"):
            assert bool(torch.isfinite(got[k]).all()) and torch.equal(got[k], again[k])
        print("exchange %-5s: max |cls - f32| %.3e (max |cls| %.3e), max |loc - f32| %.3e (max |loc| %.3e)" % (
            fmt, float((got["cls"] - want["cls"]).abs().max()), float(want["cls"].abs().max()),
            float((got["loc"] - want["loc"]).abs().max()), float(want["loc"].abs().max())))
        if fmt == "mxfp8":
            assert not (torch.equal(got["cls"], want["cls"]) and torch.equal(got["loc"], want["loc"]))
    # the format changes nothing but what the neighbours receive: with the identity in its place, the f32 bits
    det = Detector("disco", cfg, 3, 1, pre_nms_top_k=64, exchange="mxfp8")
    calls = []
    monkeypatch.setattr(ex, "roundtrip", lambda feat, fmt: calls.append(fmt) or feat)
    got = det.forward(*inputs)
    assert calls == ["mxfp8"]
    for k in ("cls", "loc"):
        assert torch.equal(got[k].view(torch.int32), want[k].view(torch.int32))


def test_detector_with_a_format_as_a_captured_step():
    from disconet_amd import Detector, graph
    cfg, inputs = _detector_setup()
    det = Detector("disco", cfg, 3, 1, pre_nms_top_k=64, exchange="mxfp8")
    eager = {k: v.clone() for k, v in det(*inputs).items()}
    assert int(eager["count"].sum()) > 0
    step = graph.GraphedStep(lambda: det(*inputs))
    replayed = step()
    torch.cuda.synchronize()
    for k, v in eager.items():
        assert torch.equal(replayed[k].view(torch.int32), v.view(torch.int32)), k
    step.drain()
