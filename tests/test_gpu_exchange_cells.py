"""The selective feature exchange on the GPU (csrc/exchange_cells.hip, ops.exchange_encode_cells / exchange_decode_cells):
every byte of the wire -- count, index list with its 0xFFFF tail and padding, the body in each of the four formats -- and
every bit of the decoded floats against the numpy statement (disconet_amd.exchange.host_encode_cells / host_decode_cells)
on the inputs of tests/exchange_cells_cases.py; the counts; what the library refuses; a captured replay; DiscoNet.fuse with a
cell budget against disco_fuse(received=) on the host statement's maps; and the Detector with a budget.

Equality is exact.  Where a value is a NaN only its position is compared (the contract fixes no NaN payload): the binary16
code of a NaN input, and the decoded floats of a non-finite MX block.  The f32 body is a copy: there a NaN keeps its bits.

Measured (MI355X, one run, printed by test_detector_with_cells, not asserted: there is no reference for it) -- 3 agents x
batch 1, 128 x 128 maps, random weights; all 256 cells of every 16 x 16 level-3 map were non-zero; max abs deviation of the
heads from the forward that sends every cell:
    f32,   64 cells  cls 1.599e-05  loc 2.078e-05
    mxfp4, 64 cells  cls 1.587e-05  loc 2.087e-05
    f32,  256 cells  cls 0          loc 0          (asserted: every cell sent as fp32 is the map itself)
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import exchange_cells_cases as cc

pytestmark = pytest.mark.gpu

FORMATS = ("f32", "f16", "mxfp8", "mxfp4")
SHAPE_K = [((1, 1, 1, 32), 1),
           ((2, 3, 5, 64), 1), ((2, 3, 5, 64), 7), ((2, 3, 5, 64), 15),       # P no multiple of a wave; the index padding shows
           ((3, 32, 32, 256), 1), ((3, 32, 32, 256), 100),                    # K c / 8 no multiple of 64
           ((3, 32, 32, 256), 128), ((3, 32, 32, 256), 1024),                 # the bench's map and capacity; K = P
           ((1, 128, 128, 32), 5000), ((1, 128, 128, 32), 16384)]             # the LDS limit: 16 rounds of the select launch
_IDS = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else "K%d" % v  # noqa: E731


def _body_at(cells):
    return 16 + (2 * cells + 15) // 16 * 16


def _assert_wire_equal(got, want, fmt, cells):
    assert got.shape == want.shape and got.dtype == want.dtype == np.uint8
    at = _body_at(cells)
    assert np.array_equal(got[:, :at], want[:, :at])                     # count, zero words, indices, tail, padding
    if fmt == "f16":                                                     # the whole body is binary16 values
        g, w = got[:, at:].copy().view(np.float16), want[:, at:].copy().view(np.float16)
        nan = np.isnan(w)
        assert np.array_equal(np.isnan(g), nan)
        assert np.array_equal(g.view(np.uint16)[~nan], w.view(np.uint16)[~nan])
    else:
        assert np.array_equal(got[:, at:], want[:, at:])


def _assert_floats_equal(got, want):
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])


def _check(x, fmt, cells, name=""):
    """device encode and decode of x [n, h, w, c] (numpy) against the host statement; returns the host's counts"""
    from disconet_amd import exchange as ex, ops
    n, h, w, c = x.shape
    want_wire = ex.host_encode_cells(x, fmt, cells)
    sent = torch.zeros(n, dtype=torch.int64, device="cuda")
    wire = ops.exchange_encode_cells(torch.from_numpy(x).cuda(), fmt, cells, sent=sent)
    assert tuple(wire.shape) == (n, ex.cells_message_bytes(fmt, h, w, c, cells)) and wire.dtype == torch.uint8, name
    _assert_wire_equal(wire.cpu().numpy(), want_wire, fmt, cells)
    count = want_wire[:, :4].copy().view("<u4").reshape(n).astype(np.int64)
    assert sent.cpu().numpy().tolist() == count.tolist(), name
    # the decode of the HOST's wire: the kernel is checked on its own, not behind the encode kernels
    back = ops.exchange_decode_cells(torch.from_numpy(want_wire).cuda(), fmt, h, w, c, cells)
    _assert_floats_equal(back.cpu().numpy(), ex.host_decode_cells(want_wire, fmt, h, w, c, cells))
    return count


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("shape,cells", SHAPE_K, ids=_IDS)
def test_wire_and_decoded_floats_equal_the_host_statement(shape, cells, fmt):
    for name, x in cc.named_inputs(*shape, cells, seed=sum(shape) + cells).items():
        _check(x, fmt, cells, name)


def test_bench_shape_last_workgroup():
    """20 x 32 x 32 x 256, the benchmark's 5 agents x batch 4, K = 128: the last workgroup of every launch's grid"""
    x = cc.mixed(20, 32, 32, 256, 128, seed=20)
    for fmt in FORMATS:
        _check(x, fmt, 128)


def test_sent_cells_after_two_calls_is_twice_the_host_counts():
    from disconet_amd import exchange as ex, ops
    x = cc.mixed(7, 3, 5, 64, 7, seed=1)
    count = ex.host_select(x, 7)[1]
    assert len(set(count.tolist())) > 1 and 0 in count.tolist()
    t = torch.from_numpy(x).cuda()
    sent = torch.zeros(9, dtype=torch.int64, device="cuda")              # two words beyond the images stay untouched
    sent[7:] = -5
    ops.exchange_encode_cells(t, "mxfp8", 7, sent=sent)
    ops.exchange_encode_cells(t, "f32", 7, sent=sent)
    assert sent.cpu().tolist() == (2 * count).tolist() + [-5, -5]
    ops.exchange_encode_cells(t, "f16", 7)                               # sent is optional
    assert sent.cpu().tolist() == (2 * count).tolist() + [-5, -5]


@pytest.mark.parametrize("fmt", FORMATS)
def test_malformed_wires_decode_as_the_contract_says(fmt):
    from disconet_amd import exchange as ex, ops
    _, _, over, past, (h, w, c, cells) = cc.malformed_wires(fmt)
    for wire in (over, past):                                            # a count above K is clamped; an index >= P is skipped
        back = ops.exchange_decode_cells(torch.from_numpy(wire).cuda(), fmt, h, w, c, cells)
        _assert_floats_equal(back.cpu().numpy(), ex.host_decode_cells(wire, fmt, h, w, c, cells))


def test_refusals_launch_nothing():
    from disconet_amd import _lib, ops
    n, h, w, c, cells = 2, 3, 5, 64, 7
    x = torch.ones(n, h, w, c, device="cuda")
    nbytes = ops.exchange_cells_message_bytes("mxfp8", h, w, c, cells)
    canary = torch.full((n * nbytes + 16,), 0xA5, dtype=torch.uint8, device="cuda")
    maps = torch.full((n * h * w * c + 4,), -7.0, device="cuda")
    sent = torch.full((n,), 11, dtype=torch.int64, device="cuda")
    out = canary[:n * nbytes]
    with pytest.raises(_lib.DnError, match="16385"):                                      # P past the LDS limit
        ops.exchange_encode_cells(torch.ones(1, 1, 16385, 32, device="cuda"), "mxfp8", 5, out=canary, sent=sent)
    for bad in (0, h * w + 1, -2):                                                        # K outside [1, P]
        with pytest.raises(_lib.DnError):
            ops.exchange_encode_cells(x, "mxfp8", bad, out=canary, sent=sent)
    with pytest.raises(_lib.DnError, match="48"):
        ops.exchange_encode_cells(torch.ones(1, 2, 2, 48, device="cuda"), "mxfp8", 2, out=canary, sent=sent)
    with pytest.raises(_lib.DnError):                                                     # short
        ops.exchange_encode_cells(x, "mxfp8", cells, out=canary[:n * nbytes - 16], sent=sent)
    with pytest.raises(_lib.DnError, match="aligned"):                                    # long enough, not 16-byte aligned
        ops.exchange_encode_cells(x, "mxfp8", cells, out=canary[1:1 + n * nbytes], sent=sent)
    with pytest.raises(_lib.DnError, match="aligned"):                                    # feat 4 bytes off
        ops.exchange_encode_cells(torch.ones(n * h * w * c + 4, device="cuda")[1:1 + n * h * w * c].view(n, h, w, c), "mxfp8",
                                  cells, out=out, sent=sent)
    with pytest.raises(_lib.DnError):
        ops.exchange_encode_cells(x, "int8", cells, out=out, sent=sent)
    with pytest.raises(_lib.DnError):
        ops.exchange_encode_cells(x, 7, cells, out=out, sent=sent)
    with pytest.raises(_lib.DnError):
        ops.exchange_encode_cells(x.cpu(), "mxfp8", cells)
    with pytest.raises(_lib.DnError):                                                     # sent of another type / too short
        ops.exchange_encode_cells(x, "mxfp8", cells, out=out, sent=sent[:1])
    # the workspace is the wrapper's own: a short and a misaligned one through the C ABI
    lib = _lib.load()
    need = lib.dn_exchange_cells_workspace_bytes(n, h, w)
    assert need >= n * h * w * 4
    work = torch.full((need + 16,), 0x3C, dtype=torch.uint8, device="cuda")
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    fmt = ops.EXCHANGE_FORMATS["mxfp8"]
    assert lib.dn_exchange_encode_cells(ptr(x), n, h, w, c, fmt, cells, ptr(work), need - 1, ptr(out), ptr(sent), stream) != 0
    assert "workspace" in lib.dn_last_error().decode()
    assert lib.dn_exchange_encode_cells(ptr(x), n, h, w, c, fmt, cells, ptr(work[4:]), need, ptr(out), ptr(sent), stream) != 0
    assert "aligned" in lib.dn_last_error().decode()
    assert lib.dn_exchange_encode_cells(ptr(x), n, h, w, c, fmt, cells, None, need, ptr(out), ptr(sent), stream) != 0
    # decode
    wire = ops.exchange_encode_cells(x, "mxfp8", cells)
    back = maps[:n * h * w * c].view(n, h, w, c)
    with pytest.raises(_lib.DnError):                                                     # a wire of another capacity's length
        ops.exchange_decode_cells(wire, "mxfp8", h, w, c, cells + 1, out=back)
    with pytest.raises(_lib.DnError):
        ops.exchange_decode_cells(wire, "mxfp4", h, w, c, cells, out=back)
    with pytest.raises(_lib.DnError):
        ops.exchange_decode_cells(wire[:, :-16].contiguous(), "mxfp8", h, w, c, cells, out=back)
    with pytest.raises(_lib.DnError, match="aligned"):
        ops.exchange_decode_cells(canary[1:1 + n * nbytes].view(n, nbytes), "mxfp8", h, w, c, cells, out=back)
    with pytest.raises(_lib.DnError, match="aligned"):
        ops.exchange_decode_cells(wire, "mxfp8", h, w, c, cells, out=maps[1:1 + n * h * w * c].view(n, h, w, c))
    with pytest.raises(_lib.DnError):
        ops.exchange_decode_cells(wire, "mxfp8", h, w, c, 0, out=back)
    with pytest.raises(_lib.DnError):
        ops.exchange_decode_cells(wire, "mxfp8", h, w, 48, cells, out=back)
    torch.cuda.synchronize()
    assert bool((canary == 0xA5).all()) and bool((maps == -7.0).all()) and bool((work == 0x3C).all())      # nothing was written
    assert sent.cpu().tolist() == [11, 11]


@pytest.mark.parametrize("fmt", FORMATS)
def test_captured_replay_over_changed_inputs_equals_eager(fmt):
    from disconet_amd import ops
    n, h, w, c, cells = 3, 5, 7, 256, 9
    inputs = [torch.from_numpy(cc.mixed(n, h, w, c, cells, seed=s)).cuda() for s in (31, 32, 33)]
    eager = []
    for t in inputs:
        sent = torch.zeros(n, dtype=torch.int64, device="cuda")
        wire = ops.exchange_encode_cells(t, fmt, cells, sent=sent)
        eager.append((wire.clone(), ops.exchange_decode_cells(wire, fmt, h, w, c, cells).clone(), sent))
    x = inputs[0].clone()
    wire = torch.empty_like(eager[0][0])
    back = torch.empty_like(x)
    sent = torch.zeros(n, dtype=torch.int64, device="cuda")

    def run():
        ops.exchange_decode_cells(ops.exchange_encode_cells(x, fmt, cells, out=wire, sent=sent), fmt, h, w, c, cells, out=back)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run()
    sent.zero_()
    total = torch.zeros_like(sent)
    for t, (want_wire, want_back, want_sent) in zip(inputs, eager):
        x.copy_(t)
        wire.fill_(0x5A)
        back.fill_(-7.0)
        g.replay()
        torch.cuda.synchronize()
        _assert_wire_equal(wire.cpu().numpy(), want_wire.cpu().numpy(), fmt, cells)
        _assert_floats_equal(back.cpu().numpy(), want_back.cpu().numpy())
        total += want_sent
        assert torch.equal(sent, total)                                  # the counts advance with every replay


def test_roundtrip_without_cells_is_todays_call_and_with_cells_the_host_statement():
    from disconet_amd import exchange as ex, ops
    n, h, w, c, cells = 3, 5, 7, 256, 9
    x = cc.mixed(n, h, w, c, cells, seed=5)
    t = torch.from_numpy(x).cuda()
    assert ex.roundtrip(t, "f32") is t and ex.roundtrip(t, "f32", cells=0) is t and ex.roundtrip(t, "f32", 0, None) is t
    for fmt in FORMATS[1:]:
        want = ops.exchange_decode(ops.exchange_encode(t, fmt), fmt, h, w, c).cpu().numpy()
        _assert_floats_equal(ex.roundtrip(t, fmt, cells=0).cpu().numpy(), want)
        _assert_floats_equal(ex.roundtrip(t, fmt).cpu().numpy(), want)
    for fmt in FORMATS:
        sent = torch.zeros(n, dtype=torch.int64, device="cuda")
        got = ex.roundtrip(t, fmt, cells=cells, sent=sent)
        assert got is not t and got.shape == t.shape
        _assert_floats_equal(got.cpu().numpy(), ex.host_decode_cells(ex.host_encode_cells(x, fmt, cells), fmt, h, w, c, cells))
        assert sent.cpu().tolist() == ex.host_select(x, cells)[1].tolist()
    with pytest.raises(ValueError, match="int8"):
        ex.roundtrip(t, "int8", cells=cells)


# ---------------------------------------------------------------------------------------------
# DiscoNet.fuse with a cell budget
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["f32", "mxfp4"])
@pytest.mark.parametrize("one_launch", [True, False], ids=["fuse_mlp", "mlp_g_tail"])
def test_fuse_with_cells_equals_received_of_the_host_statement(one_launch, fmt):
    """3 agents x batch 1 with a dead slot: the eval forward's fusion with exchange_cells = K is disco_fuse(received=) on the
    maps the host statement decodes"""
    from disconet_amd import Config, DiscoNet, exchange as ex, ops
    from disconet_amd.synthetic import make_scene_batch, randomize_bn_stats
    A, B, K = 3, 1, 40
    torch.manual_seed(3)
    m = DiscoNet(Config(map_hw=128), kd_flag=0, num_agent=A).eval()
    randomize_bn_stats(m)
    m.fuse_mlp = one_launch
    m.cuda()
    P = m._get_plan()
    assert ("_fuse_mlp" in P) == one_launch
    _, trans, na = make_scene_batch(B, A, 128, live=[2], jitter_seed=9)
    trans = trans.cuda().float().contiguous()
    num_agent = na[:, 0].to(torch.int32).cuda()
    x = cc.relu_map(A * B, 16, 16, 256, seed=4)
    feat = torch.from_numpy(x).cuda()
    sp_out = m.conv_math == "sp"
    plain = ops.as_nhwc(m.fuse(feat, trans, num_agent, B, P, sp_out=sp_out))
    m.exchange, m.exchange_cells = fmt, K
    got = ops.as_nhwc(m._fuse_exchanged(feat, trans, num_agent, B, P))
    received = torch.from_numpy(ex.host_decode_cells(ex.host_encode_cells(x, fmt, K), fmt, 16, 16, 256, K)).cuda()
    want = ops.as_nhwc(m.fuse(feat, trans, num_agent, B, P, sp_out=sp_out, received=received))
    assert got.shape == want.shape == (A * B, 16, 16, 256)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert not torch.equal(got, plain)                                   # the budget changed what some ego received
    count = ex.host_select(x, K)[1]
    assert m.exchange_sent.cpu().tolist() == count.tolist() + [1]
    m._fuse_exchanged(feat, trans, num_agent, B, P)
    assert m.exchange_sent.cpu().tolist() == (2 * count).tolist() + [2]
    assert m.exchange_sent_summary()["cells_per_image"] == count.tolist()
    m.exchange_cells = 16 * 16 + 1
    with pytest.raises(ValueError, match="exchange_cells = 257.*P = 256"):
        m(torch.zeros(A * B, 1, 128, 128, 13, device="cuda"), trans, na.cuda(), B)


# ---------------------------------------------------------------------------------------------
# Detector(exchange_cells=)
# ---------------------------------------------------------------------------------------------
def _detector_setup():
    from disconet_amd import Config
    from disconet_amd.synthetic import make_scene_batch
    return Config(map_hw=128), tuple(t.cuda() for t in make_scene_batch(1, 3, 128, jitter_seed=5))


def _watch_exchanged_map(det):
    """-> the list that collects a copy of the level-3 map of every fusion call of det's model"""
    seen, fuse = [], det.model.fuse

    def watched(feat, *args, **kw):
        seen.append(feat.clone())
        return fuse(feat, *args, **kw)

    det.model.fuse = watched
    return seen


def test_detector_with_cells(capsys):
    from disconet_amd import Detector, exchange as ex, ops
    cfg, inputs = _detector_setup()
    base = Detector("disco", cfg, 3, 1, pre_nms_top_k=64)
    want = {k: v.clone() for k, v in base.forward(*inputs).items()}
    ops.drain_sp_range()
    zero = Detector("disco", cfg, 3, 1, pre_nms_top_k=64, exchange_cells=0)
    got = zero.forward(*inputs)
    assert zero.model.exchange_sent is None
    for k in ("cls", "loc"):                     # cells = 0: the bits of a detector built without the argument
        assert torch.equal(got[k].view(torch.int32), want[k].view(torch.int32))
    ops.drain_sp_range()
    for fmt, cells in (("f32", 64), ("mxfp4", 64), ("f32", 256)):
        det = Detector("disco", cfg, 3, 1, pre_nms_top_k=64, exchange=fmt, exchange_cells=cells)
        assert det.model.exchange_cells == cells and det.model.exchange == fmt
        seen = _watch_exchanged_map(det)
        got = det.forward(*inputs)
        again = det.forward(*inputs)             # the range guard of the first forward raises here, if it found anything
        ops.drain_sp_range()
        for k in ("cls", "loc"):
            assert got[k].shape == want[k].shape and bool(torch.isfinite(got[k]).all()) and torch.equal(got[k], again[k])
        assert len(seen) == 2 and tuple(seen[0].shape) == (3, 16, 16, 256)
        score = ex.host_scores(seen[0].cpu().numpy())
        count = ex.host_select(seen[0].cpu().numpy(), cells)[1]
        assert det.model.exchange_sent.cpu().tolist() == (2 * count).tolist() + [2]
        with capsys.disabled():
            print("\nexchange %-5s cells %3d: non-zero cells of the 256 per image %s, sent %s; max |cls - all cells| %.3e, "
                  "max |loc - all cells| %.3e" % (fmt, cells, (score > 0).sum(axis=1).tolist(), count.tolist(),
                                                  float((got["cls"] - want["cls"]).abs().max()),
                                                  float((got["loc"] - want["loc"]).abs().max())), end="")
        if (fmt, cells) == ("f32", 256) and bool((score > 0).all()):
            for k in ("cls", "loc"):             # every cell sent in f32: what the neighbours receive is the map itself
                assert torch.equal(got[k].view(torch.int32), want[k].view(torch.int32))


def test_detector_with_cells_as_a_captured_step():
    from disconet_amd import Detector, exchange as ex, graph
    cfg, inputs = _detector_setup()
    det = Detector("disco", cfg, 3, 1, pre_nms_top_k=64, exchange="mxfp8", exchange_cells=100)
    seen = _watch_exchanged_map(det)
    eager = {k: v.clone() for k, v in det(*inputs).items()}
    assert int(eager["count"].sum()) > 0
    count = ex.host_select(seen[0].cpu().numpy(), 100)[1]
    assert det.model.exchange_sent.cpu().tolist() == count.tolist() + [1]
    step = graph.GraphedStep(lambda: det(*inputs))
    before = det.model.exchange_sent.clone()
    replayed = step()
    torch.cuda.synchronize()
    for k, v in eager.items():
        assert torch.equal(replayed[k].view(torch.int32), v.view(torch.int32)), k
    after = det.model.exchange_sent.cpu()
    assert (after - before.cpu()).tolist() == count.tolist() + [1]       # one replay: one frame more, its cells
    assert after[:3].tolist() == (int(after[3]) * count).tolist()
    step()
    torch.cuda.synchronize()
    assert (det.model.exchange_sent.cpu() - after).tolist() == count.tolist() + [1]
    step.drain()
