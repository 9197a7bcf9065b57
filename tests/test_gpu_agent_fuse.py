"""`--com agent` on the GPU: ops.agent_fuse (the score epilogue of csrc/fuse_mlp.hip + csrc/agent_fuse.hip), the training
step's list kernels, the model class, one training step and the tools, against the float64 / fp32 twins of
tests/agent_fusion_ref.py.

Bounds (no absolute constant is invented here).  E_w = max |fp32 twin's weights - float64 twin's weights| on the test's own
inputs, FACTOR = 4 (tests/reduce_fusion_ref.py, tests/test_gpu_fusion_fp64.py: the kernels warp and contract in another order
than torch):
    scalar weights   |w - w64| <= FACTOR E_w
    fused maps       |fused - fused64| <= TOL + FACTOR E_w max sum_k |map_k|          (TOL = 1e-4, test_gpu_fusion_fp64.py's bar)
The parameters (agent_fusion_ref.set_params: seed 2, gain 12, picked on the CPU from the float64 twin alone) make every live
ego with two or more entries spread its weights by at least 0.05 with at most one scalar clamped -- asserted in each test
before the GPU is touched, so `--com mean` cannot pass.  Exact where exactness is promised: padded egos and lists of one
entry, agents == 1, every wave layout of the score launch, two runs, an ego sub-range, a captured replay, the list kernels
against torch's fp32 loop on the kernel's own weights.

Measured (MI355X, one run; E_w on the CPU; err = max |kernel - float64|, the same in every wave layout):

A x B  h x w x C      E_w        weights err (bound)     fused err (bound)
3 x 1  8 x 8 x 64     5.878e-07  2.979e-07 (2.351e-06)   1.197e-06 (1.123e-04)
4 x 2  12 x 16 x 128  7.482e-07  3.867e-07 (2.993e-06)   1.653e-06 (1.156e-04)
5 x 2  32 x 32 x 256  3.075e-06  1.052e-06 (1.230e-05)   4.404e-06 (1.981e-04)
8 x 1  32 x 32 x 256  3.745e-06  1.038e-06 (1.498e-05)   4.430e-06 (2.256e-04)
3 x 1  6 x 5 x 64     4.152e-07  1.280e-07 (1.661e-06)   3.421e-07 (1.081e-04)
model vs twin: at most 1.5e-05 on any output (cfg1_f1 and ragged_a4, f32 and sp); list kernels: |w - host| <= 1.5e-08.
"""
import os
import subprocess
import sys
import types

import pytest
import torch

from tests import agent_fusion_ref as ar
from tests import cases

pytestmark = pytest.mark.gpu
TOL = ar.TOL


def _dev():
    return torch.device("cuda:0")


def _report(title, rows):
    print("\n" + title)
    for r in rows:
        print("    " + r)


def _packed(net, C, dev):
    """the weight net on the device and its packed form (model.fuse_mlp_params_of) + conv1_5"""
    import copy
    from disconet_amd.model import fuse_mlp_params_of
    gpu = copy.deepcopy(net).to(dev).eval()
    params, keep = fuse_mlp_params_of(gpu, C)
    return params, keep, gpu.conv1_5.weight.detach().contiguous(), gpu.conv1_5.bias.detach().contiguous()


# ---------------------------------------------------------------------------------------------
# a. the op
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ar.SHAPES, ids=str)
def test_agent_fuse_vs_float64(shape):
    """every wave layout of the score launch (default, 1, 2, 4) against the float64 twin; all layouts, a second run, the
    pixel-major form of the warped maps and an ego sub-range give the default's bits; padded egos and lists of one entry
    return the ego's bits.  6 x 5 (h w = 30): DiscoNet.fuse serves that size at C = 64, so does this (no fragment-major form)."""
    from disconet_amd import ops
    A, B, h, w, C, _, v2i = shape
    net, feat, trans, live, ref = ar.make_case(shape)
    assert A == 1 or (ref.tells_agent_from_mean() and ref.E_w > 0), (ref.spread, ref.clamped)      # on the CPU, before any launch
    dev = _dev()
    params, keep, w5, b5 = _packed(net, C, dev)
    x = ar.nhwc(feat).to(dev)
    t, na = trans.to(dev), torch.tensor(live, dtype=torch.int32, device=dev)
    w64, f64_ = ref.weights[torch.float64], ar.nhwc(ref.fused[torch.float64])
    rows, bad, first = [], [], None
    try:
        for waves in (0, 1, 2, 4, 0):
            ops.set_fuse_mlp_waves(waves)
            fused, weights = ops.agent_fuse(x, t, na, params, w5, b5, B, A, v2i, want_weights=True)
            torch.cuda.synchronize()
            err_w = (weights.cpu().double() - w64).abs().max().item()
            err_f = (fused.cpu().double() - f64_).abs().max().item()
            rows.append("%-22s waves=%d E_w = %.3e  weights %.3e (bound %.3e)  fused %.3e (bound %.3e)" % (
                "%dx%d %dx%dx%d" % (A, B, h, w, C), waves, ref.E_w, err_w, ref.weight_bound(), err_f, ref.fused_bound()))
            if err_w > ref.weight_bound() or err_f > ref.fused_bound():
                bad.append(rows[-1])
            if first is None:
                first = (fused, weights)
            else:
                assert torch.equal(fused, first[0]) and torch.equal(weights, first[1]), "waves=%d differs from the default" % waves
    finally:
        ops.set_fuse_mlp_waves(0)
    _report("agent fuse", rows)
    assert not bad, bad
    fused, weights = first
    if A > 1:
        pm = ops.agent_fuse(x, t, na, params, w5, b5, B, A, v2i, fm=False)
        assert torch.equal(pm, fused), "pixel-major warped maps give other bits than the fragment-major form"
        # mean fusion would miss: its weights sit 1 / len from these
        assert max(ref.spread.values()) >= 0.05
    if A >= 3:
        part, pw = ops.agent_fuse(x, t, na, params, w5, b5, B, A, v2i, want_weights=True, ego_first=1, ego_count=2)
        assert torch.equal(part, fused[B:3 * B]) and torch.equal(pw, weights[:, 1:3])
    n_pass = 0
    for b, i, js in ar.lists_of(live, A, B, v2i):
        n_live = max(0, min(live[b], A))
        if i >= n_live:
            assert torch.equal(fused[i * B + b], x[i * B + b]) and float(weights[b, i].abs().max()) == 0.0
            n_pass += 1
        elif not js:
            assert torch.equal(fused[i * B + b], x[i * B + b]) and weights[b, i].tolist() == [1.0] + [0.0] * (A - 1)
            n_pass += 1
    assert n_pass > 0 or live == [A] * B


def test_graph_replay_equals_eager_and_refusals():
    from disconet_amd import ops
    from disconet_amd._lib import DnError
    shape = ar.SHAPES[1]
    A, B, h, w, C, _, v2i = shape
    net, feat, trans, live, ref = ar.make_case(shape)
    dev = _dev()
    params, keep, w5, b5 = _packed(net, C, dev)
    x, t, na = ar.nhwc(feat).to(dev), trans.to(dev), torch.tensor(live, dtype=torch.int32, device=dev)
    with pytest.raises(DnError, match="ego range"):
        ops.agent_fuse(x, t, na, params, w5, b5, B, A, v2i, ego_first=3, ego_count=2)
    with pytest.raises(ValueError, match="conv1_5"):
        ops.agent_fuse(x, t, na, params, w5[..., :8].contiguous(), b5, B, A, v2i)
    with pytest.raises(DnError, match="channels unsupported"):
        ops.agent_fuse(torch.zeros(A * B, h, w, 96, device=dev), t, na, params, w5, b5, B, A, v2i)
    eager, ew = ops.agent_fuse(x, t, na, params, w5, b5, B, A, v2i, want_weights=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.agent_fuse(x, t, na, params, w5, b5, B, A, v2i, want_weights=True)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, ow = ops.agent_fuse(x, t, na, params, w5, b5, B, A, v2i, want_weights=True)
    out.zero_()
    ow.zero_()
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager) and torch.equal(ow, ew)


# ---------------------------------------------------------------------------------------------
# b. the list kernels of the training step
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw,c", [((8, 8), 64), ((5, 7), 36)])
def test_list_kernels_are_exact(hw, c):
    """lists of 1 (one of them an ego that is not live: no logit), 2, 5 and 16 maps scattered over the buffer, outputs in
    reverse order, dfused a channel slice.  fused = torch's fp32 loop (the first product, then product by product) on the
    KERNEL'S OWN weights, bit for bit; dmaps rows = w_k * dfused, bit for bit; a list of one returns its map's bits.  The
    weights themselves: the host statement's scalars are the kernel's bit for bit (one order of every sum), expf and torch.exp
    may each be 1 ulp off and the sum and the quotient round once each: |w - host| <= 8 * 2^-24 (w <= 1)."""
    from disconet_amd import train_ops as T
    from disconet_amd.fusion_modes import agent_scalar, agent_softmax, weighted_sum
    dev = _dev()
    lengths = [1, 2, 5, 16, 1, 3]
    n = sum(lengths)
    g = torch.Generator().manual_seed(c)
    image = torch.randperm(n, generator=g).tolist()
    first = [0]
    for k in lengths:
        first.append(first[-1] + k)
    ego_out = list(range(len(lengths)))[::-1]
    pair = list(image)
    pair[first[4]] = -1                                   # the second list of one: an ego that is not live
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)
    npx = hw[0] * hw[1]
    maps = torch.randn(n, hw[0], hw[1], c, generator=g)
    z4 = torch.randn(n, hw[0], hw[1], 1, generator=g)
    w5 = (torch.rand(1, 1, hw[0], hw[1], generator=g) + 0.5) * (12.0 / npx)
    b5 = torch.tensor([0.25])
    wide = torch.randn(len(lengths), hw[0], hw[1], c + 12, generator=g).to(dev)
    dfused = wide[..., 8:8 + c]
    fused = torch.full((len(lengths), hw[0], hw[1], c), 7.0, device=dev)
    weights = T.agent_combine_lists(z4.to(dev), w5.to(dev), b5.to(dev), maps.to(dev), i32(first), i32(pair), i32(image),
                                    i32(ego_out), fused)
    dmaps = torch.full((n, hw[0], hw[1], c), 7.0, device=dev)
    T.agent_combine_lists_backward(dfused, weights, maps.to(dev), i32(first), i32(image), i32(ego_out), dmaps)
    torch.cuda.synchronize()
    wk, worst = weights.cpu(), 0.0
    for e, length in enumerate(lengths):
        ks = list(range(first[e], first[e + 1]))
        own = [maps[image[k]] for k in ks]
        assert torch.equal(fused[ego_out[e]].cpu(), weighted_sum(own, wk[ks])), e
        if length == 1:
            assert wk[ks[0]].item() == 1.0 and torch.equal(fused[ego_out[e]].cpu(), own[0])
        else:
            a = torch.stack([agent_scalar(z4[pair[k]].clamp(min=0), w5, b5) for k in ks])
            assert int((a > 0).sum()) >= 2
            worst = max(worst, (wk[ks] - agent_softmax(a)).abs().max().item())
            assert float(wk[ks].max() - wk[ks].min()) > 0.05
        for k in ks:
            assert torch.equal(dmaps[image[k]], dfused[ego_out[e]] * weights[k]), (e, k)
    print("\nagent list kernels %dx%dx%d: max |w - host| = %.3e (bound %.3e)" % (hw[0], hw[1], c, worst, 8 * 2.0 ** -24))
    assert worst <= 8 * 2.0 ** -24


# ---------------------------------------------------------------------------------------------
# c. the model
# ---------------------------------------------------------------------------------------------
_REF = {}


def _ref_outputs(case):
    if case not in _REF:
        c = cases.MODEL_CASES[case]
        ref = ar.build_agent_ref(c["map_hw"], c["agents"], kd_flag=1)
        bevs, trans, na = cases.model_inputs(case)
        with torch.no_grad():
            res, x8, x7, x6, x5, fused = ref(bevs, trans, na, c["batch"])
        _REF[case] = (ref, {"cls": res["cls"], "loc": res["loc"], "x8": x8, "x5": x5, "fused": fused})
    return _REF[case]


@pytest.mark.parametrize("math", ["f32", "sp"])
@pytest.mark.parametrize("case", ["cfg1_f1", "ragged_a4"])
def test_model_vs_twin(case, math):
    """the acceptance rule of tests/test_gpu_fuse_reduce.py :: test_models_vs_twin: every output within TOL of the fp32 twin"""
    from disconet_amd import AgentWeightedFusion, Config, build_model
    c = cases.MODEL_CASES[case]
    ref, want = _ref_outputs(case)
    m = build_model("agent", Config(map_hw=c["map_hw"]), kd_flag=1, num_agent=c["agents"]).eval()
    m.conv_math = math
    m.load_state_dict({"module." + k: v for k, v in ref.state_dict().items()})
    m = m.cuda()
    assert type(m) is AgentWeightedFusion
    bevs, trans, na = cases.model_inputs(case)
    with torch.no_grad():
        res, x8, x7, x6, x5, fused = m(bevs.cuda(), trans.cuda(), na.cuda(), c["batch"])
    torch.cuda.synchronize()
    got = {"cls": res["cls"].cpu(), "loc": res["loc"].cpu(), "x8": x8.cpu(), "x5": x5.cpu(), "fused": fused.cpu()}
    rows = []
    for name in want:
        assert got[name].shape == want[name].shape, name
        rows.append("%s max abs err %.3e" % (name, (got[name] - want[name]).abs().max().item()))
    _report("agent model %s %s" % (case, math), rows)
    for name in want:
        err = (got[name] - want[name]).abs().max().item()
        assert err <= TOL, "%s/%s %s max abs err %.3e" % (case, math, name, err)


# ---------------------------------------------------------------------------------------------
# d. one training step
# ---------------------------------------------------------------------------------------------
def test_one_training_step_vs_twin(monkeypatch):
    """the smallest training case against the twin's autograd step (the twin detaches the weights, as upstream): losses within
    2e-5 relative, every backbone gradient under tests/test_gpu_train_step.py :: _assert_grads against float64 autograd; the
    weight net's parameters keep their bits (Adam with weight decay runs over the trained parameters only); its BatchNorms'
    running statistics equal the twin's within that file's bound and their call counters advanced once per call"""
    from disconet_amd import AgentTrainEngine, CoDetModule, Config, build_model
    from oracle.train_ref import train_step
    from tests.test_gpu_train_step import _assert_grads, _fp64_grads, _grad_report
    case = "cfg1"
    c = cases.TRAIN_CASES[case]
    (bevs, trans, na), (labels, targets, mask) = cases.train_inputs(case)
    ref = ar.build_agent_ref(c["map_hw"], c["agents"], kd_flag=0)
    model = build_model("agent", Config(map_hw=c["map_hw"]), kd_flag=0, num_agent=c["agents"])
    model.load_state_dict(ref.state_dict())
    model = model.cuda()
    g64 = _fp64_grads(ref, (bevs, trans, na), (labels, targets, mask), c["batch"], monkeypatch)
    assert g64 and not any(n.startswith("agent_weighted_fusion.") for n in g64)      # the twin never trains the weight net
    calls0 = int(ref.agent_weighted_fusion.bn1_1.num_batches_tracked)
    opt = torch.optim.Adam(ref.parameters(), lr=1e-3, weight_decay=1e-2)
    l_ref = train_step(ref, opt, bevs, trans, na, c["batch"], labels, targets, mask)
    n_calls = int(ref.agent_weighted_fusion.bn1_1.num_batches_tracked) - calls0
    assert n_calls == c["agents"] ** 2                    # one call per entry of every ego's list
    mod = CoDetModule(model, optimizer=torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=1e-2))
    assert type(mod.engine) is AgentTrainEngine and mod.engine.weight_decay == 1e-2
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    data = {"bev_seq": bevs.cuda(), "trans_matrices": trans.cuda(), "num_agent": na.cuda(),
            "labels": labels.cuda(), "reg_targets": targets.cuda(), "reg_loss_mask": mask.cuda()}
    out = mod.step(data, c["batch"])
    print("\nagent %s: losses %s, twin %s" % (case, out, l_ref))
    assert abs(out["cls_loss"] - l_ref[0]) < 2e-5 * abs(l_ref[0]), (out, l_ref)
    assert abs(out["loc_loss"] - l_ref[1]) < 2e-5 * abs(l_ref[1]), (out, l_ref)
    backbone = types.SimpleNamespace(named_parameters=lambda: [(n, p) for n, p in model.named_parameters() if n in g64])
    _assert_grads(_grad_report(g64, ref, mod.engine, backbone))
    moved = 0
    for n, p in model.named_parameters():
        if n.startswith("agent_weighted_fusion."):
            assert torch.equal(p.detach(), before[n]), n                     # not stepped at all, weight decay included
            assert float(mod.engine.g(p).abs().max()) == 0.0, n              # and no gradient entered the weight net
        elif n in g64:
            moved += int(not torch.equal(p.detach(), before[n]))
    assert moved > 0.9 * len(g64)
    ref_buf = dict(ref.named_buffers())
    for name, b in model.named_buffers():
        r = ref_buf[name]
        if name.endswith("num_batches_tracked"):
            assert int(b) == int(r), name
        else:
            assert float((b.cpu() - r).abs().max()) < 1e-4 * max(float(r.abs().max()), 1.0), name
    assert int(model.agent_weighted_fusion.bn1_3.num_batches_tracked) - calls0 == n_calls


def test_training_refuses_distillation_and_an_agent_shard():
    from disconet_amd import CoDetModule, Config, TeacherNet, build_model
    from disconet_amd.sharded import AgentShard
    model = build_model("agent", Config(map_hw=128), kd_flag=0, num_agent=2).cuda()
    with pytest.raises(ValueError, match="DiscoGraph"):
        CoDetModule(model, teacher=TeacherNet(Config(map_hw=128)).cuda(), kd_flag=1)
    shard = AgentShard.__new__(AgentShard)      # (never used: the engine refuses before it looks at it)
    with pytest.raises(NotImplementedError, match="--com agent"):
        CoDetModule(model, shard=shard)


# ---------------------------------------------------------------------------------------------
# e. the tools
# ---------------------------------------------------------------------------------------------
def _run(args, timeout):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable] + args, cwd=root, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def test_tools_train_and_evaluate_the_mode(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    logs = str(tmp_path / "logs")
    out = _run([os.path.join(root, "tools", "det", "train_codet.py"), "--com", "agent", "--targets", "boxes", "--num_agent", "2",
                "--batch", "1", "--nepoch", "1", "--steps_per_epoch", "3", "--logpath", logs], 300)
    assert "epoch 1:" in out
    ck = torch.load(os.path.join(logs, "epoch_1.pth"), map_location="cpu", weights_only=False)
    keys = ck["model_state_dict"]
    assert "agent_weighted_fusion.conv1_5.weight" in keys and not any(k.startswith("pixel_weighted_fusion") for k in keys)
    out = _run([os.path.join(root, "tools", "det", "eval_codet.py"), "--com", "agent", "--gt", "scene", "--num_agent", "2",
                "--resume", os.path.join(logs, "epoch_1.pth")], 300)
    assert "overall:" in out
