"""mAP on the GPU (dn_ap_match behind postprocess.match_ground_truth / MeanAP) against its host reference
(postprocess.host_match_ground_truth, average_precision_from_records) and the oracle's average_precision: rank, best_gt
and tp equal exactly, best_iou within 1e-11, AP equal as float64 bits -- on the seeded generator, crafted exact cases, the
shape limits, model outputs, shuffled rows, a full accumulator, a captured graph and the evaluation tool.

The 1e-11 bar on best_iou is 100 x the 1.1e-13 measured between two independent fp64 formulations of the same IoU (room
for another hypot / division on the device).  It cannot hide a wrong match: every input of these tests keeps each decision
(best IoU against a threshold, the two largest IoUs of a detection against each other) at least 1e-9 away, which is
asserted on the host reference before anything is compared.  Largest |best_iou - host| measured over this file on an
MI355X: 1.8e-12 (K = G = 1024, boxes over +-112 m), at most 1.4e-13 on every other input."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import ap_cases as A
from tests import cases
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

IOU_BAR = 1e-11
GT_SEED = 11            # make_gt_boxes seed of the model-output cases (the margins are asserted for it)


def _cuda(det, gb, gc):
    return ({k: torch.as_tensor(v).cuda() for k, v in det.items()}, torch.as_tensor(gb).cuda(), torch.as_tensor(gc).cuda())


def _np(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def _compare(det, gb, gc, what, thrs=A.THRS, margins=True):
    """match_ground_truth against host_match_ground_truth for numpy inputs; returns (device result, host result)"""
    from disconet_amd import postprocess as P
    if margins:
        A.assert_margins(det, gb, gc, what, thrs)
    want = P.host_match_ground_truth(det, gb, gc, thrs)
    d, b, c = _cuda(det, gb, gc)
    got = _np(P.match_ground_truth(d, b, c, thrs))
    err = float(np.abs(got["best_iou"] - want["best_iou"]).max(initial=0.0))
    print("%s: max |best_iou - host| = %.3g over %d rows, %d true positives at %g" % (
        what, err, int(np.asarray(det["count"]).sum()), int(want["tp"][0].sum()), thrs[0]))
    assert got["best_iou"].dtype == np.float64 and got["tp"].dtype == np.uint8
    assert np.array_equal(got["rank"], want["rank"]), what
    assert np.array_equal(got["best_gt"], want["best_gt"]), what
    assert np.array_equal(got["tp"], want["tp"]), what
    assert err <= IOU_BAR, (what, err)
    k = got["rank"].shape[1]
    past = np.arange(k)[None, :] >= np.asarray(det["count"])[:, None]
    assert (got["rank"][past] == -1).all() and (got["best_gt"][past] == -1).all()
    assert not got["best_iou"][past].any() and not got["tp"][:, past].any()
    return got, want


# ---- 4. matching ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pitch", [10.0, 3.5])
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_generator_equals_host(seed, pitch):
    dets, scs, gts = A.make(seed, pitch=pitch)
    det, gb, gc = A.padded(dets, scs, gts)
    got, want = _compare(det, gb, gc, "seed %d pitch %g" % (seed, pitch))
    assert want["tp"][0].sum() > 250 and want["tp"][1].sum() > 150
    assert (got["rank"] >= 0).sum() == det["count"].sum()
    # padding wider than the data (garbage behind count) changes nothing below count
    det_w, gb_w, gc_w = A.padded(dets, scs, gts, k=300, g=64)
    det_w["scores"][np.arange(300)[None, :] >= det_w["count"][:, None]] = 7.0
    det_w["boxes"][np.arange(300)[None, :] >= det_w["count"][:, None]] = 3.0
    wide, _ = _compare(det_w, gb_w, gc_w, "seed %d pitch %g, K = 300, G = 64" % (seed, pitch))
    k = det["scores"].shape[1]
    for name in ("rank", "best_gt", "best_iou"):
        assert np.array_equal(wide[name][:, :k], got[name]), name
    assert np.array_equal(wide["tp"][:, :, :k], got["tp"])


def test_crafted_exact_cases():
    dets, scs, gts, exp = A.crafted()
    for k, g in ((None, None), (70, 33)):
        det, gb, gc = A.padded(dets, scs, gts, k=k, g=g)
        got, want = _compare(det, gb, gc, "crafted K=%s G=%s" % (k, g), margins=False)     # exact ties are the point here
        A.check_crafted(got, exp)
        assert np.array_equal(got["best_iou"], want["best_iou"])                        # dyadic: exact on both sides
    det, gb, gc = A.padded(dets, scs, [t[:0] for t in gts])                               # no ground truth at all
    got, _ = _compare(det, gb, gc, "crafted, no ground truth", margins=False)
    assert (got["best_gt"] == -1).all() and not got["tp"].any()


def _crowd(n_rows, n_gt, seed):
    """one image: n_gt boxes on a 32 x 32 grid of pitch 7 centred on the origin (as the detector's frame is), n_rows
    detections = jittered copies in shuffled order"""
    r = np.random.default_rng(seed)
    cells = r.permutation(1024)[:n_gt]
    gt = np.zeros((n_gt, 6), np.float32)
    gt[:, 0] = (cells // 32 - 15.5) * 7.0 + r.uniform(-1, 1, n_gt)
    gt[:, 1] = (cells % 32 - 15.5) * 7.0 + r.uniform(-1, 1, n_gt)
    gt[:, 2], gt[:, 3] = r.uniform(1.6, 2.4, n_gt), r.uniform(3.5, 5.5, n_gt)
    yaw = r.uniform(-np.pi, np.pi, n_gt)
    gt[:, 4], gt[:, 5] = np.sin(yaw), np.cos(yaw)
    src = r.integers(0, n_gt, n_rows)
    d = gt[src].copy()
    d[:, :2] += r.normal(0, 0.4, (n_rows, 2)).astype(np.float32)
    d[:, 2:4] *= np.exp(r.normal(0, 0.1, (n_rows, 2))).astype(np.float32)
    y = yaw[src] + r.normal(0, 0.08, n_rows)
    d[:, 4], d[:, 5] = 0.6 * np.sin(y), 0.6 * np.cos(y)
    s = (r.permutation(n_rows).astype(np.float32) + 1) / (n_rows + 1)
    return d, s, gt


def test_limits_1024_rows_1024_boxes_and_40_images():
    d, s, gt = _crowd(1024, 1024, 5)
    d2, s2, gt2 = _crowd(17, 3, 6)
    det, gb, gc = A.padded([d, d2], [s, s2], [gt, gt2])
    assert det["scores"].shape == (2, 1024) and gb.shape == (2, 1024, 6)
    _, want = _compare(det, gb, gc, "K = G = 1024")
    assert want["tp"][0, 0].sum() > 300
    dets, scs, gts = A.make(7, n_img=40)
    det, gb, gc = A.padded(dets, scs, gts)
    _compare(det, gb, gc, "40 images")
    _compare({k: v[:1] for k, v in det.items()}, gb[:1], gc[:1], "1 image (no ground truth)")
    _compare({k: v[1:2, :1] if k != "count" else np.minimum(v[1:2], 1) for k, v in det.items()}, gb[1:2, :1],
             np.minimum(gc[1:2], 1), "K = G = 1")


def _model_det(case, k=300):
    from disconet_amd import Config, DiscoNet, postprocess as P
    from disconet_amd.synthetic import randomize_bn_stats
    c = cases.MODEL_CASES[case]
    torch.manual_seed(0)
    m = DiscoNet(Config(map_hw=c["map_hw"]), kd_flag=0, num_agent=c["agents"])
    randomize_bn_stats(m)
    m.eval().cuda()
    bevs, trans, na = cases.model_inputs(case)
    with torch.no_grad():
        out = m(bevs.cuda(), trans.cuda(), na.cuda(), c["batch"])
    return P.detect(out[0] if isinstance(out, tuple) else out, P.make_anchors(Config(map_hw=c["map_hw"])), pre_nms_top_k=k)


@pytest.mark.parametrize("case", ["cfg1_f1", "ragged_a4"])
def test_model_outputs_equal_host(case):
    from disconet_amd.synthetic import make_gt_boxes
    det = _np(_model_det(case))
    det.pop("index")
    assert det["count"].min() > 0
    for max_boxes in (64, 256):
        gb, gc = (t.numpy() for t in make_gt_boxes(len(det["count"]), seed=GT_SEED, max_boxes=max_boxes))
        _, want = _compare(det, gb, gc, "%s, %d ground-truth rows, seed %d" % (case, max_boxes, GT_SEED))
        print("%s: %d of %d detections meet a ground-truth box" % (case, (want["best_gt"] >= 0).sum(), det["count"].sum()))
        assert (want["best_gt"] >= 0).sum() > 0             # the boxes do meet detections: there is something to match


# ---- 5. MeanAP --------------------------------------------------------------------------------------------------------
def _frames(pitch=3.5, n_img=20):
    return [A.make(20 + f, n_img=n_img, pitch=pitch, n_gt=20 + f) for f in range(4)]


def _reference_aps(frames, batch):
    """(overall [AP per threshold], per agent [[AP per threshold]]) of the concatenated frames through the host reference
    and through the oracle; asserts that the two are the same bits"""
    from disconet_amd import postprocess as P
    n = len(frames[0][0])
    scores, flags, agent, n_gt = [], [], [], np.zeros(n // batch, np.int64)
    for dets, scs, gts in frames:
        det, gb, gc = A.padded(dets, scs, gts)
        A.assert_margins(det, gb, gc, "frame")
        s, tp, img = P.records_from_match(det, P.host_match_ground_truth(det, gb, gc, A.THRS))
        scores.append(s)
        flags.append(tp)
        agent.append(img // batch)
        np.add.at(n_gt, np.arange(n) // batch, gc)
    scores, flags, agent = np.concatenate(scores), np.concatenate(flags, axis=1), np.concatenate(agent)
    overall = [P.average_precision_from_records(scores, flags[t], n_gt.sum()) for t in range(2)]
    per_agent = [[P.average_precision_from_records(scores[agent == a], flags[t][agent == a], n_gt[a]) for t in range(2)]
                 for a in range(n // batch)]
    cat = lambda q, sel: [x for f in frames for i, x in enumerate(f[q]) if sel(i)]      # noqa: E731
    for t, thr in enumerate(A.THRS):
        want = A.oracle_ap(cat(0, lambda i: True), cat(1, lambda i: True), cat(2, lambda i: True), thr)
        assert A.bits(overall[t]) == A.bits(want)
        for a in range(n // batch):
            mine = lambda i: i // batch == a                                             # noqa: E731
            assert A.bits(per_agent[a][t]) == A.bits(A.oracle_ap(cat(0, mine), cat(1, mine), cat(2, mine), thr))
    return overall, per_agent, int(n_gt.sum()), len(scores)


def _run(metric, frames):
    for dets, scs, gts in frames:
        metric.update(*_cuda(*A.padded(dets, scs, gts)))
    return metric.compute()


def _assert_result(res, overall, per_agent, n_gt, n_det):
    assert A.bits(res["mAP@0.5"]) == A.bits(overall[0]) and A.bits(res["mAP@0.7"]) == A.bits(overall[1]), (res, overall)
    assert res["n_gt"] == n_gt and res["n_det"] == n_det and len(res["per_agent"]) == len(per_agent)
    for row, want in zip(res["per_agent"], per_agent):
        assert A.bits(row["mAP@0.5"]) == A.bits(want[0]) and A.bits(row["mAP@0.7"]) == A.bits(want[1]), (row, want)
    assert sum(r["n_det"] for r in res["per_agent"]) == n_det and sum(r["n_gt"] for r in res["per_agent"]) == n_gt


def test_mean_ap_four_updates_equal_host_and_oracle_bits():
    from disconet_amd import postprocess as P
    frames = _frames()
    overall, per_agent, n_gt, n_det = _reference_aps(frames, batch=4)
    print("four frames: %d records, %d ground truth, AP %.6f / %.6f" % (n_det, n_gt, overall[0], overall[1]))
    assert 0.05 < overall[1] < overall[0] < 0.9
    m = P.MeanAP(batch_size=4, capacity=4096)
    _assert_result(_run(m, frames), overall, per_agent, n_gt, n_det)
    first = (m.records[:n_det].cpu().numpy().copy(), m.state.cpu().numpy().copy())
    m.reset()
    assert m.compute()["n_det"] == 0 and m.compute()["n_gt"] == 0
    _assert_result(_run(m, frames), overall, per_agent, n_gt, n_det)
    other = P.MeanAP(batch_size=4, capacity=4096)
    _assert_result(_run(other, frames), overall, per_agent, n_gt, n_det)
    for again in ((m.records[:n_det].cpu().numpy(), m.state.cpu().numpy()),
                  (other.records[:n_det].cpu().numpy(), other.state.cpu().numpy())):
        assert again[0].tobytes() == first[0].tobytes() and again[1].tobytes() == first[1].tobytes()
    assert int(first[1][0]) == n_det and int(first[1][1]) == 0 and int(first[1][2:].sum()) == n_gt


# ---- 6. input order ---------------------------------------------------------------------------------------------------
def test_row_order_changes_rank_only():
    from disconet_amd import postprocess as P
    dets, scs, gts = A.make(3, pitch=3.5, quant=1 << 22)               # distinct scores within an image
    assert all(len(np.unique(s)) == len(s) for s in scs)
    det, gb, gc = A.padded(dets, scs, gts)
    base, _ = _compare(det, gb, gc, "sorted-free input")
    r = np.random.default_rng(9)
    perms = [r.permutation(len(s)) for s in scs]
    det_p, _, _ = A.padded([d[p] for d, p in zip(dets, perms)], [s[p] for s, p in zip(scs, perms)], gts)
    shuf, _ = _compare(det_p, gb, gc, "shuffled rows")
    for i, p in enumerate(perms):
        c = len(p)
        for name in ("rank", "best_gt", "best_iou"):
            assert np.array_equal(shuf[name][i, :c], base[name][i, :c][p]), (name, i)
        assert np.array_equal(shuf["tp"][:, i, :c], base["tp"][:, i, :c][:, p]), i
    a, b = A.host_ap(det, gb, gc, match=base), A.host_ap(det_p, gb, gc, match=shuf)
    assert [A.bits(x) for x in a] == [A.bits(x) for x in b]
    m = P.MeanAP(batch_size=4)
    m.update(*_cuda(det_p, gb, gc))
    res = m.compute()
    assert A.bits(res["mAP@0.5"]) == A.bits(a[0]) and A.bits(res["mAP@0.7"]) == A.bits(a[1])
    # rows that detect() sorted: rank is the row index
    order = [np.argsort(-s, kind="stable") for s in scs]
    det_s, _, _ = A.padded([d[o] for d, o in zip(dets, order)], [s[o] for s, o in zip(scs, order)], gts)
    srt, _ = _compare(det_s, gb, gc, "sorted rows")
    for i, o in enumerate(order):
        assert srt["rank"][i, :len(o)].tolist() == list(range(len(o)))


# ---- 7. capacity and non-finite scores ----------------------------------------------------------------------------------
def _guarded(metric, device="cuda"):
    """give `metric` record storage with a guard region behind it"""
    big = torch.full((metric.capacity + 256, 2), 0x5a5a5a5a, dtype=torch.int32, device=device)
    metric._allocate(device)
    metric.records = big[:metric.capacity]
    return big


def test_overflow_and_nan_raise_and_stay_inside_the_arrays():
    from disconet_amd import _lib as L
    from disconet_amd import postprocess as P
    frames = _frames()
    n_first = int(sum(len(s) for s in frames[0][1]))
    m = P.MeanAP(batch_size=4, capacity=n_first + 100)          # the second frame does not fit
    big = _guarded(m)
    with pytest.raises(L.DnError, match="capacity"):
        _run(m, frames)
    torch.cuda.synchronize()
    assert (big[m.capacity:] == 0x5a5a5a5a).all()
    assert (big[:m.capacity] != 0x5a5a5a5a).any(dim=1).all()     # every slot below the capacity was written
    state = m.state.cpu().numpy()
    assert int(state[0]) == sum(len(s) for f in frames for s in f[1]) and int(state[1]) == 1
    m.reset()                                                   # the bit is sticky until reset
    m.update(*_cuda(*A.padded(*frames[0])))
    assert m.compute()["n_det"] == n_first
    # a NaN score below count: no record, the status bit, compute() raises
    dets, scs, gts = frames[1]
    scs = [s.copy() for s in scs]
    scs[2][1] = np.nan
    m2 = P.MeanAP(batch_size=4, capacity=2048)
    big2 = _guarded(m2)
    m2.update(*_cuda(*A.padded(dets, scs, gts)))
    with pytest.raises(L.DnError, match="non-finite"):
        m2.compute()
    state = m2.state.cpu().numpy()
    n_rows = int(sum(len(s) for s in scs))
    assert int(state[0]) == n_rows - 1 and int(state[1]) == 2
    assert (big2[m2.capacity:] == 0x5a5a5a5a).all() and (big2[n_rows - 1:m2.capacity] == 0x5a5a5a5a).all()
    got, want = _compare(*A.padded(dets, scs, gts), "a NaN score", margins=False)
    assert got["rank"][2, 1] == -1 and got["best_gt"][2, 1] == -1


# ---- 8. captured graph --------------------------------------------------------------------------------------------------
def _graph_case(stream=None):
    from disconet_amd import Config, DiscoNet, graph, postprocess as P
    from disconet_amd.synthetic import make_gt_boxes, make_scene_batch, randomize_bn_stats
    agents, batch, hw, n_frames = 4, 2, 128, 4
    torch.manual_seed(0)
    model = DiscoNet(Config(map_hw=hw), kd_flag=0, num_agent=agents)
    randomize_bn_stats(model)
    model.eval().cuda()
    anchors = P.make_anchors(Config(map_hw=hw))
    inputs = [[t.cuda() for t in make_scene_batch(batch, agents, hw, jitter_seed=40 + f)] +
              [t.cuda() for t in make_gt_boxes(agents * batch, seed=GT_SEED + f, max_boxes=64)] for f in range(n_frames)]
    static = [t.clone() for t in inputs[0]]

    def load(f):
        for dst, src in zip(static, inputs[f]):
            dst.copy_(src)

    def forward_detect():
        with torch.no_grad():
            out = model(static[0], static[1], static[2], batch)
        return P.detect(out[0] if isinstance(out, tuple) else out, anchors)

    # eager sequence, and the host reference over the same detections
    eager = P.MeanAP(batch_size=batch, capacity=1 << 14)
    host_frames = []
    for f in range(n_frames):
        load(f)
        det = forward_detect()
        eager.update(det, static[3], static[4])
        d = _np(det)
        d.pop("index")
        gb, gc = static[3].cpu().numpy(), static[4].cpu().numpy()
        A.assert_margins(d, gb, gc, "graph frame %d" % f)
        host_frames.append(A.lists(d, gb, gc))
    want = eager.compute()
    overall, per_agent, n_gt, n_det = _reference_aps(host_frames, batch)
    _assert_result(want, overall, per_agent, n_gt, n_det)
    assert n_det > 50 and want["mAP@0.5"] >= 0.0

    metric = P.MeanAP(batch_size=batch, capacity=1 << 14)
    ctx = torch.cuda.stream(stream) if stream is not None else None
    if ctx is not None:
        stream.wait_stream(torch.cuda.current_stream())
        ctx.__enter__()
    try:
        load(0)
        step = graph.GraphedStep(lambda: metric.update(forward_detect(), static[3], static[4]))
        metric.reset()                               # the warm-up runs and the capture appended records
        for f in range(n_frames):
            load(f)
            step()
        step.drain()
        got = metric.compute()
    finally:
        if ctx is not None:
            ctx.__exit__(None, None, None)
            torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    _assert_result(got, overall, per_agent, n_gt, n_det)
    assert got == want
    assert metric.records[:n_det].cpu().numpy().tobytes() == eager.records[:n_det].cpu().numpy().tobytes()


def test_graph_forward_detect_update_equals_eager():
    _graph_case()


def test_graph_on_a_side_stream_equals_eager():
    _graph_case(torch.cuda.Stream())


# ---- 9. the evaluation tool -----------------------------------------------------------------------------------------------
ROW = (r"^(agent \d+|overall): mAP@0\.5 (\S+)  mAP@0\.7 (\S+)  \((\d+) detections, (\d+) ground-truth boxes, "
       r"true positives (\d+) / (\d+)\)")


def _tool(*extra):
    tool = os.path.join(ROOT, "tools", "det", "eval_codet.py")
    r = subprocess.run([sys.executable, tool, "--com", "disco", "--frames", "2"] + list(extra), cwd=ROOT,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    print(r.stdout)
    return r.stdout


def test_eval_codet_self_ground_truth_is_one():
    out = _tool("--gt", "self")
    rows = re.findall(ROW, out, re.M)
    assert [r[0] for r in rows] == ["agent %d" % a for a in range(5)] + ["overall"], out
    for _, a5, a7, n_det, n_gt, tp5, tp7 in rows:
        assert a5 == "1.0000" and a7 == "1.0000" and int(n_det) == int(n_gt) == int(tp5) == int(tp7) > 0, out


def test_eval_codet_synthetic_ground_truth_equals_host():
    from disconet_amd import Config, DiscoNet, postprocess as P
    from disconet_amd.synthetic import make_gt_boxes, make_scene_batch, randomize_bn_stats
    # up to 1024 rows per image that may overlap up to IoU 0.5: enough detections for the seeded boxes to meet some
    out = _tool("--gt", "synthetic", "--num_agent", "2", "--batch", "2", "--pre_nms_top_k", "1024", "--iou_thr", "0.5")
    assert "plumbing, not accuracy" in out
    rows = re.findall(ROW, out, re.M)
    assert [r[0] for r in rows] == ["agent 0", "agent 1", "overall"], out
    # the same frames through detect() and the host reference
    config = Config("test", binary=True, only_det=True)
    torch.manual_seed(0)                                  # the tool's seed
    model = DiscoNet(config, layer=3, kd_flag=0, num_agent=2)
    randomize_bn_stats(model)
    model.eval().cuda()
    anchors = P.make_anchors(config)
    frames = []
    for f in range(2):
        bevs, trans, na = make_scene_batch(2, 2, config.map_dims[0], jitter_seed=f)
        with torch.no_grad():
            res = model(bevs.cuda(), trans.cuda(), na.cuda(), 2)
        det = _np(P.detect(res[0] if isinstance(res, tuple) else res, anchors, pre_nms_top_k=1024, iou_thr=0.5))
        det.pop("index")
        gb, gc = (t.numpy() for t in make_gt_boxes(4, seed=f, max_boxes=64))
        A.assert_margins(det, gb, gc, "tool frame %d" % f)
        frames.append(A.lists(det, gb, gc))
    overall, per_agent, n_gt, n_det = _reference_aps(frames, 2)
    n_tp = [0, 0]
    for dets, scs, gts in frames:
        tp = P.host_match_ground_truth(*A.padded(dets, scs, gts), A.THRS)["tp"]
        n_tp = [n_tp[t] + int(tp[t].sum()) for t in range(2)]
    assert n_tp[0] > 0                                    # the figures are not trivially zero
    assert [int(v) for v in rows[-1][5:7]] == n_tp
    want = [("agent %d" % a, "%.4f" % ap[0], "%.4f" % ap[1]) for a, ap in enumerate(per_agent)]
    want.append(("overall", "%.4f" % overall[0], "%.4f" % overall[1]))
    assert [r[:3] for r in rows] == want, (rows, want)
    assert int(rows[-1][3]) == n_det and int(rows[-1][4]) == n_gt
