"""Mean IoU on the GPU (dn_seg_confusion, seg.MeanIoU) against the host statement seg.HostMeanIoU: the state, the
prediction and every compute() figure, bit for bit -- both kernel paths at the smallest shapes that can still go wrong, the
planted rows, the ignore rules, contention on one cell, accumulation, graph replay, the bench's size, and
SegModule.evaluate(metric=...) on a small SegDiscoNet."""
import numpy as np
import pytest
import torch

from tests import cases
from tests.seg_miou_cases import planted_rows

pytestmark = pytest.mark.gpu


def _inputs(n, pixels, classes, seed, ld=None, bad_labels=True):
    """seeded logits [n, pixels, classes] (a slice of a [.., ld] map when ld is given) and int64 labels [n, pixels]"""
    g = torch.Generator().manual_seed(seed)
    wide = torch.randn(n, pixels, ld or classes, generator=g)
    labels = torch.randint(0, classes, (n, pixels), generator=g)
    if bad_labels:
        for value in (-100, -1, classes, 255):
            labels[torch.rand(n, pixels, generator=g) < 0.05] = value
    return wide, labels


def _same_figures(got, want):
    assert got.keys() == want.keys()
    for key in ("per_image", "per_agent"):
        assert len(got[key]) == len(want[key])
    for a, b in zip(got["per_image"] + got["per_agent"] + [got["overall"]], want["per_image"] + want["per_agent"] + [want["overall"]]):
        assert np.array_equal(a["confusion"], b["confusion"]) and a["ignored"] == b["ignored"]
        assert np.array_equal(a["iou"].view(np.uint64), b["iou"].view(np.uint64))
        for key in ("mIoU", "accuracy"):
            assert np.float64(a[key]).view(np.uint64) == np.float64(b[key]).view(np.uint64), key


def _check(logits_dev, logits_host, labels, classes, live=None, agents=None):
    """one update on the device and on the host: state, pred and figures as bits -> the device metric"""
    from disconet_amd.seg import HostMeanIoU, MeanIoU
    n = labels.shape[0]
    dev, host = MeanIoU(n, classes), HostMeanIoU(n, classes)
    pred = dev.update(logits_dev, labels.cuda(), live=None if live is None else live.cuda(), want_pred=True)
    want = host.update(logits_host, labels, live=live, want_pred=True)
    assert pred.dtype == torch.int32 and pred.shape == labels.shape
    assert np.array_equal(pred.cpu().numpy(), want)
    assert torch.equal(pred.long(), logits_dev.argmax(-1).reshape(labels.shape))          # torch.argmax on the device as well
    assert np.array_equal(dev.state.cpu().numpy(), host.state)
    assert int(dev.state.sum()) == labels.numel()
    _same_figures(dev.compute(agents=agents, ignore_classes=(0,)), host.compute(agents=agents, ignore_classes=(0,)))
    _same_figures(dev.compute(agents=agents), host.compute(agents=agents))
    return dev


# ---- 1. the two paths at their smallest shapes ------------------------------------------------------------------------
@pytest.mark.parametrize("pixels", [1, 63, 65, 1000])
def test_row8_path_equals_host(pixels):
    logits, labels = _inputs(3, pixels, 8, seed=pixels)
    _check(logits.cuda(), logits, labels, 8, agents=3)


def test_slice_of_a_wider_map_takes_the_general_path_and_equals_host():
    wide, labels = _inputs(3, 333, 8, seed=12, ld=12)
    dev_wide = wide.cuda()
    for first in (0, 3):                                                    # rows 48 bytes apart, at offset 0 and 12 bytes
        _check(dev_wide[..., first:first + 8], wide[..., first:first + 8], labels, 8)


@pytest.mark.parametrize("classes", [2, 5, 32])
def test_general_path_equals_host(classes):
    logits, labels = _inputs(3, 777, classes, seed=classes)
    _check(logits.cuda(), logits, labels, classes)


# ---- 2. the prediction rule -------------------------------------------------------------------------------------------------
def test_planted_tie_nan_inf_rows_equal_host_and_torch_argmax():
    rows = torch.from_numpy(planted_rows())                                 # [15, 8]
    logits = rows.repeat(9, 1)[:130].reshape(2, 65, 8).contiguous()
    labels = torch.arange(130).reshape(2, 65) % 8
    _check(logits.cuda(), logits, labels, 8)
    wide = torch.full((2, 65, 11), float("nan"))                            # the general path: NaN around the slice
    wide[..., 2:10] = logits
    _check(wide.cuda()[..., 2:10], logits, labels, 8)
    five = logits[..., :5].contiguous()
    _check(five.cuda(), five, labels % 5, 5)


# ---- 3. the ignore rules ------------------------------------------------------------------------------------------------
def test_ignored_labels_and_a_dead_middle_image():
    logits, labels = _inputs(3, 1000, 8, seed=21)
    live = torch.tensor([1, 0, 1], dtype=torch.uint8)
    dev = _check(logits.cuda(), logits, labels, 8, live=live)
    state = dev.state.cpu().numpy()
    bad = ((labels < 0) | (labels >= 8)).sum(1).numpy()
    assert state[:, -1].tolist() == [bad[0], 1000, bad[2]] and bad[0] > 0
    assert state[1, :-1].sum() == 0
    _check(logits.cuda(), logits, labels, 8, live=torch.tensor([True, False, True]))      # bool masks too
    # uint8 label maps: 255 is out of range, not -1 + 256
    small = torch.where((labels >= 0) & (labels < 8), labels, torch.full_like(labels, 255)).to(torch.uint8)
    from disconet_amd.seg import MeanIoU
    m = MeanIoU(3, 8)
    m.update(logits.cuda(), small.cuda(), live=live.cuda())
    assert np.array_equal(m.state.cpu().numpy(), state)


def test_labels_wider_than_int32_stay_out_of_range_and_one_pixel_views_of_any_stride():
    logits, labels = _inputs(3, 200, 8, seed=23, bad_labels=False)
    labels[0, 0], labels[1, 7], labels[2, 199] = 2 ** 32 + 3, -(2 ** 32) + 5, 2 ** 31 + 1      # each wraps into range as int32
    dev = _check(logits.cuda(), logits, labels, 8)
    assert dev.state[:, -1].tolist() == [1, 1, 1]
    # one pixel per image: the stride of the pixel dimension says nothing, in a dense map and in a slice of a wider one
    wide = torch.randn(3, 40, 12, generator=torch.Generator().manual_seed(24))
    dev_wide = wide.cuda()
    for view_dev, view in ((dev_wide[:, 5:6, :8], wide[:, 5:6, :8]), (dev_wide[:, 39:, 4:], wide[:, 39:, 4:]),
                           (dev_wide[:1, 2:3, :8], wide[:1, 2:3, :8])):
        _check(view_dev, view, torch.arange(view.shape[0]).reshape(-1, 1), 8)


def test_70000_pixels_in_one_cell_across_workgroups():
    pixels = 70000
    logits = torch.zeros(1, pixels, 8)
    logits[..., 5] = 1.0
    labels = torch.full((1, pixels), 3)
    dev = _check(logits.cuda(), logits, labels, 8)
    state = dev.state.cpu().numpy()
    assert state[0, 3 * 8 + 5] == pixels and state.sum() == pixels


# ---- 4. accumulation, reset, no prediction -------------------------------------------------------------------------------
def test_three_updates_accumulate_reset_zeroes_and_no_pred_is_written():
    from disconet_amd import ops
    from disconet_amd.seg import HostMeanIoU, MeanIoU
    dev, total = MeanIoU(2, 8), np.zeros((2, 65), dtype=np.int64)
    for seed in (1, 2, 3):
        logits, labels = _inputs(2, 500, 8, seed=seed)
        host = HostMeanIoU(2, 8)
        host.update(logits, labels)
        total += host.state
        assert dev.update(logits.cuda(), labels.cuda()) is None             # want_pred=False: nothing to write
    assert np.array_equal(dev.state.cpu().numpy(), total)
    dev.reset()
    assert not dev.state.any()
    # the NCHW-shaped view of channels-last rows, as the model returns its logits
    logits, labels = _inputs(2, 24 * 20, 8, seed=4)
    nchw = logits.reshape(2, 24, 20, 8).cuda().permute(0, 3, 1, 2)
    host = HostMeanIoU(2, 8)
    host.update(logits.reshape(2, 24, 20, 8), labels.reshape(2, 24, 20))
    pred = dev.update(nchw, labels.reshape(2, 24, 20).cuda(), want_pred=True)
    assert pred.shape == (2, 24, 20) and np.array_equal(dev.state.cpu().numpy(), host.state)
    with pytest.raises(ops._lib.DnError):
        ops.seg_confusion(logits.cuda(), labels.cuda(), torch.zeros(2, 64, dtype=torch.int64, device="cuda"))


# ---- 5. capture -------------------------------------------------------------------------------------------------------------
def test_captured_update_replayed_three_times_gives_the_fourfold_count():
    from disconet_amd import graph
    from disconet_amd.seg import HostMeanIoU, MeanIoU
    logits, labels = _inputs(3, 1000, 8, seed=31)
    z, y, live = logits.cuda(), labels.cuda(), torch.tensor([1, 1, 0], dtype=torch.uint8).cuda()
    host = HostMeanIoU(3, 8)
    want = host.update(logits, labels, live=live.cpu(), want_pred=True)
    dev = MeanIoU(3, 8)
    step = graph.GraphedStep(lambda: dev.update(z, y, live=live, want_pred=True), warmup=1)      # one warm-up call: counted
    for replay in range(3):                                                 # (the capture itself runs nothing)
        pred = step()
    step.drain()
    torch.cuda.synchronize()
    assert np.array_equal(pred.cpu().numpy(), want)
    assert np.array_equal(dev.state.cpu().numpy(), 4 * host.state)


# ---- 6. the bench's size ----------------------------------------------------------------------------------------------------
def test_bench_size_20_images_256x256x8():
    g = torch.Generator().manual_seed(41)
    labels = torch.randint(0, 3, (20, 64, 64), generator=g).repeat_interleave(4, 1).repeat_interleave(4, 2)   # uniform 4 x 4 patches
    labels[:, :2] = -100
    logits = torch.nn.functional.one_hot(labels.clamp(min=0), 8).float() * 2.0 + torch.randn(20, 256, 256, 8, generator=g)
    live = torch.ones(20, dtype=torch.uint8)
    live[7] = 0
    dev = _check(logits.cuda(), logits, labels, 8, live=live, agents=5)
    assert 0.0 < dev.compute()["overall"]["mIoU"] < 1.0


# ---- 7. SegModule.evaluate(metric=...) ------------------------------------------------------------------------------------
def test_evaluate_with_metric_on_a_small_model():
    from disconet_amd import HostMeanIoU, MeanIoU, SegDiscoNet, SegModule
    case = "seg_ragged_a4"                                                  # 4 agents x 2 scenes at 128 x 128, live = [3, 2]
    c = cases.SEG_CASES[case]
    x, trans, na, labels = cases.seg_inputs(case)
    A, B = c["agents"], c["batch"]
    torch.manual_seed(0)
    m = SegDiscoNet(num_agent=A).eval().cuda()
    mod = SegModule(m)
    data = {"bev_seq": x.cuda(), "trans_matrices": trans.cuda(), "num_agent": na.cuda(), "labels": labels.cuda()}
    plain = mod.evaluate(data, B)
    metric = MeanIoU(A * B, 8)
    out = mod.evaluate(data, B, metric=metric)
    with torch.no_grad():
        logits = m(data["bev_seq"], data["trans_matrices"], data["num_agent"], B)
    assert out["pred"].dtype == plain["pred"].dtype and torch.equal(out["pred"], logits.argmax(1))
    assert torch.equal(out["pred"], plain["pred"])
    # the same logits through the same loss kernel; its workgroups' float64 partial sums (at most 2048) meet in an atomic
    # whose order is free: 2048 * 2^-53 = 2.3e-13 relative
    assert abs(out["loss"] - plain["loss"]) <= 2.3e-13 * abs(plain["loss"])
    # the padded slots (agent a of scene b with a >= live[b]) have empty BEVs: ignored whatever their labels are
    empty = [a * B + b for a in range(A) for b in range(B) if a >= c["live"][b]]
    live = torch.ones(A * B, dtype=torch.uint8)
    live[empty] = 0
    assert empty and all(float(x[i].abs().sum()) == 0.0 for i in empty)
    host = HostMeanIoU(A * B, 8)
    host.update(logits.cpu(), labels, live=live)
    state = metric.state.cpu().numpy()
    assert np.array_equal(state, host.state)
    hw = c["map_hw"]
    assert all(state[i, -1] == hw * hw and state[i, :-1].sum() == 0 for i in empty) and (labels[empty] >= 0).all()
    assert all(state[i, -1] == 0 for i in range(A * B) if i not in empty)
    _same_figures(metric.compute(agents=A), host.compute(agents=A))
