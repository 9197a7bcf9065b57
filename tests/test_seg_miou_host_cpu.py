"""Mean IoU of the seg variant without a GPU: the C ABI of dn_seg_confusion (declared, exported, bound), the host statement
seg.HostMeanIoU -- its prediction rule against torch.argmax on planted rows, its confusion against a plain np.bincount
restatement, compute()'s figures by hand -- and the labelled scenes of synthetic.make_seg_scene_batch against a
brute-force per-pixel loop over the returned world boxes and poses."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from tests.conftest import ROOT
from tests.seg_miou_cases import plain_confusion, planted_rows


# ---- 1. the C ABI ----------------------------------------------------------------------------------------------------
def test_header_declares_seg_confusion_and_binding_exists():
    from disconet_amd import _lib
    from disconet_amd.csrc import build
    raw = open(os.path.join(ROOT, "include", "disconet_seg.h")).read()
    assert "recalled, not pinned" in raw.lower()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert re.search(r"\bdn_seg_confusion\s*\(", text)
    lib = _lib.load()
    assert lib.dn_version() >= 146
    assert "seg_eval.hip" in build.SOURCES
    restype, argtypes = _lib.SIGNATURES["dn_seg_confusion"]
    assert restype is ctypes.c_int and len(argtypes) == 10
    assert argtypes[1] is ctypes.c_int and argtypes[4] is ctypes.c_int and argtypes[5] is ctypes.c_long and argtypes[6] is ctypes.c_int
    fn = lib.dn_seg_confusion
    assert fn.restype is ctypes.c_int and list(fn.argtypes) == list(argtypes)


@pytest.mark.parametrize("kw, word", [
    (dict(classes=1), "classes"), (dict(classes=33), "classes"), (dict(classes=0), "classes"), (dict(classes=8, ld=7), "ld"),
    (dict(n=0), "images"), (dict(n=65536), "images"), (dict(pixels=0), "pixels"), (dict(null="logits"), "null"),
    (dict(null="labels"), "null"), (dict(null="state"), "null"), (dict(state=0x1004), "8-byte aligned")])
def test_seg_confusion_refuses_bad_arguments_before_a_launch(kw, word):
    """fake (never dereferenced) device pointers: every refusal happens before a launch"""
    from disconet_amd import _lib
    lib = _lib.load()
    a = dict(classes=8, ld=8, n=2, pixels=100, null=None, state=0x1000)
    a.update(kw)
    a.setdefault("ld", a["classes"])
    p = {name: (None if name == a["null"] else ctypes.c_void_p(a["state"] if name == "state" else 0x1000))
         for name in ("logits", "labels", "state")}
    rc = lib.dn_seg_confusion(p["logits"], a["ld"], p["labels"], None, a["n"], a["pixels"], a["classes"], p["state"], None, None)
    assert rc != 0 and word in lib.dn_last_error().decode()


# ---- 2. the prediction rule ---------------------------------------------------------------------------------------------
def test_host_prediction_rule_equals_torch_argmax_on_planted_rows():
    from disconet_amd.seg import host_argmax
    rows = planted_rows()
    want = torch.from_numpy(rows).argmax(-1).numpy()
    assert np.array_equal(host_argmax(rows), want)
    assert np.array_equal(np.argmax(rows, -1), want)
    by_hand = [1, 0, 0, 3, 2, 4, 2, 0, 3, 1, 0, 0, 1, 7, 0]
    assert want.tolist() == by_hand
    # and on rows of other widths, with the planted values shuffled in
    rng = np.random.RandomState(0)
    for classes in (2, 5, 32):
        z = rng.standard_normal((4000, classes)).astype(np.float32)
        z[rng.rand(*z.shape) < 0.05] = np.nan
        z[rng.rand(*z.shape) < 0.05] = np.inf
        z[rng.rand(*z.shape) < 0.05] = -np.inf
        z[rng.rand(*z.shape) < 0.1] = 0.0
        z[rng.rand(*z.shape) < 0.1] = -0.0
        assert np.array_equal(host_argmax(z), torch.from_numpy(z).argmax(-1).numpy())


# ---- 3. the confusion ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("classes", [8, 5])
def test_host_confusion_equals_plain_bincount(classes):
    from disconet_amd.seg import HostMeanIoU
    rng = np.random.RandomState(classes)
    n, h, w = 3, 17, 23
    logits = rng.standard_normal((n, h, w, classes)).astype(np.float32)
    labels = rng.randint(0, classes, (n, h, w)).astype(np.int64)
    for value in (-100, -1, classes, 255):
        labels[rng.rand(n, h, w) < 0.05] = value
    live = np.array([1, 0, 1], dtype=np.uint8)
    m = HostMeanIoU(n, classes)
    pred = m.update(logits, labels, live=live, want_pred=True)
    assert pred.shape == labels.shape and np.array_equal(pred, logits.argmax(-1))
    counts, ignored = plain_confusion(pred, labels, classes, live)
    assert np.array_equal(m.state[:, :classes * classes], counts) and np.array_equal(m.state[:, -1], ignored)
    assert ignored[1] == h * w and counts[1].sum() == 0 and 0 < ignored[0] < h * w
    assert (m.state.sum(1) == h * w).all()
    # accumulation, the NCHW-shaped view, torch tensors and uint8 label maps (255 is a label out of range, not -1)
    assert m.update(torch.from_numpy(logits).permute(0, 3, 1, 2), torch.from_numpy(labels), live=torch.from_numpy(live)) is None
    assert np.array_equal(m.state[:, :classes * classes], 2 * counts)
    m.reset()
    assert not m.state.any()
    m.update(logits, np.where((labels >= 0) & (labels < classes), labels, 255).astype(np.uint8), live=live)
    assert np.array_equal(m.state[:, :classes * classes], counts) and np.array_equal(m.state[:, -1], ignored)
    with pytest.raises(ValueError):
        m.update(logits, labels.astype(np.float32))


def test_layout_rule_refuses_the_ambiguous_shape_and_a_wrong_image_count():
    from disconet_amd.seg import HostMeanIoU
    rng = np.random.RandomState(9)
    nhwc = rng.standard_normal((2, 8, 6, 8)).astype(np.float32)            # H == classes: [2, 8, 6, 8] could be either layout
    labels = rng.randint(0, 8, (2, 8, 6))
    m = HostMeanIoU(2, 8)
    with pytest.raises(ValueError, match="NCHW or NHWC"):
        m.update(nhwc, labels)
    with pytest.raises(ValueError, match="NCHW or NHWC"):
        m.update(torch.from_numpy(nhwc), torch.from_numpy(labels))
    want = HostMeanIoU(2, 8)
    want.update(nhwc.reshape(2, 48, 8), labels)                             # stated as rows: fine
    m.update(torch.from_numpy(nhwc).permute(0, 3, 1, 2), labels)            # the channels-last view [2, 8, 8, 6]: fine
    assert np.array_equal(m.state, want.state) and not m.state[:, -1].any()
    square = rng.standard_normal((2, 8, 8, 8)).astype(np.float32)
    m.reset(), want.reset()
    m.update(torch.from_numpy(square).permute(0, 3, 1, 2), labels[:, :, :1].repeat(8, 2))
    want.update(square.reshape(2, 64, 8), labels[:, :, :1].repeat(8, 2))
    assert np.array_equal(m.state, want.state)
    for bad in (np.zeros((3, 8, 5, 5), np.float32), np.zeros((3, 5, 5, 8), np.float32), np.zeros((2, 5, 5, 7), np.float32)):
        with pytest.raises(ValueError, match="2 images x 8 classes"):       # 3 images in either layout; 7 classes
            m.update(bad, np.zeros((bad.shape[0], 5, 5), np.int64))
    wide = np.full((2, 5, 8), 3, dtype=np.int64)
    wide[0, 0, 0], wide[1, 4, 7] = 2 ** 32 + 3, -(2 ** 32) + 3              # wider than int32: out of range, never wrapped
    m.reset()
    m.update(np.zeros((2, 5, 8, 8), np.float32), wide)
    assert m.state[:, -1].tolist() == [1, 1] and m.state[:, 3 * 8].tolist() == [39, 39]


# ---- 4. compute() -------------------------------------------------------------------------------------------------------
def test_compute_one_hot_constant_ignore_classes_agents_and_all_ignored():
    from disconet_amd.seg import HostMeanIoU, miou_figures
    rng = np.random.RandomState(3)
    classes, n, h, w = 8, 4, 12, 10
    labels = rng.randint(0, 5, (n, h, w)).astype(np.int64)                  # classes 5, 6, 7 absent
    labels[3] = -100                                                        # an all-ignored image
    one_hot = np.eye(classes, dtype=np.float32)[np.clip(labels, 0, None)]
    m = HostMeanIoU(n, classes)
    m.update(one_hot, labels)
    out = m.compute(agents=2)
    for fig in out["per_image"][:3] + [out["overall"], out["per_agent"][0]]:
        assert (fig["iou"][:5] == 1.0).all() and np.isnan(fig["iou"][5:]).all()
        assert fig["mIoU"] == 1.0 and fig["accuracy"] == 1.0
        assert fig["iou"].dtype == np.float64 and fig["confusion"].dtype == np.int64 and fig["confusion"].shape == (8, 8)
    dead = out["per_image"][3]                                              # NaN, and no exception
    assert np.isnan(dead["iou"]).all() and math.isnan(dead["mIoU"]) and math.isnan(dead["accuracy"]) and dead["ignored"] == h * w
    assert out["overall"]["ignored"] == h * w and out["per_agent"][1]["ignored"] == h * w
    # image = agent * B + b: agent 0 = images 0, 1; agent 1 = images 2, 3
    assert np.array_equal(out["per_agent"][0]["confusion"], out["per_image"][0]["confusion"] + out["per_image"][1]["confusion"])
    assert np.array_equal(out["per_agent"][1]["confusion"], out["per_image"][2]["confusion"])
    assert np.array_equal(out["overall"]["confusion"], sum(f["confusion"] for f in out["per_image"]))
    assert m.compute()["per_agent"] == []
    with pytest.raises(ValueError):
        m.compute(agents=3)

    # constant class 0: IoU_0 = the class-0 share of the live pixels, 0 for the other present classes
    m = HostMeanIoU(n, classes)
    zeros = np.zeros((n, h, w, classes), dtype=np.float32)
    m.update(zeros, labels)
    out = m.compute()
    for i in range(3):
        fig, share = out["per_image"][i], float((labels[i] == 0).sum()) / float(h * w)
        assert fig["iou"][0] == share and (fig["iou"][1:5] == 0.0).all() and np.isnan(fig["iou"][5:]).all()
        assert fig["accuracy"] == share and fig["mIoU"] == (share + 0.0 + 0.0 + 0.0 + 0.0) / 5
        # ignore_classes: the mean over the others
        assert m.compute(ignore_classes=(0,))["per_image"][i]["mIoU"] == 0.0
        assert m.compute(ignore_classes=(1, 2, 3, 4))["per_image"][i]["mIoU"] == share
        assert math.isnan(m.compute(ignore_classes=range(8))["per_image"][i]["mIoU"])
    # by hand
    fig = miou_figures(np.array([[3, 1], [2, 4]]), 7)
    assert fig["iou"].tolist() == [3.0 / 6.0, 4.0 / 7.0] and fig["mIoU"] == (3.0 / 6.0 + 4.0 / 7.0) / 2
    assert fig["accuracy"] == 7.0 / 10.0 and fig["ignored"] == 7


# ---- 5. the labelled scenes ------------------------------------------------------------------------------------------
def _brute_force_labels(scene, batch_size, num_agent, map_hw):
    from disconet_amd.config import Config
    from disconet_amd.synthetic import agent_pose
    cfg = Config(map_hw=map_hw)
    vs, lo = cfg.voxel_size[0], math.floor(cfg.area_extents[0][0] / cfg.voxel_size[0])
    out = np.zeros((num_agent * batch_size, map_hw, map_hw), dtype=np.int64)
    for b in range(batch_size):
        boxes, classes = scene["world_boxes"][b], scene["world_classes"][b]
        for a in range(num_agent):
            T = np.linalg.inv(agent_pose(a))
            mine = []
            for (x, y, w, h, s, c) in boxes:                 # the world box in the agent's frame, float64
                mine.append((T[0, 0] * x + T[0, 1] * y + T[0, 3], T[1, 0] * x + T[1, 1] * y + T[1, 3], w, h,
                             T[1, 0] * c + T[1, 1] * s, T[0, 0] * c + T[0, 1] * s))
            for i in range(map_hw):
                px = (i + lo + 0.5) * vs
                for j in range(map_hw):
                    py = (j + lo + 0.5) * vs
                    for k, (x, y, w, h, s, c) in enumerate(mine):
                        dx, dy = px - x, py - y
                        if abs(dx * c + dy * s) <= w / 2.0 and abs(dy * c - dx * s) <= h / 2.0:
                            out[a * batch_size + b, i, j] = classes[k]
                            break                            # the lowest index wins
    return out


def test_seg_scenes_are_seeded_and_labels_equal_a_brute_force_loop():
    from disconet_amd.synthetic import make_seg_scene_batch
    B, A, hw = 2, 2, 64
    one, two = make_seg_scene_batch(B, A, hw, seed=5), make_seg_scene_batch(B, A, hw, seed=5)
    other = make_seg_scene_batch(B, A, hw, seed=6)
    for key in ("bev_seq", "labels", "trans_matrices", "num_agent"):
        assert torch.equal(one[key], two[key]), key
    assert all(np.array_equal(p, q) for p, q in zip(one["points"], two["points"]))
    assert all(np.array_equal(p, q) for p, q in zip(one["world_boxes"], two["world_boxes"]))
    assert not torch.equal(one["labels"], other["labels"])
    labels = one["labels"].numpy()
    assert one["labels"].dtype == torch.int64 and labels.shape == (A * B, hw, hw)
    assert one["bev_seq"].shape == (A * B, 13, hw, hw) and one["bev_seq"].dtype == torch.float32
    assert np.array_equal(labels, _brute_force_labels(one, B, A, hw))
    assert set(np.unique(labels)) == {0, 1, 2}                              # cars and long vehicles both occur
    for b in range(B):
        cls, boxes = one["world_classes"][b], one["world_boxes"][b]
        assert ((boxes[cls == 2][:, 3] >= 10.0) & (boxes[cls == 2][:, 2] >= 2.6)).all() and (boxes[cls == 1][:, 3] <= 5.5).all()
    # the occupancy shows the boxes: occupied pixels are far more often labelled than the map at large
    occ = one["bev_seq"].numpy().max(1) > 0
    assert (labels[occ] > 0).mean() > 2 * (labels > 0).mean()


def test_seg_scene_ignore_border_writes_the_frame_only():
    from disconet_amd.synthetic import make_seg_scene_batch
    hw, k = 64, 3
    plain = make_seg_scene_batch(1, 2, hw, seed=1)["labels"].numpy()
    framed = make_seg_scene_batch(1, 2, hw, seed=1, ignore_border=k)["labels"].numpy()
    frame = np.ones((hw, hw), dtype=bool)
    frame[k:hw - k, k:hw - k] = False
    assert (framed[:, frame] == -100).all() and np.array_equal(framed[:, ~frame], plain[:, ~frame])
    assert (plain >= 0).all() and (framed == -100).sum() == 2 * (hw * hw - (hw - 2 * k) ** 2)
