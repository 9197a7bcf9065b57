"""Target assignment without a GPU: the C ABI of dn_assign_targets (declared, bound, every refusal before a launch), the
numpy reference targets.host_assign_targets on exact crafted cases, encode_boxes against the decode, the box scenes of
synthetic.make_box_scene_batch, and the tools' new flags."""
import argparse
import ctypes
import importlib.util
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import assign_cases as C
from tests.conftest import ROOT

NAMES = ("dn_assign_targets_workspace_bytes", "dn_assign_targets")


def _lib():
    from disconet_amd import _lib
    return _lib.load()


# ---- 1. the C ABI ----------------------------------------------------------------------------------------------------
def test_header_declares_assign_entry_points_and_bindings_exist():
    from disconet_amd import _lib
    raw = open(os.path.join(ROOT, "include", "disconet_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.SIGNATURES
        assert getattr(_lib.load(), name) is not None
    assert _lib.load().dn_version() >= 138
    from disconet_amd.csrc import build
    assert "assign.hip" in build.SOURCES
    import disconet_amd
    assert disconet_amd.targets.assign_targets is disconet_amd.assign_targets


POINTERS = ("anchors", "gt_boxes", "gt_count", "labels", "reg_targets", "reg_mask", "matched_gt", "best_iou", "ws")
OPTIONAL = ("matched_gt", "best_iou")


def _call(n=20, apl=393216, g=64, pos=0.6, neg=0.45, force=1, ws_bytes=None, null=()):
    """dn_assign_targets with fake (never dereferenced) device pointers: every refusal happens before a launch."""
    lib = _lib()
    need = lib.dn_assign_targets_workspace_bytes(max(1, n), max(1, apl), max(1, min(g, 1024)))
    fake = ctypes.c_void_p(0x1000)
    p = {name: (None if name in null else fake) for name in POINTERS}
    rc = lib.dn_assign_targets(p["anchors"], p["gt_boxes"], p["gt_count"], n, apl, g, pos, neg, force, p["labels"],
                               p["reg_targets"], p["reg_mask"], p["matched_gt"], p["best_iou"], p["ws"],
                               need if ws_bytes is None else ws_bytes, None)
    return rc, lib.dn_last_error().decode()


@pytest.mark.parametrize("which", [p for p in POINTERS if p not in OPTIONAL])
def test_null_required_pointer_is_refused(which):
    rc, msg = _call(null=(which,))
    assert rc != 0 and "null" in msg


def test_optional_outputs_may_be_null():
    # both optional outputs null: the call passes the pointer check and stops at the next one (a workspace of 0 bytes)
    rc, msg = _call(null=OPTIONAL, ws_bytes=0)
    assert rc != 0 and "workspace" in msg


@pytest.mark.parametrize("n", [0, -1])
def test_image_count_is_refused(n):
    rc, msg = _call(n=n)
    assert rc != 0 and "images" in msg


@pytest.mark.parametrize("apl", [0, -5])
def test_anchor_count_is_refused(apl):
    rc, msg = _call(apl=apl)
    assert rc != 0 and "anchors per image" in msg


@pytest.mark.parametrize("g", [0, 1025, -1])
def test_g_out_of_range_is_refused(g):
    rc, msg = _call(g=g)
    assert rc != 0 and "G = " in msg


@pytest.mark.parametrize("pos,neg", [(0.6, 0.0), (0.6, -0.1), (0.4, 0.45), (1.0000001, 0.45), (math.nan, 0.45),
                                     (0.6, math.nan), (math.inf, 0.45)])
def test_thresholds_are_refused(pos, neg):
    rc, msg = _call(pos=pos, neg=neg)
    assert rc != 0 and "thresholds" in msg


def test_threshold_limits_pass_and_short_workspace_is_refused():
    lib = _lib()
    need = lib.dn_assign_targets_workspace_bytes(20, 393216, 64)
    assert need >= 20 * 393216 * (8 + 4)               # one (IoU, row) per anchor at least
    rc, msg = _call(ws_bytes=need - 1)
    assert rc != 0 and "workspace" in msg
    for pos, neg in ((1.0, 1.0), (1.0, 1e-300), (0.5, 0.5)):                # the closed ends of the range pass the check
        rc, msg = _call(pos=pos, neg=neg, ws_bytes=0)
        assert rc != 0 and "workspace" in msg


def test_workspace_query_refuses_what_the_call_refuses():
    lib = _lib()
    for n, apl, g in ((0, 100, 64), (-1, 100, 64), (2, 0, 64), (2, -1, 64), (2, 100, 0), (2, 100, 1025)):
        assert lib.dn_assign_targets_workspace_bytes(n, apl, g) == 0, (n, apl, g)
    assert lib.dn_assign_targets_workspace_bytes(1, 1, 1) > 0
    assert lib.dn_assign_targets_workspace_bytes(20, 393216, 1024) > 0


def test_python_entry_point_refuses_what_it_cannot_run():
    from disconet_amd import _lib as L
    from disconet_amd import targets as T
    anchors, gb, gc, _ = C.crafted()
    with pytest.raises(L.DnError):
        T.assign_targets(torch.as_tensor(anchors), torch.as_tensor(gb), torch.as_tensor(gc))     # CPU tensors
    with pytest.raises(L.DnError):
        T.assign_targets(anchors, gb, gc)                                                       # numpy
    with pytest.raises(ValueError):
        T.assign_targets(torch.as_tensor(anchors), torch.as_tensor(gb), torch.as_tensor(gc), pos_thr=0.4, neg_thr=0.5)
    with pytest.raises(ValueError):
        T.host_assign_targets(anchors, gb, gc, pos_thr=0.6, neg_thr=0.0)


# ---- 2. encode_boxes is the inverse of the decode --------------------------------------------------------------------
def test_encode_then_decode_returns_the_boxes():
    """Measured on the CPU, 200 000 (box, anchor) pairs of the shipped anchor set (box within 3 m of its anchor, car sizes,
    any yaw, (sin, cos) of length 0.5 .. 2): the fp32 decode (oracle.postprocess_ref.decode_boxes) of the code rounded to
    fp32 deviates from the float64 decode of the float64 code by at most 9.54e-07 (the length column: one fp32 exp and one
    product at values up to 5.5); the bound is 4 x that, 3.9e-06.  The float64 decode returns the boxes to 3.5e-08 (the
    fp32 anchors' sin^2 + cos^2 is 1 only to fp32)."""
    from disconet_amd import Config, postprocess as P, targets as T
    from oracle import postprocess_ref as R
    n = 200000
    an = P.make_anchors(Config(), device="cpu").numpy().reshape(-1, 6)
    r = np.random.default_rng(0)
    a = an[r.integers(0, len(an), n)]
    b = np.zeros((n, 6), np.float32)
    b[:, :2] = a[:, :2] + r.uniform(-3, 3, (n, 2))
    b[:, 2], b[:, 3] = r.uniform(1.6, 2.4, n), r.uniform(3.5, 5.5, n)
    yaw, scale = r.uniform(-math.pi, math.pi, n), r.uniform(0.5, 2.0, n)
    b[:, 4], b[:, 5] = scale * np.sin(yaw), scale * np.cos(yaw)
    code = T.encode_boxes(b, a)
    assert code.dtype == np.float64
    a64 = a.astype(np.float64)
    want = np.stack([a64[:, 0] + code[:, 0] * a64[:, 2], a64[:, 1] + code[:, 1] * a64[:, 3], a64[:, 2] * np.exp(code[:, 2]),
                     a64[:, 3] * np.exp(code[:, 3]), a64[:, 4] * code[:, 5] + a64[:, 5] * code[:, 4],
                     a64[:, 5] * code[:, 5] - a64[:, 4] * code[:, 4]], -1)
    got = R.decode_boxes(code.astype(np.float32), a)
    dev = float(np.abs(got - want).max())
    norm = np.hypot(b[:, 4].astype(np.float64), b[:, 5].astype(np.float64))
    ref = b.astype(np.float64)
    ref[:, 4] /= norm
    ref[:, 5] /= norm
    back = float(np.abs(want - ref).max())
    print("fp32 decode of the fp32 code against the float64 decode of the float64 code: %.3g; float64 decode against the "
          "boxes: %.3g" % (dev, back))
    assert dev <= 4 * 9.54e-07
    assert back <= 4 * 3.5e-08


# ---- 3. crafted exact cases ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("force", [False, True])
def test_crafted_exact_cases(force):
    from disconet_amd import targets as T
    anchors, gb, gc, exp = C.crafted()
    res = T.host_assign_targets(anchors, gb, gc, C.POS, C.NEG, force_match=force)
    C.check_crafted(res, exp[force], gb)
    assert res["labels"].dtype == np.float32 and res["reg_targets"].dtype == np.float32
    assert res["matched_gt"].dtype == np.int32 and res["best_iou"].dtype == np.float64
    # padding wider than the data, filled with garbage, changes nothing
    wide = np.full((6, 7, 6), np.nan, np.float32)
    for i in range(6):
        wide[i, :gc[i]] = gb[i, :gc[i]]
    res_w = T.host_assign_targets(anchors, wide, gc, C.POS, C.NEG, force_match=force)
    for k in res:
        assert np.array_equal(res[k], res_w[k]), k


def test_forced_code_is_the_inverse_of_the_decode():
    from disconet_amd import targets as T
    from oracle import postprocess_ref as R
    anchors, gb, gc, _ = C.crafted()
    res = T.host_assign_targets(anchors, gb, gc, C.POS, C.NEG, force_match=True)
    pos = np.nonzero(res["matched_gt"] >= 0)
    assert len(pos[0]) == 6
    boxes = R.decode_boxes(res["reg_targets"][pos], anchors.reshape(-1, 6)[pos[1]])
    assert np.abs(boxes - gb[pos[0], res["matched_gt"][pos]]).max() <= 4 * 9.54e-07


# ---- 4. scenes whose boxes and occupancy agree -----------------------------------------------------------------------
def test_make_box_scene_batch_is_seeded_padded_and_consistent():
    from disconet_amd import Config
    from disconet_amd import synthetic as S
    from oracle import voxel_ref
    hw, agents, batch, g = 128, 3, 2, 16
    cfg = Config(map_hw=hw)
    half = float(cfg.area_extents[0][1])
    s = S.make_box_scene_batch(batch, agents, hw, seed=5, boxes_per_scene=g)
    s2 = S.make_box_scene_batch(batch, agents, hw, seed=5, boxes_per_scene=g)
    for k in ("bev_seq", "trans_matrices", "num_agent", "gt_boxes", "gt_count"):
        assert torch.equal(s[k], s2[k]), k
    assert not torch.equal(s["gt_boxes"], S.make_box_scene_batch(batch, agents, hw, seed=6, boxes_per_scene=g)["gt_boxes"])
    n = agents * batch
    assert tuple(s["bev_seq"].shape) == (n, 1, hw, hw, 13) and s["bev_seq"].dtype == torch.float32
    assert tuple(s["gt_boxes"].shape) == (n, g, 6) and s["gt_boxes"].dtype == torch.float32
    assert s["gt_count"].dtype == torch.int32 and tuple(s["gt_count"].shape) == (n,)
    ref_bevs, ref_trans, ref_na = S.make_scene_batch(batch, agents, hw)
    assert torch.equal(s["trans_matrices"], ref_trans) and torch.equal(s["num_agent"], ref_na)
    assert int(s["gt_count"].min()) >= 1 and int(s["gt_count"][:batch].min()) == g          # agent 0 sees every box
    ext = np.asarray(cfg.area_extents, dtype=np.float64)
    centres = (np.arange(hw) + 0.5) * cfg.voxel_size[0] - half
    cx, cy = np.meshgrid(centres, centres, indexing="ij")
    for b in range(batch):
        wb = s["world_boxes"][b]
        d = np.hypot(wb[:, None, 0] - wb[None, :, 0], wb[:, None, 1] - wb[None, :, 1]) + 1e9 * np.eye(len(wb))
        assert d.min() >= 6.0 and (0.5 * np.hypot(wb[:, 2], wb[:, 3])).max() <= 3.0 + 1e-9          # circles never meet
        for a in range(agents):
            img = a * batch + b
            c = int(s["gt_count"][img])
            rows = s["gt_boxes"][img].numpy()
            assert not rows[c:].any()
            assert (np.abs(rows[:c, :2]) < half).all() and (rows[:c, 2:4] > 0).all()
            # the agent's boxes are the world boxes under its pose (kept: centre inside the extents, in order)
            T = np.linalg.inv(S.agent_pose(a))
            xy = wb[:, :2] @ T[:2, :2].T + T[:2, 3]
            yaw = np.arctan2(wb[:, 4], wb[:, 5]) - 0.15 * a
            keep = (np.abs(xy[:, 0]) < half) & (np.abs(xy[:, 1]) < half)
            want = np.concatenate([xy, wb[:, 2:4], np.sin(yaw)[:, None], np.cos(yaw)[:, None]], 1)[keep]
            assert c == int(keep.sum())
            assert np.abs(rows[:c] - want).max() < 1e-5
            # the occupancy is the voxelizer's of the image's cloud, and every box shows in it
            dense = voxel_ref.voxelize_occupy(s["points"][img], cfg.voxel_size, ext)
            assert np.array_equal(dense, s["bev_seq"][img, 0].numpy())
            occ = dense.any(-1)
            for x, y, w, h, sn, cs in rows[:c].astype(np.float64):
                u = (cx - x) * cs + (cy - y) * sn
                v = -(cx - x) * sn + (cy - y) * cs
                inside = (np.abs(u) < w / 2) & (np.abs(v) < h / 2)
                assert (occ & inside).sum() >= 1
            assert 0 < occ.mean() < 0.5


# ---- 5. the tools' flags ---------------------------------------------------------------------------------------------
def _load(name):
    import sys
    here = os.path.join(ROOT, "tools", "det")
    if here not in sys.path:
        sys.path.insert(0, here)
    spec = importlib.util.spec_from_file_location(name, os.path.join(here, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_tool_flags_parse():
    t = _load("train_codet")
    a = t.parse_args(["--com", "disco"])
    assert (a.targets, a.pos_thr, a.neg_thr) == ("synthetic", 0.6, 0.45)
    a = t.parse_args(["--targets", "boxes", "--pos_thr", "0.7", "--neg_thr", "0.3", "--scenes", "2"])
    assert (a.targets, a.pos_thr, a.neg_thr, a.scenes) == ("boxes", 0.7, 0.3, 2)
    with pytest.raises(SystemExit):
        t.parse_args(["--targets", "noise"])
    e = _load("eval_codet")
    ap = e.build_eval_parser()
    assert ap.parse_args([]).gt == "synthetic"
    assert ap.parse_args(["--gt", "scene", "--resume", "x/epoch_1.pth"]).gt == "scene"
    assert ap.parse_args(["--gt", "self"]).gt == "self"
    with pytest.raises(SystemExit):
        ap.parse_args(["--gt", "boxes"])


def test_default_targets_build_the_same_first_step_data():
    from disconet_amd.synthetic import make_scene_batch, make_train_targets
    t = _load("train_codet")
    args = t.parse_args(["--batch", "1", "--num_agent", "2"])
    hw, agents = 32, 2
    data = t.step_data(args, agents, hw, epoch=1, it=0, device="cpu")
    seed = 1000
    bevs, trans, na = make_scene_batch(1, agents, hw, jitter_seed=seed)
    labels, reg, mask = make_train_targets(agents, hw, seed=seed)
    want = {"bev_seq": bevs, "trans_matrices": trans, "num_agent": na, "labels": labels, "reg_targets": reg,
            "reg_loss_mask": mask}
    assert sorted(data) == sorted(want)
    for k, v in want.items():
        assert data[k].dtype == v.dtype and torch.equal(data[k], v), k
    # data-parallel ranks draw their own seeds, as before
    d3 = t.step_data(args, agents, hw, epoch=2, it=3, world=4, rank=1, device="cpu")
    assert torch.equal(d3["labels"], make_train_targets(agents, hw, seed=(2 * 1000 + 3) * 4 + 1)[0])
