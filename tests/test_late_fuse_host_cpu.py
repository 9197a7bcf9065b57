"""Host side of `--com late` and `--com lowerbound`: the contract of dn_late_fuse as postprocess.host_late_fuse states it
in numpy (geometry against the box scenes, the edges of the contract), the C ABI's new symbols and refusals, the NoFusion
model and the tools' command lines.  No GPU.

The geometry bound (test_geometry_agrees_with_the_scenes) is derived, not tuned.  u = 2^-24 is the relative rounding of
fp32, L = 32 m the half width of the extents: every stored and every returned centre coordinate is below L.
  position, per coordinate
    the stored row          |x|, |y| < L rounded to fp32: L u each, and the rotation adds the two: 2 L u
    the matrix              a rotation entry (|m| <= 1) is off by u / 2, times a coordinate below L, two entries: L u
                            the translation entry is off by |t| u
    the result              |x'| < L rounded to fp32: L u
    the float64 steps       six operations on values below 2 L: 1e-12 covers them
  heading, per component
    the stored (sin, cos)   u / 2 each, the rotation adds the two: u
    the matrix              two entries off by u / 2, times components of at most 1: u
    the result              u / 2
For orientation: measured on the CPU over the 250 to 270 neighbour rows of each seed, 2.4e-6 m and 8.4e-8 at worst; the
bounds are 7.6e-6 + |t| u = 9.2e-6 m and 1.5e-7."""
import ctypes
import importlib.util
import os
import re
from unittest import mock

import numpy as np
import pytest
import torch

from tests import late_cases as lc
from tests.conftest import ROOT

U = 2.0 ** -24
L = 32.0


def _fuse(det, trans, live, B, A, **kw):
    from disconet_amd.postprocess import host_late_fuse
    return host_late_fuse(det, trans, live, B, A, **kw)


# ---------------------------------------------------------------------------
# geometry
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_geometry_agrees_with_the_scenes(seed):
    from disconet_amd.synthetic import boxes_in_agent_frame, make_box_scene_batch
    A, B = 5, 2
    scene = make_box_scene_batch(batch_size=B, num_agent=A, device=None, clutter=0, seed=seed)
    gt, gc, trans = scene["gt_boxes"].numpy(), scene["gt_count"].numpy(), scene["trans_matrices"]
    k = gt.shape[1]
    rng = np.random.RandomState(100 + seed)
    scores = ((rng.permutation(A * B * k) + 1.0) / (A * B * k + 1.0)).astype(np.float32).reshape(A * B, k)
    det = {"boxes": gt, "scores": scores, "count": gc}
    t_max = float(np.abs(trans.numpy()[..., :2, 3]).max())
    pos_bound = 2 * L * U + L * U + t_max * U + L * U + 1e-12
    head_bound = U + U + U / 2 + 1e-12
    worst_pos = worst_head = 0.0
    n_rows = n_from_neighbours = 0
    for only_v2i in (False, True):
        out = _fuse(det, trans, [A] * B, B, A, top_k=A * k, extents=lc.EXTENTS, only_v2i=only_v2i)
        for b in range(B):
            world = scene["world_boxes"][b]
            truth = [boxes_in_agent_frame(world, a) for a in range(A)]
            inside = [(np.abs(t[:, 0]) < L) & (np.abs(t[:, 1]) < L) for t in truth]
            # the condition on the inputs: no centre within 1e-3 m of an extent edge, in any agent's frame
            for t in truth:
                assert np.abs(np.abs(t[:, :2]) - L).min() > 1e-3
            # row of world box w in agent a's ground truth (the rows are the boxes inside, in world order)
            row_of = [np.cumsum(m) - 1 for m in inside]
            for i in range(A):
                lst = [i] + [j for j in range(A) if j != i and not (only_v2i and i != 0 and j != 0)]
                want = {}
                for w in range(len(world)):
                    holders = [j for j in lst if inside[j][w]]
                    if inside[i][w] and holders:
                        best = max(holders, key=lambda j: scores[j * B + b, row_of[j][w]])
                        want[best * k + row_of[best][w]] = w
                img = i * B + b
                c = int(out["count"][img])
                assert sorted(out["source"][img, :c].tolist()) == sorted(want), (seed, only_v2i, b, i)
                for r in range(c):
                    src = int(out["source"][img, r])
                    w = want[src]
                    got = out["boxes"][img, r].astype(np.float64)
                    assert out["scores"][img, r] == scores[(src // k) * B + b, src % k]
                    dp = np.abs(got[:2] - truth[i][w, :2]).max()
                    dh = np.abs(got[4:] - truth[i][w, 4:]).max()
                    assert dp <= pos_bound and dh <= head_bound, (dp, pos_bound, dh, head_bound)
                    assert np.array_equal(got[2:4], gt[(src // k) * B + b, src % k, 2:4].astype(np.float64))
                    if src // k != i:
                        worst_pos, worst_head = max(worst_pos, dp), max(worst_head, dh)
                        n_from_neighbours += 1
                    else:
                        assert np.array_equal(out["boxes"][img, r], gt[img, src % k])      # an own row: the same bits
                    n_rows += 1
    print("\nlate fusion geometry, seed %d: %d rows, %d from neighbours, worst %.3e m (bound %.3e), heading %.3e (bound %.3e)"
          % (seed, n_rows, n_from_neighbours, worst_pos, pos_bound, worst_head, head_bound))
    assert n_from_neighbours >= 20 and worst_pos > 0


# ---------------------------------------------------------------------------
# contract edges
# ---------------------------------------------------------------------------
def _by_hand(det, trans, live, B, A, i, b, top_k, only_v2i=False, extents=None):
    """the ordered candidates of ego (i, b) without the NMS, written independently of host_late_fuse: (agent, row) pairs"""
    n = max(0, min(int(live[b]), A))
    lst = [i] + ([j for j in range(n) if j != i and not (only_v2i and i != 0 and j != 0)] if i < n else [])
    k = det["scores"].shape[1]
    cand = []
    for pos, j in enumerate(lst):
        img = j * B + b
        for r in range(max(0, min(int(det["count"][img]), k))):
            s = float(det["scores"][img, r])
            if not (np.isfinite(s) and s >= 0):
                continue
            if pos and extents is not None:
                M = trans[b, i, j].numpy().astype(np.float64)
                x, y = (float(v) for v in det["boxes"][img, r, :2])
                xp = float(np.float32((M[0, 0] * x + M[0, 1] * y) + M[0, 3]))
                yp = float(np.float32((M[1, 0] * x + M[1, 1] * y) + M[1, 3]))
                if not (extents[0][0] < xp < extents[0][1] and extents[1][0] < yp < extents[1][1]):
                    continue
            cand.append((-s, pos, r, j))
    cand.sort(key=lambda t: t[:3])
    return [(j, r) for _, _, r, j in cand[:top_k]]


def test_order_ties_scores_counts_and_padding():
    """iou_thr = 2 suppresses nothing: the output is the ordered candidate list itself"""
    A, B, k = 4, 2, 12
    trans = lc.trans_of(A, B)
    det = lc.plant_score_edges(lc.random_rows(A, B, k, seed=5), B)
    live = [4, 3]
    for only_v2i in (False, True):
        for top_k, ext in ((A * k, None), (A * k, lc.EXTENTS), (7, None)):
            out = _fuse(det, trans, live, B, A, top_k=top_k, iou_thr=2.0, extents=ext, only_v2i=only_v2i)
            assert out["boxes"].shape == (A * B, top_k, 6) and out["source"].dtype == np.int32
            for b in range(B):
                for i in range(A):
                    want = _by_hand(det, trans, live, B, A, i, b, top_k, only_v2i, ext)
                    img = i * B + b
                    c = int(out["count"][img])
                    assert c == len(want)
                    assert out["source"][img, :c].tolist() == [j * k + r for j, r in want]
                    assert (out["source"][img, c:] == -1).all() and not out["boxes"][img, c:].any()
                    assert not out["scores"][img, c:].any()
                    for q, (j, r) in enumerate(want):
                        assert out["scores"][img, q].tobytes() == det["scores"][j * B + b, r].tobytes()      # -0 stays -0
                        if j == i:
                            assert out["boxes"][img, q].tobytes() == det["boxes"][img, r].tobytes()
    # what the planted rows mean, spelled out on ego 1 of scene 0 (live 4; agent 0's count is -3: no rows)
    out = _fuse(det, trans, live, B, A, top_k=A * k, iou_thr=2.0)
    src = out["source"][1 * B + 0, :int(out["count"][1 * B + 0])].tolist()
    assert not any(s // k == 0 for s in src)                                  # count below 0
    assert not any(s % k in (0, 3, 4, 5) for s in src)                        # NaN, negative, +inf, -inf
    half = [s for s in src if s % k in (6, 7)]
    assert half == [1 * k + 6, 1 * k + 7, 2 * k + 6, 2 * k + 7, 3 * k + 6, 3 * k + 7]      # ties: list position, then row
    zeros = [s for s in src if s % k in (1, 2)]
    assert zeros == [1 * k + 1, 1 * k + 2, 2 * k + 1, 2 * k + 2, 3 * k + 1, 3 * k + 2]      # -0 == +0: position, then row
    assert src[-len(zeros):] == zeros
    # the last agent's last scene has count k + 5: clamped, every finite non-negative row of it is there
    own = out["source"][(A - 1) * B + 1, :int(out["count"][(A - 1) * B + 1])]
    assert sorted(s % k for s in own.tolist() if s // k == A - 1) == [1, 2, 6, 7, 8, 9, 10, 11]


def test_empty_agents_padded_egos_and_ego_ranges():
    A, B, k = 5, 2, 6
    trans = lc.trans_of(A, B)
    det = lc.random_rows(A, B, k, seed=9, counts="full")
    det["count"][2 * B + 1] = 0                                               # agent 2 of scene 1 found nothing
    live = [0, 5]
    full = _fuse(det, trans, live, B, A, iou_thr=2.0, top_k=A * k)
    for i in range(A):                                                        # scene 0: every ego is padded -- its own rows alone
        img = i * B
        assert int(full["count"][img]) == k and set(full["source"][img, :k] // k) == {i}
    assert int(full["count"][2 * B + 1]) == 4 * k and 2 not in set(full["source"][2 * B + 1, :4 * k] // k)
    assert int(full["count"][0 * B + 1]) == 4 * k
    part = _fuse(det, trans, live, B, A, iou_thr=2.0, top_k=A * k, ego_first=1, ego_count=2)
    for key in lc.KEYS:
        assert np.array_equal(part[key], full[key][B:3 * B]), key
    empty = dict(det, count=np.zeros(A * B, dtype=np.int32))
    none = _fuse(empty, trans, live, B, A)
    assert not none["count"].any() and (none["source"] == -1).all() and not none["boxes"].any() and not none["scores"].any()
    for first, count in ((-1, 2), (4, 2), (0, 0), (5, 1)):
        with pytest.raises(ValueError, match="ego range"):
            _fuse(det, trans, live, B, A, ego_first=first, ego_count=count)
    # pad_detections' dict and tensors are taken too
    from disconet_amd.postprocess import pad_detections
    lists_b = [det["boxes"][n, :det["count"][n]] for n in range(A * B)]
    lists_s = [det["scores"][n, :det["count"][n]] for n in range(A * B)]
    padded = pad_detections(lists_b, lists_s, width=k)
    again = _fuse({key: torch.from_numpy(v) for key, v in padded.items()}, trans, torch.tensor(live), B, A, iou_thr=2.0,
                  top_k=A * k)
    assert not lc.same_bytes(again, full)


def test_copies_are_suppressed_or_kept_and_top_k_truncates():
    """every agent holds a copy of each object: at the default threshold one row per object survives, the best-scored
    copy; at a threshold no IoU exceeds every copy stays; a top_k below the candidate count cuts the list before the NMS"""
    A, B, objects, k = 4, 2, 6, 8
    trans = lc.trans_of(A, B)
    det = lc.copies(A, B, objects, k, seed=4, trans=trans)
    live = [4, 4]
    one = _fuse(det, trans, live, B, A, top_k=A * k)
    every = _fuse(det, trans, live, B, A, top_k=A * k, iou_thr=2.0)
    cut = _fuse(det, trans, live, B, A, top_k=5)
    for b in range(B):
        for i in range(A):
            img = i * B + b
            assert int(one["count"][img]) == objects and int(every["count"][img]) == A * objects
            rows = one["source"][img, :objects] % k
            assert sorted(rows.tolist()) == list(range(objects))
            for q in range(objects):
                r = int(rows[q])
                assert one["scores"][img, q] == max(det["scores"][j * B + b, r] for j in range(A))
            assert np.array_equal(cut["source"][img, :int(cut["count"][img])],
                                  [s for s in one["source"][img, :objects]
                                   if s in set(every["source"][img, :5].tolist())])


def test_extent_edges_and_extents_off():
    A, B, k = 4, 2, 40
    trans = lc.trans_of(A, B)
    det, rows = lc.plant_extent_edge(lc.random_rows(A, B, k, seed=6, counts="full"), trans, B, ego=1, nbr=2)
    on = _fuse(det, trans, [4, 4], B, A, top_k=A * k, iou_thr=2.0, extents=lc.EXTENTS)
    off = _fuse(det, trans, [4, 4], B, A, top_k=A * k, iou_thr=2.0)
    img = 1 * B + 0
    kept = [r for r in rows if 2 * k + r in set(on["source"][img, :int(on["count"][img])].tolist())]
    assert 0 < len(kept) < len(rows), (kept, rows)                    # rows on either side of the edges
    assert all(2 * k + r in set(off["source"][img].tolist()) for r in rows)
    assert int(off["count"][img]) == A * k                             # extents off: every row is a candidate
    own = 2 * B + 0                                                    # the neighbour itself keeps all of its own rows
    assert all(2 * k + r in set(on["source"][own].tolist()) for r in rows)


# ---------------------------------------------------------------------------
# the library and the models
# ---------------------------------------------------------------------------
def test_library_has_the_entry_points_and_refuses_without_a_gpu():
    from disconet_amd import _lib
    lib = _lib.load()
    assert lib.dn_version() >= 148
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "disconet_hip.h")).read(), flags=re.S)
    for name, n_args, restype in (("dn_late_fuse_workspace_bytes", 6, ctypes.c_size_t), ("dn_late_fuse", 22, ctypes.c_int)):
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, text)
        assert decl and len(decl.group(1).split(",")) == n_args, name
        assert _lib.SIGNATURES[name][0] is restype and len(_lib.SIGNATURES[name][1]) == n_args
        assert list(getattr(lib, name).argtypes) == list(_lib.SIGNATURES[name][1])
    assert lib.dn_late_fuse_workspace_bytes(2, 5, 300, 300, 0, 5) > 0
    assert lib.dn_late_fuse_workspace_bytes(1, 8, 1024, 1024, 0, 8) > 0
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)                  # a non-null pointer nothing reads: every call below is refused first
    ext = (ctypes.c_double * 4)(-32.0, 32.0, -32.0, 32.0)

    def call(batch=2, agents=4, k_in=8, only_v2i=0, ego_first=0, ego_count=4, top_k=8, iou_thr=0.01, use_ext=0, ext=ext,
             ptr=p, ws_bytes=1 << 30):
        return lib.dn_late_fuse(ptr, p, p, p, p, batch, agents, k_in, only_v2i, ego_first, ego_count, top_k, iou_thr,
                                use_ext, ext, p, p, p, p, p, ws_bytes, None)

    refused = [
        (dict(ptr=None), b"null"), (dict(batch=0), b"batch"), (dict(agents=17, ego_count=17), b"agents"),
        (dict(k_in=0), b"k_in"), (dict(k_in=1025, agents=2, ego_count=2), b"k_in"),
        (dict(agents=16, ego_count=16, k_in=600), b"at most 8192"), (dict(top_k=0), b"top_k"), (dict(top_k=1025), b"top_k"),
        (dict(iou_thr=float("nan")), b"iou_thr"), (dict(iou_thr=-0.5), b"iou_thr"), (dict(iou_thr=float("inf")), b"iou_thr"),
        (dict(ego_first=-1), b"ego range"), (dict(ego_first=3, ego_count=2), b"ego range"), (dict(ego_count=0), b"ego range"),
        (dict(use_ext=1, ext=None), b"xy_extents"),
        (dict(use_ext=1, ext=(ctypes.c_double * 4)(32.0, -32.0, -32.0, 32.0)), b"extents"),
        (dict(use_ext=1, ext=(ctypes.c_double * 4)(float("nan"), 32.0, -32.0, 32.0)), b"extents"),
        (dict(ws_bytes=16), b"workspace"),
    ]
    for kw, word in refused:
        assert call(**kw) == -1, kw
        assert word in lib.dn_last_error(), (kw, lib.dn_last_error())
    for shape in ((0, 4, 8, 8, 0, 4), (2, 17, 8, 8, 0, 17), (2, 4, 0, 8, 0, 4), (2, 4, 1025, 8, 0, 4), (2, 16, 600, 8, 0, 16),
                  (2, 4, 8, 0, 0, 4), (2, 4, 8, 1025, 0, 4), (2, 4, 8, 8, -1, 4), (2, 4, 8, 8, 3, 2), (2, 4, 8, 8, 0, 0)):
        assert lib.dn_late_fuse_workspace_bytes(*shape) == 0, shape
    # the Python surface refuses host tensors: there is no CPU path behind late_fuse
    from disconet_amd import late_fuse
    det = lc.random_rows(2, 1, 4, seed=0)
    with pytest.raises(_lib.DnError):
        late_fuse({k: torch.from_numpy(v) for k, v in det.items()}, lc.trans_of(2, 1), torch.tensor([2]), 1, 2)


def test_nofusion_owns_no_attention_parameters_and_the_modes_are_listed():
    import disconet_amd
    from disconet_amd import COM_MODES, DET_COM_MODES, Config, DiscoNet, NoFusion, build_model
    from disconet_amd.fusion_modes import NoFusionTrainEngine, ReduceTrainEngine
    assert COM_MODES == ("disco", "sum", "mean", "max")
    assert DET_COM_MODES == ("disco", "sum", "mean", "max", "lowerbound", "late")
    for name in ("NoFusion", "DET_COM_MODES", "late_fuse"):
        assert name in disconet_amd.__all__ and hasattr(disconet_amd, name)
    disco = DiscoNet(Config())
    want = {k for k in disco.state_dict() if not k.startswith("pixel_weighted_fusion.")}
    for com in ("lowerbound", "late"):
        m = build_model(com, Config(), layer=3, in_channels=13, kd_flag=True, num_agent=5, compress_level=0, only_v2i=False)
        assert type(m) is NoFusion and m.com == "lowerbound" and not hasattr(m, "pixel_weighted_fusion")
        assert set(m.state_dict()) == want
        with pytest.raises(RuntimeError, match="Unexpected key"):
            m.load_state_dict(disco.state_dict())
        m.load_state_dict({"module." + k: v for k, v in disco.state_dict().items() if k in want})
        assert m._fusion_plan(0) == {}
        assert m._train_engine_class() is NoFusionTrainEngine and issubclass(NoFusionTrainEngine, ReduceTrainEngine)
        # fuse() hands back the served egos' own maps and reads neither the poses nor the counts
        feat = torch.arange(5 * 2 * 3 * 3 * 4, dtype=torch.float32).reshape(10, 3, 3, 4)
        assert m.fuse(feat, None, None, 2, None) is feat
        assert torch.equal(m.fuse(feat, None, None, 2, None, ego_first=1, ego_count=2), feat[2:6])
        with pytest.raises(ValueError, match="ego range"):
            m.fuse(feat, None, None, 2, None, ego_first=4, ego_count=2)
        with pytest.raises(ValueError, match="no agent weights"):
            m.fuse(feat, None, None, 2, None, want_weights=True)
    with pytest.raises(ValueError, match="v2v"):
        build_model("v2v", Config())
    with pytest.raises(ValueError, match="upperbound"):
        build_model("upperbound", Config())


# ---------------------------------------------------------------------------
# the tools
# ---------------------------------------------------------------------------
class _Reached(Exception):
    pass


def _tool(rel):
    spec = importlib.util.spec_from_file_location("late_tool_" + rel.replace("/", "_").replace(".py", ""),
                                                  os.path.join(ROOT, "tools", rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("rel", ["det/detect_codet.py", "det/eval_codet.py", "track/sort_codet.py", "track/eval_sort.py"])
def test_det_and_track_tools_take_lowerbound_and_late(rel, monkeypatch):
    mod = _tool(rel)
    with pytest.raises(SystemExit, match=r"disco \| sum \| mean \| max \| lowerbound \| late"):
        mod.main(["--com", "v2v"])
    asked = []

    def build_model(com, config, **kw):                  # what the tool builds its detector with: the mode must arrive here
        asked.append((com, kw["num_agent"]))
        raise _Reached()
    from disconet_amd import detector
    monkeypatch.setattr(torch.cuda, "set_device", lambda *a, **kw: None)
    monkeypatch.setattr(detector, "build_model", build_model)      # Detector's: the tools' one construction site
    extra = []
    if rel.startswith("track/"):                         # (the tracker and the metrics are built first, on the GPU: stand-ins)
        monkeypatch.setattr(mod, "tracking", mock.MagicMock())
        extra = ["--source", "net"]
    for com in ("lowerbound", "late"):
        with pytest.raises(_Reached):
            mod.main(["--com", com, "--num_agent", "3"] + extra)
    assert asked == [("lowerbound", 3), ("late", 3)]
    # the tool constructs its Detector with com == "late": Detector.tail then runs late_fuse behind detect(), which
    # tests/test_detector_cpu.py :: test_tail_reaches_late_fuse_for_late_only asserts on the call path itself
    made = []

    class _Detector:
        def __init__(self, com, config, num_agent, batch_size, **kw):
            made.append((com, num_agent, batch_size, kw["only_v2i"], kw["iou_thr"]))
            raise _Reached()
    import codet_common                                  # (tools/det: the tool put it on the path)
    monkeypatch.setattr(codet_common, "Detector", _Detector)
    with pytest.raises(_Reached):
        mod.main(["--com", "late", "--num_agent", "3", "--batch", "2", "--only_v2i", "1", "--iou_thr", "0.05"] + extra)
    assert made == [("late", 3, 2, True, 0.05)]


def test_train_tool_takes_lowerbound_and_refuses_late(monkeypatch):
    mod = _tool("det/train_codet.py")
    with pytest.raises(SystemExit, match="train --com lowerbound and pass its checkpoint"):
        mod.main(["--com", "late"])
    with pytest.raises(SystemExit, match=r"disco \| sum \| mean \| max"):
        mod.main(["--com", "v2v"])
    asked = []

    def build_model(com, config, **kw):
        asked.append((com, kw["num_agent"]))
        raise _Reached()
    monkeypatch.setattr(torch.cuda, "set_device", lambda *a, **kw: None)
    monkeypatch.setattr(mod, "build_model", build_model)
    with pytest.raises(_Reached):
        mod.main(["--com", "lowerbound", "--num_agent", "3"])
    assert asked == [("lowerbound", 3)]
