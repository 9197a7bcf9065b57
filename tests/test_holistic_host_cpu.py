"""The teacher's holistic views without a GPU: the C ABI of dn_voxelize_views (declared, bound, every refusal before a
launch), the source lists of holistic.view_sources, the numpy reference holistic.host_holistic_views on a box scene, the
conditions under which the crafted cloud of tests/holistic_cases.py tells the contract's arithmetic from its two most
likely wrong implementations, and the training tool's KD form on box scenes."""
import ctypes
import importlib.util
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests import holistic_cases as H
from tests.conftest import ROOT

NAME = "dn_voxelize_views"


def _lib():
    from disconet_amd import _lib
    return _lib.load()


# ---- 1. the C ABI ----------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_point_and_the_binding_exists():
    from disconet_amd import _lib
    raw = open(os.path.join(ROOT, "include", "disconet_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert re.search(r"\b%s\s*\(" % NAME, text)
    assert NAME in _lib.SIGNATURES
    assert getattr(_lib.load(), NAME) is not None
    assert _lib.load().dn_version() >= 139
    import disconet_amd
    assert disconet_amd.holistic.holistic_views is disconet_amd.holistic_views
    assert callable(disconet_amd.ops.voxelize_views)
    # the header states the arithmetic and that the upstream merge is not pinned
    assert "((T[r][0]*x + T[r][1]*y) + T[r][2]*z) + T[r][3]" in raw and "NOT PINNED" in raw


POINTERS = ("pts", "src_begin", "src_count", "src_view", "src_pose", "poses", "vs", "ext", "dims")


def _call(null=(), n_pts=1000, stride=4, n_pose=9, n_src=12, max_count=100, n_views=3, z_hi=2.0, dims=(256, 256, 13),
          dense=True, bits=True):
    """dn_voxelize_views with fake (never dereferenced) device pointers: every refusal happens before a launch."""
    lib = _lib()
    fake = ctypes.c_void_p(0x1000)
    dev = {k: (None if k in null else fake) for k in POINTERS[:6]}
    vs = None if "vs" in null else (ctypes.c_double * 3)(0.25, 0.25, 0.4)
    ext = None if "ext" in null else (ctypes.c_double * 6)(-32.0, 32.0, -32.0, 32.0, -3.0, z_hi)
    d = None if "dims" in null else (ctypes.c_int * 3)(*dims)
    rc = lib.dn_voxelize_views(dev["pts"], n_pts, stride, dev["src_begin"], dev["src_count"], dev["src_view"],
                               dev["src_pose"], dev["poses"], n_pose, n_src, max_count, n_views, vs, ext, d,
                               fake if dense else None, fake if bits else None, None)
    return rc, lib.dn_last_error().decode()


@pytest.mark.parametrize("which", POINTERS)
def test_null_required_pointer_is_refused(which):
    rc, msg = _call(null=(which,))
    assert rc == -1 and ("null" in msg or "bad" in msg), msg


def test_both_outputs_null_is_refused():
    rc, msg = _call(dense=False, bits=False)
    assert rc == -1 and "null outputs" in msg


@pytest.mark.parametrize("kw,word", [(dict(n_views=0), "0 views"), (dict(n_views=-2), "-2 views"), (dict(n_src=-1), "-1 sources"),
                                     (dict(stride=2), "got 2"), (dict(dims=(256, 256, 12)), "(256,256,12)"),
                                     (dict(dims=(255, 256, 13)), "(255,256,13)")])
def test_bad_sizes_are_refused_and_named(kw, word):
    rc, msg = _call(**kw)
    assert rc == -1 and word in msg, msg


def test_33_height_bins_with_bits_are_refused():
    # z in (-3, 9.9) at 0.4 m: ceil(24.75) - floor(-7.5) = 33 bins, too many for one word per pixel
    rc, msg = _call(z_hi=9.9, dims=(256, 256, 33))
    assert rc == -1 and "33 height bins" in msg, msg


def test_python_wrapper_refuses_host_tensors_and_unknown_outputs():
    from disconet_amd import _lib as L, holistic, ops
    i = torch.zeros(1, dtype=torch.int32)
    c = H.cfg(64)
    with pytest.raises(L.DnError):
        ops.voxelize_views(torch.zeros(4, 3), i, i, i, i, torch.eye(4)[None], 1, 4, c.voxel_size, c.area_extents, c.map_dims)
    with pytest.raises(ValueError):
        holistic.pack_clouds([np.zeros((4, 3), np.float32), np.zeros((4, 4), np.float32)], "cpu")
    with pytest.raises(ValueError):
        holistic.pack_clouds([np.zeros((4, 2), np.float32)], "cpu")
    pts, off = holistic.pack_clouds([np.ones((4, 4), np.float32), np.zeros((0, 4), np.float32), torch.ones(2, 4)], "cpu")
    assert tuple(pts.shape) == (6, 4) and pts.dtype == torch.float32 and off.tolist() == [0, 4, 4, 6]


# ---- 2. the source lists ----------------------------------------------------------------------------------------------
def test_view_sources_follow_the_reference_loop_order():
    from disconet_amd.holistic import view_sources
    A, B = 3, 2
    s = view_sources([3, 3], A, B)
    want = [(j * B + b, i * B + b, -1 if i == j else (b * A + i) * A + j) for b in range(B) for i in range(A) for j in range(A)]
    assert list(zip(s["src_image"], s["src_view"], s["src_pose"])) == want and s["n_views"] == A * B
    # the same (b, i, j) order as the training fusion's lists
    from disconet_amd.train import _fusion_index_lists
    f = _fusion_index_lists(A, False, [3, 3], B, "cpu")
    warps = [(b, i, j) for b in range(B) for i in range(A) for j in range(A) if j != i]
    assert f["_poses_idx"].tolist() == [list(w) for w in warps]
    assert [p for p in s["src_pose"] if p >= 0] == [(b * A + i) * A + j for b, i, j in warps]


def test_view_sources_ragged_batch():
    from disconet_amd.holistic import view_sources
    A, B = 3, 2
    s = view_sources([3, 2], A, B)
    per_view = {v: [] for v in range(A * B)}
    for img, v, p in zip(s["src_image"], s["src_view"], s["src_pose"]):
        per_view[v].append((img, p))
    assert per_view[2 * B + 1] == []                                   # the padded ego (agent 2 of scene 1): no sources
    assert all(len(per_view[i * B + 0]) == 3 for i in range(3)) and all(len(per_view[i * B + 1]) == 2 for i in range(2))
    assert 2 * B + 1 not in s["src_image"]                             # no live ego lists the padded agent's cloud
    assert all(p == -1 or (p % A < 2 and (p // A) % A < 2) for (img, p) in per_view[1] + per_view[B + 1])


def test_view_sources_ego_range_and_own_views():
    from disconet_amd.holistic import view_sources
    A, B = 3, 2
    full = view_sources([3, 3], A, B)
    part = view_sources([3, 3], A, B, ego_first=1, ego_count=2)
    assert part["n_views"] == 2 * B and sorted(set(part["src_view"])) == list(range(2 * B))
    pick = [(img, v - 1 * B, p) for img, v, p in zip(full["src_image"], full["src_view"], full["src_pose"]) if v >= 1 * B]
    assert list(zip(part["src_image"], part["src_view"], part["src_pose"])) == pick
    own = view_sources([3, 2], A, B, ego_first=1, ego_count=2, own=True)
    base = view_sources([3, 2], A, B, ego_first=1, ego_count=2)
    k = len(base["src_image"])
    assert own["n_views"] == 2 * base["n_views"] and own["src_image"][:k] == base["src_image"]
    tail = list(zip(own["src_image"][k:], own["src_view"][k:], own["src_pose"][k:]))
    assert tail == [(1 * B + 0, 2 * B + 0, -1), (2 * B + 0, 2 * B + B + 0, -1), (1 * B + 1, 2 * B + 1, -1)]
    with pytest.raises(ValueError):
        view_sources([3, 3], A, B, ego_first=2, ego_count=2)
    with pytest.raises(ValueError):
        view_sources([4, 3], A, B)


# ---- 3. the numpy reference on a box scene ----------------------------------------------------------------------------
def test_host_holistic_views_on_the_64_map_scene():
    from disconet_amd.holistic import host_holistic_views
    s = H.scene_64()
    own, hol = s["bev_seq"].numpy(), s["bev_seq_teacher"].numpy()
    assert own.shape == hol.shape == (6, 1, 64, 64, 13) and hol.dtype == np.float32
    assert tuple(int(v.sum()) for v in own) == H.OWN_CELLS_64
    assert tuple(int(v.sum()) for v in hol) == H.HOLISTIC_CELLS_64
    assert set(np.unique(hol)) == {0.0, 1.0}
    assert (hol >= own).all()                          # the ego's own cloud is not transformed: its cells are all there
    gain = [int(h.sum() - o.sum()) for h, o in zip(hol, own)]
    print("cells gained per view", gain)
    assert min(gain) >= 100
    swapped = host_holistic_views(s["points"], s["trans_matrices"].transpose(1, 2), [3, 3], 2, H.cfg(64))["dense"]
    differ = [int((a != b).sum()) for a, b in zip(swapped, hol)]
    print("cells that differ with the pose direction swapped", differ)
    assert min(differ) >= 400
    both = host_holistic_views(s["points"], s["trans_matrices"], s["num_agent"], 2, H.cfg(64), own=True)
    assert np.array_equal(both["dense"], hol) and np.array_equal(both["own_dense"], own)


def test_box_scene_teacher_flag_adds_one_key_and_changes_nothing_else():
    from disconet_amd.holistic import host_holistic_views
    from disconet_amd.synthetic import make_box_scene_batch
    with_t = H.scene_64()
    plain = make_box_scene_batch(**H.SCENE_64)
    assert set(with_t) == set(plain) | {"bev_seq_teacher"}
    for k, v in plain.items():
        if isinstance(v, torch.Tensor):
            assert v.dtype == with_t[k].dtype and np.array_equal(v.numpy().view(np.uint8), with_t[k].numpy().view(np.uint8)), k
        else:
            assert len(v) == len(with_t[k]) and all(a.dtype == b.dtype and np.array_equal(a, b) for a, b in zip(v, with_t[k])), k
    ref = host_holistic_views(plain["points"], plain["trans_matrices"], [3, 3], 2, H.cfg(64))["dense"]
    assert np.array_equal(with_t["bev_seq_teacher"].numpy(), ref)


# ---- 4. the crafted cloud tells the contract from its likely wrong implementations -----------------------------------
@pytest.mark.parametrize("hw", [64, 128, 256])
def test_crafted_cloud_separates_the_contract_from_float32_and_unrounded_float64(hw):
    T = H.crafted_pose()
    pts = H.near_face_cloud(T, hw)
    assert pts.shape == (7 * 4096, 3) and pts.dtype == np.float32
    contract = H.cells(H.coords_contract(pts, T), hw)
    f32 = H.cells(H.coords_float32_arithmetic(pts, T), hw)
    f64 = H.cells(H.coords_float64_unrounded(pts, T), hw)
    n32, n64 = int((contract != f32).sum()), int((contract != f64).sum())
    cells = int((H.grid_of(contract, hw) != H.grid_of(f32, hw)).sum())
    print("map %d: %d points land elsewhere in float32 arithmetic, %d without the rounding to float32; the float32 form's "
          "grid differs in %d cells" % (hw, n32, n64, cells))
    assert n32 >= 256 and n64 >= 256 and cells >= 16
    # the helper's rule is the package's: the grid of the contract's cells is host_occupancy of the contract's coordinates
    from disconet_amd.synthetic import host_occupancy
    c = H.cfg(hw)
    assert np.array_equal(H.grid_of(contract, hw), host_occupancy(H.coords_contract(pts, T), c.voxel_size, c.area_extents,
                                                                 c.map_dims))


# ---- 5. the training tool ---------------------------------------------------------------------------------------------
def _tool():
    spec = importlib.util.spec_from_file_location("train_codet_tool", os.path.join(ROOT, "tools", "det", "train_codet.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_train_tool_accepts_kd_on_box_scenes():
    tool = _tool()
    args = tool.parse_args(["--targets", "boxes", "--kd_flag", "1"])
    assert args.targets == "boxes" and args.kd_flag == 1
    src = inspect.getsource(tool.main)
    assert "no teacher view" not in src and "SystemExit(\"--targets boxes" not in src
    assert "teacher=bool(args.kd_flag)" in inspect.getsource(tool.step_data)
    assert "INITIAL weights" in src
