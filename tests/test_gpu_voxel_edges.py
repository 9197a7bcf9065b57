"""The voxel front end (disconet_amd/csrc/voxel.hip) at the grids, tails, capacities and edges the default geometry never
reaches: every kernel against the numpy oracle or the numpy statements of tests/voxel_cases.py, every comparison exact.
tests/test_voxel_cases_cpu.py shows that those statements are the oracle's rule and that the sweeps used here move a cell
when the rule is broken.

What counts as occupied for dn_voxel_compact is `dense != 0`: 1.0, 0.5, -1.0, a subnormal and NaN do, 0.0 and -0.0 do not.
A row of a scatter form belongs to image g when offsets[g] <= row < offsets[g + 1]; a row before offsets[0] or from
offsets[n_images] on belongs to no image and writes nothing."""
import ctypes

import numpy as np
import pytest
import torch

from tests import voxel_cases as V

pytestmark = pytest.mark.gpu

NAMES = list(V.GEOMETRIES)
STRIDE_TRIP = 2048 * 256          # threads of the voxelize and scatter launches: item STRIDE_TRIP is a thread's second


def _ops():
    from disconet_amd import ops
    return ops


def _cuda(a):
    return torch.from_numpy(np.array(a)).cuda()          # a C-ordered copy: the shared references are read-only


def _i32(v):
    return torch.tensor(v, dtype=torch.int32).cuda()


_REFERENCE = {}


def _reference(name, kind):
    """(points, the oracle's grid, the oracle's index list) of a geometry's sweep or cloud: computed once, read-only"""
    if (name, kind) not in _REFERENCE:
        from oracle.voxel_ref import voxelize_occupy
        g = V.GEOMETRIES[name]
        pts = V.sweep(g) if kind == "sweep" else V.cloud(g, 20000, seed=11)
        dense, idx = voxelize_occupy(pts, g.voxel, g.extents, return_indices=True)
        idx = idx.astype(np.int32)
        for a in (pts, dense, idx):
            a.setflags(write=False)
        _REFERENCE[name, kind] = (pts, dense, idx)
    return _REFERENCE[name, kind]


def _views_one_source(pts, g):
    """dn_voxelize_views with one view, one source, pose -1 -> (dense [X, Y, Z], words uint32 [X, Y])"""
    ops = _ops()
    n = pts.shape[0]
    out = ops.voxelize_views(pts, _i32([0]), _i32([n]), _i32([0]), _i32([-1]), torch.eye(4)[None].cuda(),
                             1, n, g.voxel, g.extents, g.dims, want=("dense", "bits"))
    assert tuple(out["dense"].shape) == (1, 1) + g.dims
    return out["dense"][0, 0].cpu().numpy(), out["bits"].data.cpu().numpy().view(np.uint32)[0]


# ---- a. the voxel rule, per geometry --------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["sweep", "cloud"])
@pytest.mark.parametrize("name", NAMES)
def test_voxel_rule_and_index_list(name, kind):
    ops, g = _ops(), V.GEOMETRIES[name]
    pts, want, want_idx = _reference(name, kind)
    dense = ops.voxelize_occupy(_cuda(pts), g.voxel, g.extents, g.dims)
    assert np.array_equal(dense.cpu().numpy(), want)
    idx, m = ops.voxel_compact(dense)
    assert m == len(want_idx)
    assert np.array_equal(idx.cpu().numpy(), want_idx)


@pytest.mark.parametrize("kind", ["sweep", "cloud"])
@pytest.mark.parametrize("name", NAMES)
def test_views_of_one_untransformed_source_are_voxelize_occupy(name, kind):
    g = V.GEOMETRIES[name]
    pts, want, _ = _reference(name, kind)
    dense, words = _views_one_source(_cuda(pts), g)
    assert np.array_equal(dense, want)
    assert np.array_equal(words, V.bits_np(want))


@pytest.mark.parametrize("name", NAMES)
def test_point_strides_3_4_6(name):
    ops, g = _ops(), V.GEOMETRIES[name]
    sweep, cloud = _reference(name, "sweep")[0], _reference(name, "cloud")[0]
    pts = np.concatenate([sweep, cloud])
    from oracle.voxel_ref import voxelize_occupy
    want = voxelize_occupy(pts[:, :3], g.voxel, g.extents)
    filler = np.random.default_rng(2).uniform(-50, 50, size=(len(pts), 2)).astype(np.float32)
    for p in (pts[:, :3], pts, np.concatenate([pts, filler], axis=1)):
        p = _cuda(p)
        assert p.shape[1] in (3, 4, 6)
        assert np.array_equal(ops.voxelize_occupy(p, g.voxel, g.extents, g.dims).cpu().numpy(), want), p.shape[1]
        assert np.array_equal(_views_one_source(p, g)[0], want), p.shape[1]


# ---- b. non-finite and huge coordinates -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["default", "A"])
def test_non_finite_and_huge_points_are_dropped(name):
    from oracle.voxel_ref import voxelize_occupy
    ops, g = _ops(), V.GEOMETRIES[name]
    rng = np.random.default_rng(17)
    valid = V.cloud(g, 3000, seed=7)
    inside = V.cloud(g, 4000, seed=8)
    inside = inside[((g.extents[:, 0] < inside[:, :3]) & (inside[:, :3] < g.extents[:, 1])).all(axis=1)]
    assert len(inside) >= 260
    bad = []
    for col in range(3):
        for value in (np.nan, np.inf, -np.inf, 3e38, -1e30):
            rows = inside[len(bad) * 10:len(bad) * 10 + 10].copy()          # in-grid points but for the one coordinate
            rows[:, col] = value
            bad.append(rows)
    bad = np.concatenate(bad)
    nan_intensity = inside[200:260].copy()
    nan_intensity[:, 3] = np.nan                                               # x, y, z are fine: these rows count
    misses = np.full((64, 4), np.nan, np.float32)                              # what dn_lidar_scan writes for a missed ray
    body = np.concatenate([valid, bad, nan_intensity])
    body = body[rng.permutation(len(body))]
    pts = np.concatenate([body[:1500], misses, body[1500:]]).astype(np.float32)
    want = V.voxelize_np(np.concatenate([valid, nan_intensity]), g)
    assert want.sum() > V.voxelize_np(valid, g).sum()
    assert np.array_equal(voxelize_occupy(pts, g.voxel, g.extents), want)      # numpy drops the others too
    dense = ops.voxelize_occupy(_cuda(pts), g.voxel, g.extents, g.dims)
    assert np.array_equal(dense.cpu().numpy(), want)


# ---- the four scatter forms against their numpy statements -----------------------------------------------------------
def _pieces(t):
    """a device tensor's bytes as uint16 [pieces, 8]"""
    return t.contiguous().view(torch.uint8).cpu().numpy().view(np.uint16).reshape(-1, 8)


def _same_pieces(got, want, what):
    assert got.shape == want.shape, "%s: %s pieces against %s" % (what, got.shape, want.shape)
    bad = np.argwhere((got != want).any(-1))[:, 0]
    assert len(bad) == 0, "%s: %d of %d pieces differ, first %s" % (what, len(bad), len(want), bad[:4].tolist())


def _run_forms(idx, off, n_images, dims):
    """-> the bytes each of the four forms wrote: dense [n, X, Y, Z], sp and hi pieces, words uint32 [n, X, Y]"""
    ops = _ops()
    i, o = _cuda(idx), _cuda(off)
    dense = ops.scatter_dense(i, o, n_images, dims)
    assert tuple(dense.shape) == (n_images, 1) + tuple(dims)
    sp = ops.scatter_dense_sp(i, o, n_images, dims)
    hi = ops.scatter_dense_sp(i, o, n_images, dims, hi_only=True)
    bits = ops.scatter_dense_bits(i, o, n_images, dims)
    assert tuple(bits.data.shape) == (n_images,) + tuple(dims[:2])
    return {"dense": dense[:, 0].cpu().numpy(), "sp": _pieces(sp.data), "hi": _pieces(hi.data),
            "bits": bits.data.cpu().numpy().view(np.uint32)}


def _check_forms(idx, off, n_images, dims):
    want = V.scatter_np(idx, off, n_images, dims)
    got = _run_forms(idx, off, n_images, dims)
    assert np.array_equal(got["dense"], want), "scatter_dense"
    _same_pieces(got["sp"], V.sp_np(want), "scatter_dense_sp")
    _same_pieces(got["hi"], V.sp_np(want, hi_only=True), "scatter_dense_sp(hi_only)")
    assert np.array_equal(got["bits"], V.bits_np(want)), "scatter_dense_bits"
    return want, got


# ---- c. the second trip of the stride loops -----------------------------------------------------------------------------
def _second_trip_cells():
    """STRIDE_TRIP + 300 cells of geometry D: the first STRIDE_TRIP repeat 20 000 cells with ix < 28, the last 300 are
    distinct cells with ix >= 28, which only a thread's second trip reaches"""
    g = V.GEOMETRIES["D"]
    rng = np.random.default_rng(23)
    x, y, z = g.dims
    some = np.stack([rng.integers(0, 28, 20000), rng.integers(0, y, 20000), rng.integers(0, z, 20000)], axis=1)
    first = some[rng.integers(0, len(some), STRIDE_TRIP)]
    late = rng.choice((x - 28) * y * z, size=300, replace=False)
    last = np.stack([28 + late // (y * z), late // z % y, late % z], axis=1)
    return g, np.concatenate([first, last]).astype(np.int32)


def test_voxelize_second_trip():
    ops = _ops()
    g, cells = _second_trip_cells()
    # a point three quarters into its cell: z bin 0 is the half cell [-3.0, -2.8), its middle would lie on the extent
    inner = ((cells + V.min_cell(g) + 0.75) * np.asarray(g.voxel)).astype(np.float32)
    pts = np.concatenate([inner, np.zeros((len(cells), 1), np.float32)], axis=1)
    want = V.scatter_np(cells, [0, len(cells)], 1, g.dims)[0]
    assert np.array_equal(V.voxelize_np(pts, g), want) and want[28:].sum() == 300
    dense = ops.voxelize_occupy(_cuda(pts), g.voxel, g.extents, g.dims)
    assert np.array_equal(dense.cpu().numpy(), want)
    assert np.array_equal(_views_one_source(_cuda(pts), g)[0], want)


def test_scatter_forms_second_trip():
    g, cells = _second_trip_cells()
    off = np.array([0, STRIDE_TRIP // 2 + 17, len(cells)], np.int32)
    want, _ = _check_forms(cells, off, 2, g.dims)
    assert want[1, 28:].sum() == 300 and want[0, 28:].sum() == 0


# ---- d. dn_voxel_compact on hand-made grids -----------------------------------------------------------------------------
def _compact_is(dense):
    """dense: numpy [X, Y, Z] float32 -> the checked (indices, count) of ops.voxel_compact"""
    want = V.compact_np(dense)
    idx, m = _ops().voxel_compact(_cuda(dense))
    assert m == len(want), "count %d against %d" % (m, len(want))
    assert idx.dtype == torch.int32 and tuple(idx.shape) == (len(want), 3)
    assert np.array_equal(idx.cpu().numpy(), want)
    return want


def _grid(dims, flat_cells=None, fill=0.0):
    dense = np.full(int(np.prod(dims)), fill, np.float32)
    if flat_cells is not None:
        dense[flat_cells] = 1.0
    return dense.reshape(dims)


@pytest.mark.parametrize("what", ["empty", "full", "last"])
def test_compact_grid_smaller_than_a_tile(what):
    dims = (3, 5, 7)
    dense = {"empty": _grid(dims), "full": _grid(dims, fill=1.0), "last": _grid(dims, [104])}[what]
    want = _compact_is(dense)
    assert len(want) == {"empty": 0, "full": 105, "last": 1}[what]
    if what == "last":
        assert want.tolist() == [[2, 4, 6]]


@pytest.mark.parametrize("what", ["ends", "full"])
def test_compact_short_tail_tile(what):
    g = V.GEOMETRIES["A"]
    n = V.ncell(g)
    assert n % V.TILE == 256
    want = _compact_is(_grid(g.dims, [0, n - 1]) if what == "ends" else _grid(g.dims, fill=1.0))
    if what == "ends":
        assert want.tolist() == [[0, 0, 0], [g.dims[0] - 1, g.dims[1] - 1, g.dims[2] - 1]]
    else:
        assert len(want) == n


CARRY_DIMS = (64, 75, 64)          # 300 tiles: dn_voxel_compact's scan takes 256 of them in its first pass, 44 in its second


def _carry_grid(what):
    n = int(np.prod(CARRY_DIMS))
    assert n == 300 * V.TILE
    if what == "one_in_tile_256":
        return _grid(CARRY_DIMS, [256 * V.TILE + 517])
    if what == "tiles_255_256_full":
        return _grid(CARRY_DIMS, np.arange(255 * V.TILE, 257 * V.TILE))
    if what == "last_tile_full":
        return _grid(CARRY_DIMS, np.arange(299 * V.TILE, n))
    return _grid(CARRY_DIMS, np.flatnonzero(np.random.default_rng(29).random(n) < 0.03))


@pytest.mark.parametrize("what", ["one_in_tile_256", "tiles_255_256_full", "last_tile_full", "three_percent"])
def test_compact_carry_across_scan_passes(what):
    want = _compact_is(_carry_grid(what))
    if what != "three_percent":
        assert len(want) == {"one_in_tile_256": 1, "tiles_255_256_full": 2 * V.TILE, "last_tile_full": V.TILE}[what]


def test_compact_occupied_means_not_equal_zero():
    values = np.array([1.0, 0.5, -1.0, 1e-45, np.nan, 0.0, -0.0], np.float32)
    assert values[3] != 0 and np.signbit(values[6])
    dense = np.resize(values, 105).reshape(3, 5, 7)                    # the pattern walks the z bins: bins 5 and 6 stay free
    want = _compact_is(dense)
    assert len(want) == 75 and set(want[:, 2].tolist()) == {0, 1, 2, 3, 4}


def _compact_raw(dense, capacity, pad=64, sentinel=-7):
    """the C entry point with an index buffer of capacity + pad rows pre-filled with a sentinel -> (buffer, count)"""
    from disconet_amd import _lib
    ops, lib = _ops(), _lib.load()
    d = (ctypes.c_int * 3)(*dense.shape)
    ws = torch.empty(max(1, lib.dn_voxel_compact_workspace(d)), dtype=torch.uint8, device="cuda")
    idx = torch.full((capacity + pad, 3), sentinel, dtype=torch.int32, device="cuda")
    cnt = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    _lib.check(lib.dn_voxel_compact(ops._ptr(dense), d, ops._ptr(idx), capacity, ops._ptr(cnt), ops._ptr(ws), ops._stream()),
               "dn_voxel_compact")
    return idx.cpu().numpy(), int(cnt.item())


def test_compact_short_capacity_reports_the_full_count_and_stays_inside():
    dense_np = _carry_grid("three_percent")
    want = V.compact_np(dense_np)
    m = len(want)
    assert 8000 < m < 10500
    dense = _cuda(dense_np)
    for capacity in (m, m - 1, 1, 0):
        kept = min(m, capacity)
        buf, count = _compact_raw(dense, capacity)
        assert count == m, capacity
        assert np.array_equal(buf[:kept], want[:kept]), capacity
        assert (buf[capacity:] == -7).all(), "capacity %d: a row past the capacity was written" % capacity
        idx, count = _ops().voxel_compact(dense, capacity=capacity)
        assert count == m and tuple(idx.shape) == (kept, 3), capacity
        assert np.array_equal(idx.cpu().numpy(), want[:kept]), capacity


# ---- e. the scatter forms at Z = 1, 13, 17, 32 ---------------------------------------------------------------------------
def _with_image(idx, off, rows):
    rows = np.asarray(rows, np.int32).reshape(-1, 3)
    return np.concatenate([idx, rows]), np.concatenate([off, [off[-1] + len(rows)]]).astype(np.int32)


@pytest.mark.parametrize("counts", [(0, 40, 9, 0, 0, 25, 0), (30,)], ids=["7_images", "1_image"])
@pytest.mark.parametrize("z", [1, 13, 17, 32])
def test_scatter_forms(z, counts):
    dims = (16, 16, z)
    idx, off = V.scatter_case(dims, counts, seed=100 + z)
    n = len(counts)
    if z == 32 and n > 1:      # one more image: bin 31 in every pixel, and all 32 bins in pixel (3, 5)
        px = np.stack(np.meshgrid(np.arange(16), np.arange(16), indexing="ij"), axis=-1).reshape(-1, 2)
        top = np.concatenate([px, np.full((256, 1), 31)], axis=1)
        column = np.stack([np.full(32, 3), np.full(32, 5), np.arange(32)], axis=1)
        idx, off = _with_image(idx, off, np.concatenate([top, column]))
        n += 1
    if z == 17 and n > 1:      # one more image: bin 16 alone, the one live channel of the second chunk
        idx, off = _with_image(idx, off, [[0, 0, 16], [7, 9, 16], [15, 15, 16]])
        n += 1
    want, got = _check_forms(idx, off, n, dims)
    for img, count in enumerate(counts):
        assert (want[img].sum() == 0) == (count == 0)
    if z == 32 and n > len(counts):
        words = got["bits"][n - 1]
        assert words.dtype == np.uint32 and (words >= 2 ** 31).all() and words[3, 5] == 0xFFFFFFFF
        assert (np.delete(words.reshape(-1), 3 * 16 + 5) == 2 ** 31).all()
    if z == 17 and n > len(counts):
        sp = got["sp"].reshape(n, 2, 4, 256, 8)[n - 1]
        hi = got["hi"].reshape(n, 2, 2, 256, 8)[n - 1]
        assert not sp[0].any() and not hi[0].any()                         # bins 0 .. 15: nothing
        assert not sp[1, 1:].any() and not hi[1, 1].any()                  # second chunk: octet 1 of hi, both of lo
        assert int((sp[1, 0, :, 0] == 0x3C00).sum()) == 3 and not sp[1, 0, :, 1:].any()
        assert np.array_equal(hi[1, 0], sp[1, 0])


# ---- f. rows that belong to no image ------------------------------------------------------------------------------------
@pytest.mark.parametrize("offsets", [(5, 9, 9, 20), (3, 10)], ids=["3_images", "1_image"])
def test_rows_outside_the_offsets_belong_to_no_image(offsets):
    dims = (16, 16, 13)
    rng = np.random.default_rng(31)
    px = rng.choice(256, size=30, replace=False)                       # 30 rows in 30 different pixels
    idx = np.stack([px // 16, px % 16, rng.integers(0, 13, 30)], axis=1).astype(np.int32)
    off = np.array(offsets, np.int32)
    n = len(offsets) - 1
    want, got = _check_forms(idx, off, n, dims)
    owned = np.zeros(30, bool)
    for img in range(n):
        rows = idx[off[img]:off[img + 1]]
        owned[off[img]:off[img + 1]] = True
        assert want[img].sum() == len(rows) and (want[img, rows[:, 0], rows[:, 1], rows[:, 2]] == 1).all()
    assert owned.sum() == offsets[-1] - offsets[0]
    stray = idx[~owned]
    assert len(stray) == 30 - owned.sum()
    assert not got["dense"][:, stray[:, 0], stray[:, 1], stray[:, 2]].any(), "a row outside the offsets was written"
    assert not got["bits"][:, stray[:, 0], stray[:, 1]].any()
