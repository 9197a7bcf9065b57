"""tests/voxel_cases.py against the oracle, and its mutants against itself (no GPU).  The GPU tests of the voxel front end
(tests/test_gpu_voxel_edges.py) compare the kernels with oracle.voxel_ref on voxel_cases' sweeps and clouds: this file
shows that the numpy statement IS the oracle's rule, bit for bit, and that a kernel which got the rule wrong in one of
four ways would move a cell on those sweeps."""
import numpy as np
import pytest

from tests import voxel_cases as V

NAMES = list(V.GEOMETRIES)


@pytest.mark.parametrize("name", NAMES)
def test_voxelize_np_is_the_oracle(name):
    from oracle.voxel_ref import voxelize_occupy
    g = V.GEOMETRIES[name]
    for pts in (V.sweep(g), V.cloud(g, 20000, seed=5)):
        want, idx = voxelize_occupy(pts, g.voxel, g.extents, return_indices=True)
        assert want.shape == g.dims
        assert np.array_equal(V.voxelize_np(pts, g), want)
        assert np.array_equal(V.compact_np(want), idx.astype(np.int32))
        assert 0 < want.sum() < want.size


@pytest.mark.parametrize("name", NAMES)
def test_sweep_form(name):
    """lattice values from one cell below the grid to two past it, the extents, float32 neighbours on both sides"""
    g = V.GEOMETRIES[name]
    s = V.sweep(g)
    assert s.dtype == np.float32 and s.shape == (3 * (sum(g.dims) + 9 + 6), 4)
    lo = V.min_cell(g)
    for axis in range(3):
        col = s[:, axis]
        for k in (lo[axis] - 1, lo[axis], lo[axis] + g.dims[axis], lo[axis] + g.dims[axis] + 1):
            v = np.float32(k * g.voxel[axis])
            for want in (v, np.nextafter(v, np.float32(-np.inf)), np.nextafter(v, np.float32(np.inf))):
                assert (col == want).any(), (axis, k)
        for e in g.extents[axis]:
            assert (col == np.float32(e)).any()
    c = V.cloud(g, 4000, seed=1)[:, :3].astype(np.float64)
    assert (c < g.extents[:, 0]).any(axis=0).all() and (c > g.extents[:, 1]).any(axis=0).all()


# Which geometries' sweeps see each mutant (the grid differs from the faithful one), and why the others cannot.
BITES = {
    "f32_divide": {"default": True, "A": True, "B": True, "D": True,
                   "C": False},     # C's voxel sizes are powers of two: the float32 quotient is the float64 one
    "closed_extents": {"default": True, "A": True, "B": True, "C": True, "D": True},
    "trunc": {"default": True, "A": True, "B": True, "C": True, "D": True},
    "min_round": {"B": True, "C": True,
                  # lo / voxel is whole on x and y and -7.5 on z, which rounds half to even, to floor's -8
                  "default": False, "A": False, "D": False},
}


def test_mutants_bite_where_recorded():
    got = {m: {} for m in V.MUTANTS}
    for name, g in V.GEOMETRIES.items():
        s = V.sweep(g)
        faithful = V.voxelize_np(s, g)
        for m in V.MUTANTS:
            got[m][name] = not np.array_equal(V.voxelize_np(s, g, m), faithful)
    assert got == BITES
    for m in V.MUTANTS:
        assert sum(BITES[m].values()) >= 2, m
    assert all(BITES["f32_divide"][k] for k in ("A", "B", "D"))


def test_only_boundaries_see_the_float32_divide():
    """a uniform cloud does not: this is why the GPU tests run sweeps"""
    for g in V.GEOMETRIES.values():
        c = V.cloud(g, 20000, seed=5)
        assert np.array_equal(V.voxelize_np(c, g, "f32_divide"), V.voxelize_np(c, g))


def test_scatter_and_bit_statements():
    dims = (4, 3, 32)
    idx = np.array([[0, 0, 0], [1, 2, 31], [1, 2, 31], [3, 2, 5], [4, 0, 0], [0, 0, -1], [2, 1, 7], [2, 2, 2]], np.int32)
    dense = V.scatter_np(idx, [1, 4, 4, 7], 3, dims)             # rows 0 and 7 belong to no image, rows 4 and 5 to no cell
    assert dense.shape == (3, 4, 3, 32) and dense.sum() == 3
    assert dense[0, 1, 2, 31] == 1 and dense[0, 3, 2, 5] == 1 and dense[2, 2, 1, 7] == 1 and dense[1].sum() == 0
    words = V.bits_np(dense)
    assert words.dtype == np.uint32 and words[0, 1, 2] == 2 ** 31 and words[0, 3, 2] == 32 and words[2, 2, 1] == 128
    assert V.bits_np(np.ones((1, 1, 32), np.float32))[0, 0] == 2 ** 32 - 1
    full, hi = V.sp_np(dense), V.sp_np(dense, hi_only=True)
    assert full.shape == (3 * 2 * 4 * 12, 8) and hi.shape == (3 * 2 * 2 * 12, 8)
    assert int((full == 0x3C00).sum()) == 3 and int((hi == 0x3C00).sum()) == 3 and set(np.unique(full)) == {0, 0x3C00}
    values = np.array([1.0, 0.5, -1.0, 1e-45, np.nan, 0.0, -0.0], np.float32).reshape(1, 1, 7)
    assert V.compact_np(values)[:, 2].tolist() == [0, 1, 2, 3, 4]


def test_scatter_case_form():
    dims = (16, 16, 17)
    idx, off = V.scatter_case(dims, (0, 40, 9, 0, 0, 25, 0), seed=3)
    assert idx.dtype == np.int32 and off.dtype == np.int32 and off[0] == 0 and off[-1] == len(idx)
    assert (np.diff(off) == 0).tolist() == [True, False, False, True, True, False, True]
    out = len(V.outside_rows(dims))
    assert np.diff(off)[1] == 40 + 10 + out
    inside = ((idx >= 0) & (idx < np.array(dims))).all(axis=1)
    assert int((~inside).sum()) == 3 * out
    assert idx.min() == V.INT32_MIN and idx.max() == V.INT32_MAX
