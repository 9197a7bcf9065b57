"""The voxel front end's test cases and a numpy statement of every output of disconet_amd/csrc/voxel.hip.  numpy only:
no GPU import and nothing from the library, so that tests/test_gpu_voxel_edges.py compares the kernels with text written
apart from them.  tests/test_voxel_cases_cpu.py holds this file to oracle.voxel_ref and shows that each way of getting
the voxel rule wrong (MUTANTS) moves a cell on the sweeps below: without that the GPU tests could not see a wrong kernel.

The voxel rule (include/disconet_hip.h, K1): a float32 point is kept when lo < c < hi on every axis, compared in float64
against the float64 extents; its cell is floor(c / voxel) - floor(lo / voxel), the divide in float64.  The grid has
ceil(hi / voxel) - floor(lo / voxel) cells per axis."""
import collections

import numpy as np

from tests import sp_format

TILE = 1024                   # cells per workgroup of dn_voxel_compact: a grid that is no multiple of it has a short tail tile
SP_CHUNK = 16                 # channels per SP chunk: Z > 16 puts bins into a second chunk

Geometry = collections.namedtuple("Geometry", "name voxel extents dims why")


def _dims_of(voxel, extents):
    """the grid dims as the oracle derives them (its num_divisions): read off the grid it returns for an empty cloud"""
    from oracle.voxel_ref import voxelize_occupy
    return tuple(int(v) for v in voxelize_occupy(np.zeros((0, 3), np.float32), voxel, extents).shape)


def _geometry(name, voxel, ext, why):
    extents = np.array(ext, dtype=np.float64)
    return Geometry(name, tuple(float(v) for v in voxel), extents, _dims_of(voxel, extents), why)


GEOMETRIES = collections.OrderedDict((g.name, g) for g in (
    _geometry("default", (0.25, 0.25, 0.4), [[-32.0, 32.0], [-32.0, 32.0], [-3.0, 2.0]],
              "the shipped grid, 832 whole tiles"),
    _geometry("A", (0.4, 0.4, 0.4), [[-8.0, 8.0], [-6.4, 6.4], [-3.0, 2.0]],
              "16 tiles + 256 cells (short tail tile); voxel off the binary lattice on every axis"),
    _geometry("B", (0.1, 0.1, 0.2), [[-3.2, 3.3], [0.3, 4.1], [-3.0, 3.4]],
              "Z = 32: bit 31, two SP chunks; positive miny; y extents off the lattice"),
    _geometry("C", (0.25, 0.5, 0.125), [[-4.1, 4.05], [-8.0, 8.0], [-1.0, 1.125]],
              "Z = 17: second SP chunk with one live channel; x extents off the lattice"),
    _geometry("D", (0.25, 0.25, 0.4), [[2.0, 10.0], [-10.0, -2.0], [-3.0, 2.0]],
              "all-positive x, all-negative y"),
))


def ncell(g):
    return g.dims[0] * g.dims[1] * g.dims[2]


def min_cell(g, rounding=np.floor):
    """floor(lo / voxel) per axis, float64"""
    return rounding(g.extents[:, 0] / np.asarray(g.voxel, np.float64)).astype(np.int64)


def on_lattice(g, axis):
    """both extents of the axis are whole multiples of the voxel (as float64 quotients)"""
    q = g.extents[axis] / g.voxel[axis]
    return bool((q == np.round(q)).all())


def _binary(v):
    """v is a power of two: a divide by it is exact in float32 and in float64"""
    m, _ = np.frexp(v)
    return m == 0.5


def check_table():
    """the property each row is in the table for: a later edit of the table cannot silently drop the edge"""
    G = GEOMETRIES
    assert G["default"].dims == (256, 256, 13) and ncell(G["default"]) % TILE == 0
    a = G["A"]
    assert a.dims == (40, 32, 13) and ncell(a) == 16 * TILE + 256 and not any(_binary(v) for v in a.voxel)
    b = G["B"]
    assert b.dims[2] == 32 and b.dims[2] > SP_CHUNK and ncell(b) % TILE != 0
    assert min_cell(b)[1] > 0 and not on_lattice(b, 1)
    c = G["C"]
    assert c.dims == (34, 32, 17) and c.dims[2] == SP_CHUNK + 1 and not on_lattice(c, 0) and ncell(c) % TILE != 0
    assert all(_binary(v) for v in c.voxel)
    d = G["D"]
    assert d.dims == (32, 32, 13) and min_cell(d)[0] > 0 and d.extents[0, 0] > 0 and d.extents[1, 1] < 0
    assert all(g.dims[2] <= 32 for g in G.values())           # every geometry has a bit-word form
    for g in G.values():                                      # sweep()'s nine lines lie inside the grid
        held = g.extents.mean(axis=1)[None] + np.arange(-3, 6)[:, None] * np.asarray(g.voxel)
        assert ((g.extents[:, 0] < held) & (held < g.extents[:, 1])).all(), g.name


check_table()


# ---- points ------------------------------------------------------------------------------------------------------------
def _with_neighbours(values):
    """float32 values -> [k, 3]: each value, its float32 neighbour below and its float32 neighbour above"""
    v = np.asarray(values, np.float32)
    return np.stack([v, np.nextafter(v, np.float32(-np.inf)), np.nextafter(v, np.float32(np.inf))], axis=1)


def sweep(g):
    """[n, 4] float32.  Per axis: every lattice value k * voxel, k from one cell below the grid to two past it, rounded to
    float32, with its two float32 neighbours; then the axis' two extents (float32) with theirs.  The other two coordinates
    are held near the centre of the grid, on one of nine lines a whole number of cells off it: a value, its lower and its
    upper neighbour take lines of their own, even and odd k again, and so do the three of an extent.  On a single line
    the sweep would fill every cell of the line whatever the rule, and a point put one cell off would change nothing; on
    its own line a lattice point shares its cell with no other point, so the GRID moves when the point does."""
    voxel = np.asarray(g.voxel, np.float64)
    centre = g.extents.mean(axis=1)
    lo = min_cell(g)
    rows = []
    for axis in range(3):
        k = np.arange(lo[axis] - 1, lo[axis] + g.dims[axis] + 2)
        for variant, col in enumerate(_with_neighbours(k * voxel[axis]).T):
            line = variant + 3 * (k & 1) - 3                      # -3 .. 2
            p = centre + line[:, None] * voxel
            p[:, axis] = col
            rows.append(p)
        for col, line in zip(_with_neighbours(g.extents[axis]).T, (3, 4, 5)):
            p = np.tile(centre + line * voxel, (len(col), 1))
            p[:, axis] = col
            rows.append(p)
    xyz = np.concatenate(rows).astype(np.float32)
    return np.concatenate([xyz, np.zeros((len(xyz), 1), np.float32)], axis=1)


def cloud(g, n, seed):
    """[n, 4] float32: a seeded uniform cloud that reaches 10 % of each extent's width past it; column 3 an intensity"""
    rng = np.random.default_rng(seed)
    span = g.extents[:, 1] - g.extents[:, 0]
    xyz = rng.uniform(g.extents[:, 0] - 0.1 * span, g.extents[:, 1] + 0.1 * span, size=(n, 3))
    return np.concatenate([xyz, rng.uniform(0, 1, size=(n, 1))], axis=1).astype(np.float32)


# ---- the voxel rule, and ways to get it wrong ---------------------------------------------------------------------------
MUTANTS = ("f32_divide", "closed_extents", "trunc", "min_round")


def voxelize_np(pts, g, mutant=None):
    """pts [n, >= 3] float32 -> dense [X, Y, Z] float32 0/1 by the voxel rule.  mutant: one of MUTANTS breaks it --
    f32_divide: the divide in float32; closed_extents: <= for <; trunc: the quotient cut toward zero where the rule takes
    its floor; min_round: round(lo / voxel) for floor(lo / voxel).  A cell outside the grid is dropped (the kernels guard
    their store the same way), so a mutant grid has the rule's shape."""
    assert mutant is None or mutant in MUTANTS
    p32 = np.ascontiguousarray(np.asarray(pts)[:, :3], dtype=np.float32)
    p = p32.astype(np.float64)
    lo, hi = g.extents[:, 0], g.extents[:, 1]
    keep = ((lo <= p) & (p <= hi)).all(axis=1) if mutant == "closed_extents" else ((lo < p) & (p < hi)).all(axis=1)
    p32, p = p32[keep], p[keep]
    if mutant == "f32_divide":
        quot = (p32 / np.asarray(g.voxel, np.float32)).astype(np.float64)
    else:
        quot = p / np.asarray(g.voxel, np.float64)
    cell = (np.trunc(quot) if mutant == "trunc" else np.floor(quot)).astype(np.int64)
    cell -= min_cell(g, np.round if mutant == "min_round" else np.floor)
    inside = ((cell >= 0) & (cell < np.asarray(g.dims))).all(axis=1)
    cell = cell[inside]
    dense = np.zeros(g.dims, np.float32)
    dense[cell[:, 0], cell[:, 1], cell[:, 2]] = 1.0
    return dense


# ---- the other outputs ----------------------------------------------------------------------------------------------------
def compact_np(dense):
    """dn_voxel_compact: the cells with dense != 0 (NaN and subnormals count, 0.0 and -0.0 do not) as [m, 3] int32 rows;
    argwhere walks the grid in its linear order, which is the reference's lexsort(x, then y, then z) order"""
    return np.argwhere(np.asarray(dense) != 0).astype(np.int32)


def scatter_np(indices, offsets, n_images, dims):
    """the dense rebuild -> [n_images, X, Y, Z] float32: image g owns rows offsets[g] .. offsets[g + 1] - 1 of `indices`;
    a row before offsets[0] or from offsets[n_images] on belongs to no image; a row outside the grid is dropped"""
    indices = np.asarray(indices, np.int64).reshape(-1, 3)
    offsets = np.asarray(offsets, np.int64)
    assert len(offsets) == n_images + 1
    dense = np.zeros((n_images,) + tuple(dims), np.float32)
    for img in range(n_images):
        rows = indices[max(offsets[img], 0):max(min(offsets[img + 1], len(indices)), 0)]
        rows = rows[((rows >= 0) & (rows < np.asarray(dims))).all(axis=1)]
        dense[img, rows[:, 0], rows[:, 1], rows[:, 2]] = 1.0
    return dense


def bits_np(dense):
    """[..., Z <= 32] 0/1 -> uint32 [...]: bit z = bin z is occupied; summed in uint64, then cast"""
    dense = np.asarray(dense)
    z = dense.shape[-1]
    assert z <= 32
    words = ((dense != 0).astype(np.uint64) << np.arange(z, dtype=np.uint64)).sum(axis=-1, dtype=np.uint64)
    return words.astype(np.uint32)


def sp_np(dense, hi_only=False):
    """[n, X, Y, Z] -> uint16 [pieces, 8]: the bytes of the SP tensor [n][chunk][4 quarters][X * Y] (tests/sp_format);
    hi_only: quarters 0 and 1 of every chunk, [n][chunk][2][X * Y]"""
    n, x, y, z = dense.shape
    image = sp_format.act_image(dense)
    if not hi_only:
        return image
    return np.ascontiguousarray(image.reshape(n, sp_format.chunks_of(z), 4, x * y, 8)[:, :, :2]).reshape(-1, 8)


# ---- row lists for the scatter forms ----------------------------------------------------------------------------------------
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


def outside_rows(dims):
    """rows that lie outside a grid of `dims`, each by one coordinate only (the other two are valid cells)"""
    x, y, z = dims
    return np.array([[-1, 0, 0], [0, -1, 0], [0, 0, -1], [x, 0, 0], [0, y, 0], [0, 0, z], [x - 1, y - 1, z],
                     [INT32_MIN, 1, 0], [1, INT32_MIN, 0], [1, 1, INT32_MIN], [INT32_MAX, 1, 0], [1, INT32_MAX, 0],
                     [1, 1, INT32_MAX], [INT32_MIN, INT32_MIN, INT32_MIN], [INT32_MAX, INT32_MAX, INT32_MAX]], np.int64)


def scatter_case(dims, counts, seed):
    """-> (indices [m, 3] int32, offsets [len(counts) + 1] int32).  Image g gets counts[g] seeded cells, a quarter of them
    a second time, and every row of outside_rows(dims), all shuffled; counts[g] == 0 leaves the image's list empty."""
    rng = np.random.default_rng(seed)
    lists = []
    for count in counts:
        if count == 0:
            lists.append(np.zeros((0, 3), np.int64))
            continue
        cells = np.stack([rng.integers(0, d, size=count) for d in dims], axis=1)
        rows = np.concatenate([cells, cells[:max(1, count // 4)], outside_rows(dims)])
        lists.append(rows[rng.permutation(len(rows))])
    offsets = np.concatenate([[0], np.cumsum([len(rows) for rows in lists])]).astype(np.int32)
    return np.concatenate(lists).astype(np.int32), offsets
