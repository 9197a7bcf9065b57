"""The voxel front end's host side without a GPU: what dn_voxelize_occupy, dn_voxelize_views, dn_voxel_compact and the four
dn_scatter_dense forms refuse is refused before anything is launched, with a dn_last_error message that names the argument.
Device pointers are fake and never dereferenced, as in tests/test_detect_host_cpu.py."""
import ctypes

import pytest

FAKE = ctypes.c_void_p(0x1000)
VOXEL, EXTENTS, DIMS = (0.25, 0.25, 0.4), (-8.0, 8.0, -8.0, 8.0, -3.0, 2.0), (64, 64, 13)
SCATTER_FORMS = ["dn_scatter_dense", "dn_scatter_dense_sp", "dn_scatter_dense_sp_hi", "dn_scatter_dense_bits"]


def _lib():
    from disconet_amd import _lib
    return _lib.load()


def _doubles(v):
    return None if v is None else (ctypes.c_double * len(v))(*v)


def _ints(v):
    return None if v is None else (ctypes.c_int * len(v))(*v)


def _voxelize(entry, voxel=VOXEL, extents=EXTENTS, dims=DIMS, pt_stride=4, bits=False):
    lib = _lib()
    if entry == "dn_voxelize_occupy":
        rc = lib.dn_voxelize_occupy(FAKE, 16, pt_stride, _doubles(voxel), _doubles(extents), _ints(dims), FAKE, None)
    else:
        rc = lib.dn_voxelize_views(FAKE, 16, pt_stride, FAKE, FAKE, FAKE, FAKE, FAKE, 1, 1, 16, 1, _doubles(voxel),
                                   _doubles(extents), _ints(dims), FAKE, FAKE if bits else None, None)
    return rc, lib.dn_last_error().decode()


def _scatter(entry, n_images=2, total=8, dims=(16, 16, 13), null=None):
    lib = _lib()
    ptr = {k: (None if k == null else FAKE) for k in ("indices", "offsets", "out")}
    rc = getattr(lib, entry)(ptr["indices"], ptr["offsets"], n_images, total, _ints(dims), ptr["out"], None)
    return rc, lib.dn_last_error().decode()


VOXELIZERS = ["dn_voxelize_occupy", "dn_voxelize_views"]


@pytest.mark.parametrize("entry", VOXELIZERS)
@pytest.mark.parametrize("dims", [(64, 64, 12), (65, 64, 13), (64, 63, 13), (0, 0, 0)])
def test_dims_that_do_not_match_extents_and_voxel_are_refused(entry, dims):
    rc, msg = _voxelize(entry, dims=dims)
    assert rc != 0 and "dims" in msg and "(64,64,13)" in msg


@pytest.mark.parametrize("entry", VOXELIZERS)
@pytest.mark.parametrize("voxel", [(0.0, 0.25, 0.4), (0.25, -0.25, 0.4), (0.25, 0.25, 0.0), (0.25, 0.25, float("nan"))])
def test_voxel_size_that_is_not_positive_is_refused(entry, voxel):
    rc, msg = _voxelize(entry, voxel=voxel)
    assert rc != 0 and "voxel_size" in msg


@pytest.mark.parametrize("entry", VOXELIZERS)
@pytest.mark.parametrize("pt_stride", [2, 0, -4])
def test_point_stride_below_three_is_refused(entry, pt_stride):
    rc, msg = _voxelize(entry, pt_stride=pt_stride)
    assert rc != 0 and "pt_stride" in msg


@pytest.mark.parametrize("entry", VOXELIZERS)
@pytest.mark.parametrize("which", ["voxel", "extents", "dims"])
def test_null_host_arrays_are_refused_by_name(entry, which):
    rc, msg = _voxelize(entry, **{which: None})
    assert rc != 0 and "null" in msg and {"voxel": "voxel_size", "extents": "extents", "dims": "dims"}[which] in msg


def test_views_refuse_33_height_bins_for_the_word_form():
    ext = EXTENTS[:4] + (-3.0, 9.9)
    rc, msg = _voxelize("dn_voxelize_views", extents=ext, dims=(64, 64, 33), bits=True)
    assert rc != 0 and "33 height bins" in msg and "dims" in msg


def test_compact_workspace_is_one_int_per_tile_of_1024_cells():
    assert _lib().dn_voxel_compact_workspace(_ints((40, 32, 13))) == 17 * 4          # 16 whole tiles and a short one
    assert _lib().dn_voxel_compact_workspace(_ints((3, 5, 7))) == 4
    assert _lib().dn_voxel_compact_workspace(None) == 0


def test_compact_refuses_null_dims_and_an_empty_grid():
    lib = _lib()
    rc = lib.dn_voxel_compact(FAKE, None, FAKE, 8, FAKE, FAKE, None)
    assert rc != 0 and "null dims" in lib.dn_last_error().decode()
    rc = lib.dn_voxel_compact(FAKE, _ints((16, 0, 13)), FAKE, 8, FAKE, FAKE, None)
    assert rc != 0 and "dims" in lib.dn_last_error().decode()
    rc = lib.dn_voxel_compact(FAKE, _ints((16, 16, 13)), FAKE, -1, FAKE, FAKE, None)
    assert rc != 0 and "capacity" in lib.dn_last_error().decode()
    rc = lib.dn_voxel_compact(FAKE, _ints((16, 16, 13)), None, 8, FAKE, FAKE, None)
    assert rc != 0 and "indices" in lib.dn_last_error().decode()


@pytest.mark.parametrize("entry", SCATTER_FORMS)
@pytest.mark.parametrize("n_images", [0, -1])
def test_scatter_refuses_no_images(entry, n_images):
    rc, msg = _scatter(entry, n_images=n_images)
    assert rc != 0 and "n_images" in msg


@pytest.mark.parametrize("entry", SCATTER_FORMS)
def test_scatter_refuses_null_dims_and_null_pointers_by_name(entry):
    rc, msg = _scatter(entry, dims=None)
    assert rc != 0 and "null dims" in msg
    for which in ("indices", "offsets"):
        rc, msg = _scatter(entry, null=which)
        assert rc != 0 and "null" in msg and which in msg
    rc, msg = _scatter(entry, null="out")
    assert rc != 0 and "null" in msg
    rc, msg = _scatter(entry, total=-1)
    assert rc != 0 and "n_indices_total" in msg
    rc, msg = _scatter(entry, dims=(16, 0, 13))
    assert rc != 0 and "dims" in msg


@pytest.mark.parametrize("z", [33, 64])
def test_word_form_refuses_more_than_32_height_bins(z):
    rc, msg = _scatter("dn_scatter_dense_bits", dims=(16, 16, z))
    assert rc != 0 and "dims[2]" in msg and "%d height bins" % z in msg
