"""The element-wise and gather kernels of the training step -- dn_upsample2_sum, dn_add_rows, dn_pair_add_ego,
dn_pair_sum_ego, dn_channel_sum, dn_fuse_combine / _backward -- against float64 on the CPU, at the tolerances of their
unit tests in tests/test_gpu_train_ops.py (1e-6 / 1e-5 / 2e-5 of the largest reference entry), at sizes above the
2 097 152 elements of their capped grids and on the paths those tests leave out."""
import pytest
import torch

from tests import train_small_ops as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# the shape of the tensor each kernel's grid-stride loop runs over, above 8192 * 256 elements
BIG = {
    "upsample2_sum": (3, 128, 128, 64),          # the OUTPUT [n, h, w, c]
    "add_rows": (3, 128, 128, 48),
    "pair_add_ego": (9, 64, 64, 64),             # z1 [pairs, h, w, c]
    "pair_sum_ego": (9, 64, 64, 64),             # de [images, h, w, c]
}


def rel_err(got, ref):
    ref = ref.double()
    return float((got.double().cpu() - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


def _block_sums(g):
    n, h2, w2, c = g.shape
    return g.double().view(n, h2 // 2, 2, w2 // 2, 2, c).sum((2, 4))


@pytest.mark.parametrize("c", [3, 64])
@pytest.mark.parametrize("sliced", [False, True])
def test_upsample2_sum_direct(c, sliced):
    """the backward of the nearest x2 upsample on its own (only a whole training step reached it): 2 x 2 block sums of a dense
    gradient and of a channel slice of a wider one, odd map sizes, 3 channels (no float4) and 64"""
    from disconet_amd import train_ops
    g = torch.Generator().manual_seed(c)
    for n, h, w in ((1, 1, 1), (2, 5, 7), (3, 16, 9)):
        wide = torch.randn(n, 2 * h, 2 * w, c + 5, generator=g)
        src = wide[..., 2:2 + c] if sliced else wide[..., 2:2 + c].contiguous()
        dev = wide.to(DEV)[..., 2:2 + c] if sliced else src.to(DEV)
        assert dev.is_contiguous() != sliced
        out = train_ops.upsample2_sum(dev)
        assert tuple(out.shape) == (n, h, w, c) and out.is_contiguous()
        assert rel_err(out, _block_sums(src)) < 1e-6, (n, h, w)


def test_upsample2_sum_above_the_grid_cap():
    from disconet_amd import train_ops
    n, h, w, c = BIG["upsample2_sum"]
    g = torch.randn(n, 2 * h, 2 * w, c, generator=torch.Generator(device=DEV).manual_seed(1), device=DEV)
    out = train_ops.upsample2_sum(g)
    assert out.numel() > T.ELEMENTWISE_CAP
    assert rel_err(out, _block_sums(g.cpu())) < 1e-6


def test_add_rows_above_the_grid_cap():
    from disconet_amd import train_ops
    n, h, w, c = BIG["add_rows"]
    gen = torch.Generator().manual_seed(2)
    a = torch.randn(n, h, w, c, generator=gen)
    wide = torch.randn(n, h, w, c + 16, generator=gen)
    assert a.numel() > T.ELEMENTWISE_CAP
    ag, wg = a.to(DEV), wide.to(DEV)
    train_ops.add_rows(ag, wg[..., 4:4 + c])
    assert rel_err(ag, a.double() + wide[..., 4:4 + c].double()) < 1e-6
    # ... into a slice of a wider tensor: nothing outside it moves
    dst = wide.to(DEV)
    train_ops.add_rows(dst[..., 4:4 + c], a.to(DEV))
    assert rel_err(dst[..., 4:4 + c], a.double() + wide[..., 4:4 + c].double()) < 1e-6
    assert torch.equal(dst[..., :4].cpu(), wide[..., :4]) and torch.equal(dst[..., 4 + c:].cpu(), wide[..., 4 + c:])


def test_pair_kernels_above_the_grid_cap_with_repeated_unused_and_empty_entries():
    """z1[p] += e[ego[p]] with ego indices that repeat and images nobody uses; de[img] = sum of dz1 over the image's pairs with
    an image whose pair list is empty (first[i] == first[i + 1]): zeros are WRITTEN there (the output starts as NaN)"""
    from disconet_amd import train_ops
    gen = torch.Generator().manual_seed(3)
    p, h, w, c = BIG["pair_add_ego"]
    z1 = torch.randn(p, h, w, c, generator=gen)
    e = torch.randn(6, h, w, c, generator=gen)
    ego = torch.tensor([4, 0, 0, 4, 4, 2, 0, 5, 4], dtype=torch.int32)           # images 1 and 3 unused
    assert z1.numel() > T.ELEMENTWISE_CAP
    got = train_ops.pair_add_ego(z1.to(DEV), e.to(DEV), ego.to(DEV))
    assert rel_err(got, z1.double() + e.double()[ego.long()]) < 1e-6
    n_img = BIG["pair_sum_ego"][0]
    first = torch.tensor([0, 2, 2, 3, 3, 3, 7, 8, 8, 9], dtype=torch.int32)      # images 1, 3, 4, 7: no pair
    pairs = torch.tensor([8, 0, 3, 1, 2, 4, 5, 7, 6], dtype=torch.int32)
    assert first.numel() == n_img + 1 and n_img * h * w * c > T.ELEMENTWISE_CAP
    de = train_ops.pair_sum_ego(z1.to(DEV), first.to(DEV), pairs.to(DEV), n_img)
    ref = torch.stack([z1.double()[pairs[first[i]:first[i + 1]].long()].sum(0) for i in range(n_img)])
    assert rel_err(de, ref) < 1e-6
    for i in (1, 3, 4, 7):
        assert float(de[i].abs().max()) == 0.0
    # the wrapper's output is torch.empty: hand the allocator a block of NaN first, so that a skipped write shows
    del de
    torch.full((n_img, h, w, c), float("nan"), device=DEV)
    de = train_ops.pair_sum_ego(z1.to(DEV), first.to(DEV), pairs.to(DEV), n_img)
    assert bool(torch.isfinite(de).all()) and float(de[4].abs().max()) == 0.0


@pytest.mark.parametrize("c", [1, 6, 37, 36])
@pytest.mark.parametrize("rows", [1, 3, 300000])
def test_channel_sum_scalar_path(c, rows):
    """the per-element kernel: channel counts that are no multiple of 4 (1, 6, 37), and c = 36 from a view whose pointer is
    not 16-byte aligned; 1, 3 and 300 000 rows (dn_reduce_workspace_bytes: more than one partial block); accumulate on / off"""
    from disconet_amd import _lib, train_ops
    gen = torch.Generator().manual_seed(rows % 97 + c)
    wide = torch.randn(rows, c + 8, generator=gen) + 0.25
    wg = wide.to(DEV)
    view = wg[:, 1:1 + c]                                                  # 4 bytes past a 16-byte boundary; c = 36: row stride 44, a multiple of 4
    assert view.data_ptr() % 16 == 4 and (c % 4 != 0 or view.stride(0) % 4 == 0)
    ref = wide[:, 1:1 + c].double().sum(0)
    scale = float(wide[:, 1:1 + c].double().abs().sum(0).max())
    out = torch.full((c,), 7.0, device=DEV)
    train_ops.channel_sum(view, out)
    # the partials are float64; what is left is the rounding of the result and of the fold: 1e-6 of the largest |sum| as
    # in the unit test, and never more than 1e-6 of the sum of magnitudes
    assert rel_err(out, ref) < 1e-6
    assert float((out.double().cpu() - ref).abs().max()) <= 1e-6 * scale
    train_ops.channel_sum(view, out, accumulate=True)
    assert rel_err(out, 2 * ref) < 1e-6
    blocks = _lib.load().dn_reduce_workspace_bytes(1, rows, c) // (16 * c) - 1      # [2 c] doubles per block, one for the fold
    assert (blocks > 1) == (rows == 300000), blocks


@pytest.mark.parametrize("c", [64, 512])
def test_fuse_combine_partial_lanes_short_and_long_lists(c):
    """c = 64 (16 of 64 lanes busy) and 512 (two passes of the lane loop); 5 x 7 pixels x 3 egos = 105 items, the last
    workgroup of four holds one; lists of 1, 2 and 6 entries; z4 negative (dz4 exactly 0), exactly 0, and 80 (a weight of
    1 within rounding); a map in no list keeps the caller's dmaps rows; dfused as a channel slice.  Float64 autograd, the unit
    test's 1e-5 (fused, dmaps) and 2e-5 (dz4)."""
    from disconet_amd import train_ops
    z4, maps, dfused = T.fuse_case(c)
    lists, ego_out = T.FUSE_LISTS, T.FUSE_EGO_OUT
    outs, wts, dmaps_ref, dz4_ref = T.fuse_combine_ref(z4, maps, lists, ego_out, dfused)
    first = torch.tensor([0] + [sum(len(l) for l in lists[:k + 1]) for k in range(len(lists))], dtype=torch.int32).to(DEV)
    pair_index = torch.tensor([p for l in lists for p, _ in l], dtype=torch.int32).to(DEV)
    map_image = torch.tensor([m for l in lists for _, m in l], dtype=torch.int32).to(DEV)
    eo = torch.tensor(ego_out, dtype=torch.int32).to(DEV)
    mg, zg = maps.to(DEV), z4.to(DEV)
    h, w = T.FUSE_HW
    fused = torch.full((4, h, w, c), -9.0, device=DEV)
    wk = train_ops.fuse_combine(zg, mg, first, pair_index, map_image, eo, fused)
    for o, e_ in zip(outs, ego_out):
        assert rel_err(fused[e_], o) < 1e-5
    assert float((fused[1] + 9.0).abs().max()) == 0.0                      # the image no ego writes to
    for lst, wr in zip(lists, wts):
        for k, (p, _) in enumerate(lst):
            if p >= 0:      # weights in [0, 1]: exp to 2 ulp, a sum of <= 6 terms, a quotient -- under 10 u = 6e-7
                assert float((wk[p, ..., 0].cpu().double() - wr[k]).abs().max()) < 1e-6
    wide = torch.zeros(4, h, w, c + 64)
    wide[..., 64:] = dfused
    dmaps = torch.full_like(mg, 7.0)
    dz4 = train_ops.fuse_combine_backward(wide.to(DEV)[..., 64:], zg, wk, mg, first, pair_index, map_image, eo, dmaps)
    used = sorted(m for l in lists for _, m in l)
    assert rel_err(dmaps[used], dmaps_ref[used]) < 1e-5
    assert float((dmaps[9] - 7.0).abs().max()) == 0.0                      # map 9 is in no list: left as the caller had it
    assert rel_err(dz4, dz4_ref) < 2e-5
    assert float(dz4.cpu()[z4 <= 0].abs().max()) == 0.0
