"""The split-planar f16 format as the kernels write it, byte for byte against the numpy statement of tests/sp_format.py:
activation tensors (dn_sp_from_nhwc / dn_sp_to_nhwc) and the plain packed weight images of both conv engines.  The
tap-merged, heads, post-1x1 and fragment images have no host statement here: the float64 conv tests hold their values."""
import numpy as np
import pytest
import torch

from tests import sp_format as F

pytestmark = pytest.mark.gpu

PLANTED = [0.0, -0.0, 1e-5, 2.0 ** -25, 65519.9, 70000.0, -70000.0]


def _bits(t):
    """a device tensor's bytes as uint16 [pieces, 8]"""
    return t.contiguous().view(torch.uint8).cpu().numpy().view(np.uint16).reshape(-1, 8)


def _same_pieces(got, want, what):
    assert got.shape == want.shape, "%s: %s pieces against %s" % (what, got.shape, want.shape)
    bad = np.argwhere((got != want).any(-1))[:, 0]
    assert len(bad) == 0, "%s: %d of %d pieces differ, first %s: %s against %s" % (
        what, len(bad), len(want), bad[:4].tolist(), ["%04x" % v for v in got[bad[0]]], ["%04x" % v for v in want[bad[0]]])


def _activations(c, ld):
    g = torch.Generator().manual_seed(100 + c)
    wide = torch.randn(2, 3, 5, ld, generator=g) * 3.0
    at = torch.randperm(2 * 3 * 5 * c, generator=g)[:len(PLANTED)]
    for i, v in zip(at.tolist(), PLANTED):
        wide[tuple(int(k) for k in np.unravel_index(i, (2, 3, 5, c)))] = v      # inside the first c channels
    return wide


@pytest.mark.parametrize("c,extra", [(8, 0), (24, 0), (32, 0), (24, 8)])
def test_activation_tensor_bytes(c, extra):
    from disconet_amd import ops
    ops.sp_range_flags(reset=True)
    try:
        wide = _activations(c, c + extra)
        x = wide[..., :c]                                  # extra > 0: a channel slice, pixel stride c + extra
        t = ops.SpTensor.from_nhwc(wide.cuda()[..., :c])
        want = F.act_image(x.numpy())
        _same_pieces(_bits(t.data), want, "SpTensor.from_nhwc, %d channels (ld %d)" % (c, c + extra))
        # padded octets: zero in all four quarters
        chunks, hw = F.chunks_of(c), 15
        data = _bits(t.data).reshape(2, chunks, 4, hw, 8)
        for oct8 in range((c + 7) // 8, 2 * chunks):
            assert not data[:, oct8 // 2, [oct8 % 2, 2 + oct8 % 2]].any(), "padded octet %d is not zero" % oct8
        # back: float(hi) + float(lo), exactly
        hi, lo = F.split_bits(x.numpy())
        assert np.array_equal(t.nhwc().cpu().numpy().view(np.uint32), F.value_of(hi, lo).view(np.uint32))
        # the planted 70000: bit 1 = a value above 2^14 was split, bit 0 = a value was clamped
        flags = ops.sp_range_flags(reset=True)
        assert flags & 3 == 3, "range flags %#x" % flags
    finally:
        ops.sp_range_flags(reset=True)


def _weight(c_out, c_in, k, seed):
    return torch.randn(c_out, c_in, k, k, generator=torch.Generator().manual_seed(seed)) * 0.05


@pytest.mark.parametrize("c_out,c0,c1,k", [(5, 20, 0, 3), (70, 16, 0, 1), (12, 16, 8, 3)])
def test_plain_sp_weight_image_bytes(c_out, c0, c1, k):
    from disconet_amd import ops
    w = _weight(c_out, c0 + c1, k, 7 * c_out + k)
    d = ops.conv_desc(1, 8, 8, c0, c_out, k, c1=c1, math="sp")
    wmul = 2.0 ** 9
    packed, got_wmul = ops.sp_pack_conv_weights(d, w.cuda(), wmul=wmul)
    assert got_wmul == wmul
    _same_pieces(_bits(packed), F.plain_weight_image(w.numpy(), wmul, c0=c0), "dn_spconv_pack_weights %s" % ((c_out, c0, c1, k),))


@pytest.mark.parametrize("math", ["f32", "f16x3"])
@pytest.mark.parametrize("c_out,c_in,k", [(5, 20, 3), (40, 9, 1)])
def test_nhwc_weight_image_bytes(c_out, c_in, k, math):
    from disconet_amd import ops
    w = _weight(c_out, c_in, k, 11 * c_out + k)
    d = ops.conv_desc(1, 8, 8, c_in, c_out, k, math=math)
    got = ops.pack_conv_weights(d, w.cuda()).view(torch.uint8).cpu().numpy()
    want = F.nhwc_weight_image(w.numpy(), split=math == "f16x3")
    assert got.shape == want.shape
    assert np.array_equal(got, want), "dn_conv_pack_weights (%s): %d bytes differ" % (math, int((got != want).sum()))
