"""The UNet's resampling kernels -- dn_maxpool2_nhwc / _backward, dn_upsample2_bilinear_nhwc / _backward and the SP forms
dn_sp_maxpool2 / dn_sp_upsample2_bilinear -- over a sweep of map sizes against float64, on maps of NaN, +-inf and signed
zeros against ATen bit for bit, and above the 4 194 304 items of their capped grid, where the whole-batch launch must equal
the image-by-image launches bit for bit.  References: tests/train_small_ops.py."""
import pytest
import torch

from tests import train_small_ops as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("c", [4, 40])
def test_bilinear_upsample_size_sweep(c):
    """every (h, w) of {1, 2, 3, 5, 8, 31, 64} x {1, 2, 7, 33}: forward 1e-6 absolute on O(1) data, backward 2e-6 of the
    gradient's maximum (the gather over five candidate rows / columns must cover every non-zero tap), the SP form 1e-5;
    the gradient passed as a channel slice of a wider tensor; with dy = 1 every channel of dx sums to the number of output
    pixels (the taps' weights of one output pixel sum to 1 within 2 u each way: 1e-5 of the count is generous)"""
    from disconet_amd import ops, train_ops
    g = torch.Generator().manual_seed(40 + c)
    for h, w in T.UPSAMPLE_SIZES:
        x = torch.randn(2, h, w, c, generator=g)
        wide = torch.randn(2, 2 * h, 2 * w, c + 12, generator=g)
        dy = wide[..., 8:8 + c]
        y_ref, dx_ref = T.upsample_ref(x, dy)
        y = train_ops.upsample2_bilinear(x.to(DEV))
        assert tuple(y.shape) == (2, 2 * h, 2 * w, c)
        assert float((y.cpu().double() - y_ref).abs().max()) <= 1e-6, (h, w)
        dx = train_ops.upsample2_bilinear_backward(wide.to(DEV)[..., 8:8 + c])
        assert tuple(dx.shape) == (2, h, w, c)
        assert float((dx.cpu().double() - dx_ref).abs().max()) <= 2e-6 * float(dx_ref.abs().max()), (h, w)
        ones = train_ops.upsample2_bilinear_backward(torch.ones(2, 2 * h, 2 * w, c, device=DEV))
        assert float((ones.cpu().double().sum((1, 2)) - 4 * h * w).abs().max()) <= 1e-5 * 4 * h * w, (h, w)
        sp = ops.SpTensor.from_nhwc(x.to(DEV))
        up = ops.sp_upsample2_bilinear(sp)
        want = T.upsample_ref(sp.nhwc().cpu())
        assert tuple(up.shape) == (2, 2 * h, 2 * w, c)
        assert float((up.nhwc().cpu().double() - want).abs().max()) <= 1e-5, (h, w)


def test_maxpool_special_values_bit_for_bit():
    """NaN, +inf, -inf at every window position, several NaNs, +0 / -0 ties, all-equal windows: values and the routing of the
    gradient as ATen on the CPU, compared as bit patterns (torch.equal is false on NaN, true on -0 == +0); the kernel's rule is
    `val > max || isnan(val)` in scan order."""
    from disconet_amd import train_ops
    x = T.pool_special_map(8)
    n, h, w, c = x.shape
    wide = torch.randn(n, h // 2, w // 2, c + 8, generator=torch.Generator().manual_seed(2))
    dy = wide[..., 4:4 + c]
    y_ref, dx_ref = T.maxpool_aten(x, dy)
    y = train_ops.maxpool2(x.to(DEV))
    assert torch.equal(T.bits(y.cpu()), T.bits(y_ref))
    dx = train_ops.maxpool2_backward(x.to(DEV), wide.to(DEV)[..., 4:4 + c])
    assert torch.equal(T.bits(dx.cpu()), T.bits(dx_ref))
    assert int(torch.isnan(y_ref).sum()) > 50 and int((y_ref == float("-inf")).sum()) >= 8


def test_sp_maxpool_special_values():
    """the SP form on the same map: an SP tensor holds what dn_sp_from_nhwc makes of the values (clamped to +-65504, no
    NaN), so the reference is ATen on the decoded tensor; signed-zero ties and all-equal windows stay what they are.  The
    (hi, lo) pair of the maximum is copied, so the decoded values are equal bit for bit."""
    from disconet_amd import ops
    x = T.pool_special_map(40)
    x = torch.where(torch.isnan(x), torch.full_like(x, 70000.0), x)       # (a NaN has no SP form; above the clamp instead)
    sp = ops.SpTensor.from_nhwc(x.to(DEV))
    ops.sp_range_flags(reset=True)                                        # (the clamp of +-inf / 70000 is flagged: expected)
    dec = sp.nhwc().cpu()
    assert float(dec.max()) == 65504.0 and float(dec.min()) == -65504.0 and bool((dec == 0).any())
    got = ops.sp_maxpool2(sp).nhwc().cpu()
    assert torch.equal(T.bits(got), T.bits(T.maxpool_aten(dec)))


# (n, h, w, c) of the INPUT map: more than 4 194 304 items for the batch, fewer for one image
# (tests/test_train_small_ops_cpu.py checks both against the launch code's item counts)
BIG = {
    "maxpool2": (5, 512, 512, 64),
    "maxpool2_backward": (5, 512, 512, 64),
    "upsample2_bilinear": (5, 128, 128, 64),
    "upsample2_bilinear_backward": (5, 256, 256, 64),
    "sp_maxpool2": (10, 512, 512, 64),
    "sp_upsample2_bilinear": (10, 128, 128, 64),
}


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_maxpool_above_the_grid_cap():
    """5 images of 512 x 512 x 64 (256 x 256 x 16 float4 outputs each: 5 242 880 items; a 256 x 256 input would stay under the
    cap): the batch launch = the five single-image launches bit for bit, forward and backward; image 3 against ATen."""
    from disconet_amd import train_ops
    n, h, w, c = BIG["maxpool2"]
    g = torch.Generator(device=DEV).manual_seed(1)
    x = torch.randn(n, h, w, c, generator=g, device=DEV).clamp_(min=-0.5)          # ties at the clamp value
    dy = torch.randn(n, h // 2, w // 2, c, generator=g, device=DEV)
    y = train_ops.maxpool2(x)
    dx = train_ops.maxpool2_backward(x, dy)
    for i in range(n):
        assert _same_bits(y[i:i + 1], train_ops.maxpool2(x[i:i + 1])), i
        assert _same_bits(dx[i:i + 1], train_ops.maxpool2_backward(x[i:i + 1], dy[i:i + 1])), i
    y_ref, dx_ref = T.maxpool_aten(x[3:4].cpu(), dy[3:4].cpu())
    assert torch.equal(T.bits(y[3:4].cpu()), T.bits(y_ref)) and torch.equal(T.bits(dx[3:4].cpu()), T.bits(dx_ref))


def test_bilinear_upsample_above_the_grid_cap():
    """forward: 5 images of 128 x 128 x 64 (5 242 880 output float4s); backward gather: 5 images of 256 x 256 x 64 (5 242 880
    input float4s): batch launch = single-image launches bit for bit; image 4 against float64 at the sweep's bounds."""
    from disconet_amd import train_ops
    g = torch.Generator(device=DEV).manual_seed(2)
    n, h, w, c = BIG["upsample2_bilinear"]
    x = torch.randn(n, h, w, c, generator=g, device=DEV)
    y = train_ops.upsample2_bilinear(x)
    for i in range(n):
        assert _same_bits(y[i:i + 1], train_ops.upsample2_bilinear(x[i:i + 1])), i
    assert float((y[4:5].cpu().double() - T.upsample_ref(x[4:5].cpu())).abs().max()) <= 1e-6
    n, h, w, c = BIG["upsample2_bilinear_backward"]
    dy = torch.randn(n, 2 * h, 2 * w, c, generator=g, device=DEV)
    dx = train_ops.upsample2_bilinear_backward(dy)
    for i in range(n):
        assert _same_bits(dx[i:i + 1], train_ops.upsample2_bilinear_backward(dy[i:i + 1])), i
    _, dx_ref = T.upsample_ref(torch.zeros(1, h, w, c), dy[4:5].cpu())
    assert float((dx[4:5].cpu().double() - dx_ref).abs().max()) <= 2e-6 * float(dx_ref.abs().max())


def test_sp_resampling_above_the_grid_cap():
    """10 images: pool of 512 x 512 x 64 and upsample of 128 x 128 x 64, 5 242 880 items each (524 288 per image): the batch
    launch = single-image launches bit for bit (the SP planes themselves); image 7 against torch on the decoded input."""
    from disconet_amd import ops
    g = torch.Generator(device=DEV).manual_seed(3)

    def one(sp, i):
        return ops.SpTensor(1, sp.h, sp.w, sp.c, data=sp.data[i:i + 1])

    n, h, w, c = BIG["sp_maxpool2"]
    sp = ops.SpTensor(n, h, w, c, device=DEV)
    for i in range(n):                       # (image by image: the fp32 copy of the whole batch is not needed)
        sp.data[i:i + 1].copy_(ops.SpTensor.from_nhwc(torch.randn(1, h, w, c, generator=g, device=DEV)).data)
    pooled = ops.sp_maxpool2(sp)
    for i in range(n):
        assert torch.equal(pooled.data[i:i + 1].view(torch.int16), ops.sp_maxpool2(one(sp, i)).data.view(torch.int16)), i
    assert torch.equal(T.bits(one(pooled, 7).nhwc().cpu()), T.bits(T.maxpool_aten(one(sp, 7).nhwc().cpu())))
    n, h, w, c = BIG["sp_upsample2_bilinear"]
    sp = ops.SpTensor.from_nhwc(torch.randn(n, h, w, c, generator=g, device=DEV))
    up = ops.sp_upsample2_bilinear(sp)
    for i in range(n):
        assert torch.equal(up.data[i:i + 1].view(torch.int16), ops.sp_upsample2_bilinear(one(sp, i)).data.view(torch.int16)), i
    want = T.upsample_ref(one(sp, 7).nhwc().cpu())
    assert float((one(up, 7).nhwc().cpu().double() - want).abs().max()) <= 1e-5
