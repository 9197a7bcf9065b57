"""dn_det_loss (focal + smooth-L1, both kernels: the float4 streams and the per-anchor form) against
oracle.train_ref.det_loss in float64 under autograd, where the unit test of tests/test_gpu_train_ops.py does not look:
saturated logits (the clamped focal form stopped at a wrong-side gap of ln 1e30 = 69), the smooth-L1 threshold and its
float neighbours, "don't care" rows, and an input long enough for the grid-stride loops of both kernels to iterate.

Tolerances are those of test_det_loss_and_gradients_match_the_oracle: 1e-5 of each loss, 2e-5 for the gradients -- the
class gradient per anchor against |ref| + a_t / norm, a_t / norm being the magnitude it saturates at."""
import pytest
import torch

from tests import train_small_ops as T

pytestmark = pytest.mark.gpu


def _run(tensors, norm, alpha, gamma, sigma, unaligned=False):
    """-> (losses [2] float64 cpu, dcls cpu, dloc cpu, took the float4 path?)"""
    from disconet_amd import train_ops
    dev = torch.device("cuda:0")
    cls, labels, loc, targets, mask = (t.to(dev) for t in tensors)
    if unaligned:
        cls = T.unaligned_copy(cls)
    n, code = loc.shape
    v4 = T.det_takes_float4_path(n, code, cls.data_ptr(), labels.data_ptr(), loc.data_ptr(), targets.data_ptr())
    losses, dcls, dloc = train_ops.det_loss(cls, labels, loc, targets, mask, norm=norm, alpha=alpha, gamma=gamma, sigma=sigma)
    return losses.cpu(), dcls.cpu(), dloc.cpu(), v4


def _check(got, tensors, norm, alpha, gamma, sigma, what):
    losses, dcls, dloc, _ = got
    l_cls, l_loc, rc, rl = T.det_ref(*tensors, norm, alpha, gamma, sigma)
    print(what, "loss got %.9g %.9g ref %.9g %.9g" % (float(losses[0]), float(losses[1]), l_cls, l_loc))
    assert abs(float(losses[0]) - l_cls) <= 1e-5 * abs(l_cls), (what, float(losses[0]), l_cls)
    assert abs(float(losses[1]) - l_loc) <= 1e-5 * abs(l_loc), (what, float(losses[1]), l_loc)
    scale = T.focal_grad_scale(tensors[1], alpha, norm).unsqueeze(1)
    err = (dcls.double() - rc).abs()
    bound = 2e-5 * (rc.abs() + scale)
    worst = int((err - bound).max(1).values.argmax())
    print(what, "dcls worst anchor %d got %s ref %s" % (worst, dcls[worst].tolist(), rc[worst].tolist()))
    assert bool((err <= bound).all()), (what, worst, dcls[worst].tolist(), rc[worst].tolist())
    assert float((dloc.double() - rl).abs().max()) <= 2e-5 * float(rl.abs().max()), what
    return l_cls, l_loc


PARAMS = [(gamma, alpha, sigma, code) for gamma in (0.0, 1.0, 2.0) for alpha in (0.25, 0.5) for sigma in (1.0, 3.0) for code in (6, 7)]


@pytest.mark.parametrize("gamma,alpha,sigma,code", PARAMS)
def test_focal_saturation_sweep(gamma, alpha, sigma, code):
    """every gap of T.GAPS (0 ... 120, 1e4), each target class, each sign of the gap: four anchors of one class per call
    (so a loss is a per-gap, per-class number), once through the float4 kernel and once through the per-anchor kernel
    (the same tensors from an 8-byte-offset `cls` view): losses and per-anchor gradients against float64, and
    dcls / dloc of the two kernels bit for bit.
    Against the kernels of dn_version 139 (log q = logf(max(q, 1e-30)), gradient divided by the clamp) this fails at
    every gap >= 70; the first to fail (gamma 2, alpha 0.25, background, gap 70, float4 kernel): class loss 51.8082 for 52.5."""
    norm = 2.0
    for gap in T.GAPS:
        for fg in (False, True):
            tensors = T.sweep_case(gap, fg, code)
            what = "gap %g %s" % (gap, "fg" if fg else "bg")
            a = _run(tensors, norm, alpha, gamma, sigma)
            b = _run(tensors, norm, alpha, gamma, sigma, unaligned=True)
            assert a[3] and not b[3]
            _check(a, tensors, norm, alpha, gamma, sigma, what + " float4")
            _check(b, tensors, norm, alpha, gamma, sigma, what + " scalar")
            assert torch.equal(T.bits(a[1]), T.bits(b[1])) and torch.equal(T.bits(a[2]), T.bits(b[2])), what


@pytest.mark.parametrize("gamma,alpha,sigma,code", [p for p in PARAMS if p[1] == 0.25])
def test_scalar_path_by_count_and_dont_care_rows(gamma, alpha, sigma, code):
    """the per-anchor kernel reached by the COUNT: odd n, and code 7 with n even but n * code % 4 != 0 -- saturated rows
    of both classes and signs plus "don't care" rows (all-zero label): their gradient is exactly 0 and they add no loss;
    a batch of only such rows under mask 0 gives two losses of exactly 0."""
    norm = 3.0
    parts = [T.sweep_case(gap, fg, code, seed=int(gap)) for gap in (0.0, 30.0, 75.0, 1e4) for fg in (False, True)]
    full = [torch.cat([p[k] for p in parts]) for k in range(5)]           # 32 anchors
    for n in (5, 6, 31, 32):
        tensors = [t[:n].clone() for t in full]
        tensors[1][1] = 0
        tensors[1][n - 1] = 0                                             # two "don't care" rows, one with a mask of 1
        tensors[4][1] = 1.0
        for unaligned in (False, True):
            got = _run(tensors, norm, alpha, gamma, sigma, unaligned)
            assert got[3] == (not unaligned and T.det_takes_float4_path(n, code))
            l_cls, _ = _check(got, tensors, norm, alpha, gamma, sigma, "n %d code %d" % (n, code))
            assert float(got[1][1].abs().max()) == 0 and float(got[1][n - 1].abs().max()) == 0
            # no loss from those rows: the same call without them gives the same class loss
            keep = [t[[k for k in range(n) if k not in (1, n - 1)]] for t in tensors]
            assert abs(T.det_ref(*keep, norm, alpha, gamma, sigma)[0] - l_cls) <= 1e-14 * l_cls
    assert not T.det_takes_float4_path(6, 7) and not T.det_takes_float4_path(5, 6) and T.det_takes_float4_path(32, 7)
    for n in (3, 4):
        tensors = [t[:n].clone() for t in full]
        tensors[1].zero_()
        tensors[4].zero_()
        losses, dcls, dloc, _ = _run(tensors, norm, alpha, gamma, sigma)
        assert float(losses[0]) == 0.0 and float(losses[1]) == 0.0
        assert float(dcls.abs().max()) == 0.0 and float(dloc.abs().max()) == 0.0


@pytest.mark.parametrize("sigma", [1.0, 3.0])
@pytest.mark.parametrize("code", [6, 7])
def test_smooth_l1_at_its_threshold_and_beyond(sigma, code):
    """residuals of 0, -0, +-1/sigma^2 and their float neighbours on both sides (the two branches meet there in value and
    slope, so whichever side float32 takes is within the tolerance), ordinary ones, and +-1e6 / 3e30; masks of 0 and 1;
    both kernels.  A masked-out element has a gradient of exactly 0."""
    for big in (False, True):
        tensors = T.smooth_l1_edge_case(sigma, code, big)
        a = _run(tensors, 2.0, 0.25, 2.0, sigma)
        b = _run(tensors, 2.0, 0.25, 2.0, sigma, unaligned=True)
        assert a[3] and not b[3]
        for got, what in ((a, "float4"), (b, "scalar")):
            _check(got, tensors, 2.0, 0.25, 2.0, sigma, "sigma %g code %d big %d %s" % (sigma, code, big, what))
            assert float(got[2][tensors[4] == 0].abs().max()) == 0.0
        assert torch.equal(T.bits(a[1]), T.bits(b[1])) and torch.equal(T.bits(a[2]), T.bits(b[2]))
        if not big:      # without the huge residuals in the maximum: every element to 2e-5 of its own saturated size, 1 / norm
            _, _, _, rl = T.det_ref(*tensors, 2.0, 0.25, 2.0, sigma)
            assert bool(((a[2].double() - rl).abs() <= 2e-5 * (rl.abs() + 0.5 * tensors[4].double().unsqueeze(1))).all())


def test_long_input_both_kernels():
    """786 432 anchors (two 256 x 256 x 6 maps): 1 179 648 float4s of loc against the float4 kernel's 1 048 576 threads, and
    786 432 anchors against the per-anchor kernel's 524 288 -- both grid-stride loops iterate.  Each against the float64
    oracle; dcls / dloc of the two bit for bit."""
    tensors = T.long_det_case()[:5]
    norm = 2.0
    a = _run(tensors, norm, 0.25, 2.0, 3.0)
    b = _run(tensors, norm, 0.25, 2.0, 3.0, unaligned=True)
    assert a[3] and not b[3]
    l_cls, l_loc, rc, rl = T.det_ref(*tensors, norm, 0.25, 2.0, 3.0)
    scale = T.focal_grad_scale(tensors[1], 0.25, norm).unsqueeze(1)
    for (losses, dcls, dloc, _), what in ((a, "float4"), (b, "scalar")):
        print(what, "losses", losses.tolist(), "ref", l_cls, l_loc)
        assert abs(float(losses[0]) - l_cls) <= 1e-5 * abs(l_cls), what
        assert abs(float(losses[1]) - l_loc) <= 1e-5 * abs(l_loc), what
        assert float((dcls.double() - rc).abs().max()) <= 2e-5 * float(rc.abs().max()), what
        assert float((dloc.double() - rl).abs().max()) <= 2e-5 * float(rl.abs().max()), what
        assert bool(((dcls.double() - rc).abs() <= 2e-5 * (rc.abs() + scale)).all()), what
    assert torch.equal(T.bits(a[1]), T.bits(b[1])) and torch.equal(T.bits(a[2]), T.bits(b[2]))
    assert float((a[0] - b[0]).abs().max()) <= 1e-12 * float(a[0].abs().max())
