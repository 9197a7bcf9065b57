"""dn_kd_kl_loss, dn_adam_step and dn_seg_ce_loss / dn_seg_label_count against float64 on the CPU (tests/train_small_ops.py)
at channel counts off the 64 lanes, saturated rows, and sizes above each kernel's capped grid, where a thread of the
grid-stride loop runs a second iteration."""
import pytest
import torch

from tests import train_small_ops as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


# ---- knowledge distillation ------------------------------------------------------------------------------------------------
def _kd_check(s, t, kd_weight, norm_rows=None):
    from disconet_amd import train_ops
    ref, dref = T.kd_ref(s, t, kd_weight, norm_rows)
    loss = torch.full((1,), 5.0, dtype=torch.float64, device=DEV)
    d = train_ops.kd_kl_loss(s.to(DEV), t.to(DEV), kd_weight, loss, norm_rows=norm_rows)      # accumulates onto the preset 5
    print("kd", tuple(s.shape), "got", float(loss) - 5.0, "ref", ref)
    assert abs(float(loss) - 5.0 - ref) <= 2e-5 * abs(ref) + 5.0 * 2.0 ** -52
    assert float((d.cpu().double() - dref).abs().max()) <= 2e-5 * float(dref.abs().max())
    zeroed = torch.full((1,), 5.0, dtype=torch.float64, device=DEV)
    d2 = train_ops.kd_kl_loss(s.to(DEV), t.to(DEV), kd_weight, zeroed, zero=True, norm_rows=norm_rows)
    assert abs(float(zeroed) - ref) <= 2e-5 * abs(ref)
    assert torch.equal(d, d2)
    return d


@pytest.mark.parametrize("c", [1, 8, 32, 100, 512])
def test_kd_kl_channel_counts_and_saturated_rows(c):
    """fewer channels than lanes, no multiple of 64, several passes of the lane loop; rows with a student / teacher gap of
    200 (the float32 teacher probabilities underflow to 0: the term is 0 by xlogy's rule and the gradient is still
    softmax(s) * scale), rows of all-equal logits; accumulation onto a preset value against zero=True (the preset 5 may
    cost the accumulated sum one rounding of 5: 2^-52 * 5); norm_rows.  The existing 2e-5; with c = 1 everything is exactly 0."""
    rows = 3 * 7 * 11                                    # odd: the last workgroup of 4 rows is partly filled
    s, t = T.kd_case(rows, c, seed=c)
    s, t = s.view(3, 7, 11, c), t.view(3, 7, 11, c)
    d = _kd_check(s, t, 1e5)
    _kd_check(s, t, 1e5, norm_rows=5 * rows)
    if c == 1:
        assert float(d.abs().max()) == 0.0


def test_kd_kl_more_rows_than_one_pass():
    """33 800 rows x 32 channels against the 8192 workgroups x 4 rows of one pass"""
    rows = 33800
    assert rows > T.KD_ROWS_CAP
    s, t = T.kd_case(rows, 32, seed=3)
    _kd_check(s.view(2, 130, 130, 32), t.view(2, 130, 130, 32), 1e5)


# ---- Adam ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wd,eps", T.ADAM_GRID)
def test_adam_step_matches_float64(wd, eps):
    """n = 1 048 576 + 4 099 elements (a full pass of the capped grid and a partial one), steps 1-3 chained from zero state and
    a step numbered 5000 from non-zero m, v; gradient entries of exactly 0 on m = v = 0, of 1e-20 (the square underflows), of
    +-1e15 and of O(1); weight decay and a non-default eps.  Each step against adam64 on the SAME float32 state.

    m, v -- derived.  With u = 2^-24, G = |g| + wd |p| and b in [0.5, 1) a hyper-parameter rounded to float (relative u),
    its complement c = 1 - b rounded on its own (relative u):
      g' = fl(g + fl(wd p))                     |g' - (g + wd p)| <= u G + 2 u wd |p| <= 3 u G
      m' = fl(fl(b1 m) + fl(c1 g'))             |dm| <= 3 u b1 |m| [b1, product, sum] + (1 - b1) (3 + 3) u G [g' | c1, product, sum]
                                                     <= u (3 |m| + (0.5 + 6 (1 - b1)) G)
      v' = fl(fl(b2 v) + fl(fl(c2 g') g'))      |dv| <= 3 u b2 |v| + (1 - b2) (6 + 4) u G^2 [g' twice | c2, two products, sum]
                                                     <= u (3 |v| + (0.5 + 10 (1 - b2)) G^2)
    (the 0.5 covers a complement formed from the float-rounded b: |c - (1 - b)| <= 2^-25), plus 4 * 2^-126 for products
    that leave the normal range (1e-40 flushed or rounded to a subnormal).  A fused multiply-add only removes roundings.

    update p_new - p_old -- measured (T.ADAM_UPDATE_BOUND): torch's own float32 CPU Adam deviates from adam64 by at most
    4.363e-9 on these inputs (|p| < 0.12: half an ulp of p is 3.7e-9); the kernel is allowed 4 x 4.4e-9 = 1.76e-8.
    Before dn_version 140 (1 - beta from the float-rounded beta) the step-5000 update was 7e-8 off."""
    from disconet_amd import train_ops
    p0, g0, m0, v0 = T.adam_case()
    assert p0.numel() == 1048576 + 4099
    p, m, v = p0.to(DEV), torch.zeros_like(p0, device=DEV), torch.zeros_like(p0, device=DEV)
    for step in T.ADAM_STEPS:
        if step == 5000:
            p, m, v = p0.to(DEV), m0.to(DEV), v0.to(DEV)
        g = T.adam_grad(g0, step)
        before = (p.cpu(), m.cpu(), v.cpu())
        train_ops.adam_step(p, g.to(DEV), m, v, step, lr=1e-3, eps=eps, weight_decay=wd)
        p64, m64, v64 = T.adam64(before[0], g, before[1], before[2], step, lr=1e-3, eps=eps, weight_decay=wd)
        bm, bv = T.adam_mv_bounds(before[0], g, before[1], before[2], (0.9, 0.999), wd)
        em, ev = (m.cpu().double() - m64).abs(), (v.cpu().double() - v64).abs()
        upd = p.cpu().double() - before[0].double()
        eu = (upd - (p64 - before[0].double())).abs()
        print("adam wd %g eps %g step %d: m %.3g of its bound, v %.3g of its bound, update off by %.4g (bound %.4g)"
              % (wd, eps, step, float((em / bm).max()), float((ev / bv).max()), float(eu.max()), T.ADAM_UPDATE_BOUND))
        assert bool((em <= bm).all()), step
        assert bool((ev <= bv).all()), step
        assert float(eu.max()) <= T.ADAM_UPDATE_BOUND, step
        if wd == 0:                                           # g = m = v = 0: 0 / (0 + eps), nothing moves
            zero = (g == 0) & (before[2] == 0)
            assert int(zero.sum()) > 60000 and float(upd[zero].abs().max()) == 0.0
            assert float(m.cpu()[zero].abs().max()) == 0.0 and float(v.cpu()[zero].abs().max()) == 0.0
    assert bool(torch.isfinite(p).all()) and bool(torch.isfinite(v).all())


# ---- segmentation cross-entropy -------------------------------------------------------------------------------------------------
def _live_count(y, classes):
    from disconet_amd import _lib
    from disconet_amd.ops import _ptr, _stream
    lab = y.to(device=DEV, dtype=torch.int32).contiguous()
    counts = torch.empty(2, dtype=torch.int32, device=DEV)
    _lib.check(_lib.load().dn_seg_label_count(_ptr(lab), lab.numel(), classes, _ptr(counts), _stream()), "dn_seg_label_count")
    return counts.tolist()


@pytest.mark.parametrize("classes", [1, 5, 8, 19])
def test_seg_ce_above_both_caps(classes):
    """600 000 pixels against the 524 288 threads of dn_seg_ce_loss and the 262 144 of dn_seg_label_count; the compiled-in 8
    classes and the general path; 30 % ignored; rows with a logit gap of 1e4.  The existing criteria (1e-6 of the loss, 1e-6
    of the largest gradient entry -- without their 1e-9 floor, which would be a third of the largest entry here: the mean
    over 420 000 live pixels makes every entry <= 2.4e-6)."""
    from disconet_amd import ops
    z, y = T.seg_case(classes)
    assert y.numel() == 600000 > T.SEG_CE_CAP
    want, dref = T.seg_ref(z, y)
    loss, grad = ops.seg_ce_loss(z.to(DEV), y.to(DEV))
    print("seg ce", classes, "got", float(loss), "ref", want)
    assert abs(float(loss) - want) <= 1e-6 * abs(want)
    g = grad.cpu()
    assert float((g.double() - dref).abs().max()) <= 1e-6 * float(dref.abs().max())
    assert float(g[y == -100].abs().max()) == 0.0
    assert _live_count(y, classes) == [int((y != -100).sum()), 0]
    if classes == 1:
        assert float(loss) == 0.0 and float(g.abs().max()) == 0.0


@pytest.mark.parametrize("classes", [8, 19])
def test_seg_ce_all_ignored_batch(classes):
    """no live pixel: torch's mean is 0 / 0; the wrapper reports a loss of 0, every gradient entry is exactly 0 and the
    live count is torch's (0)"""
    from disconet_amd import ops
    z, y = T.seg_case(classes, shape=(2, 30, 50))
    y.fill_(-100)
    loss, grad = ops.seg_ce_loss(z.to(DEV), y.to(DEV))
    assert float(loss) == 0.0
    assert float(grad.abs().max()) == 0.0 and bool(torch.isfinite(grad).all())
    assert _live_count(y, classes) == [int((y != -100).sum()), 0] == [0, 0]
