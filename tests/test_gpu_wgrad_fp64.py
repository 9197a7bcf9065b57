"""Every weight-gradient kernel (conv_wgrad.hip, wgrad_sp.inl) against the float64 reference of tests/wgrad_fp64.py, at the
shapes that reach each plan edge -- and named: after every launch dn_conv_wgrad_last_form (the record the entry points
themselves write) must equal the case's claimed kernel, vector flags, grid and slice count, so a dispatch change cannot move
a case onto another kernel unseen.  Every element is held to |got - dW| <= c A (A = sum |dz~| |x~|, A = 0 -> exactly 0); the
operands' surroundings, the workspace behind dn_conv_wgrad*_workspace() bytes and dW's surroundings (the other columns of a
wider weight included) are 0xFF bytes before the launch and must be 0xFF bytes after it; a second launch must give the same
bits; the SP-dz entry (dn_conv_wgrad_sp_z) must give the fp32-dz entry's bits; no range flag.

Measured on the MI355X, largest err / (c A) over the cases of each form (1.0 is the bound; c = 4 yard, + 2^-22 for the
split-f16 kernels; the float32 yardsticks are wgrad_fp64.YARD: 1.2e-7 .. 3.4e-7 of A per family, 8.4e-7 for the one family
with a dz at 65504):
    F32-3x3s1 0.217   F32-3x3s2 0.202   F32-1x1 0.209   F64 0.282
    SP64s1 0.248      SP32s1 0.158      SP64s2 0.165    SP32s2 0.123
The SP-dz instantiations give the fp32-dz instantiations' bits on every case with c_out % 16 == 0, so the figures are theirs
too.  First run of this file: both dz-at-65504 cases raised the "clamped" range flag although nothing was clamped (the staging
pass took its maximum after the clamp and could not tell 65504 from beyond); wgrad_sp.inl now takes it before the clamp."""
import ctypes

import pytest
import torch

from tests import wgrad_fp64 as W
from tests.nhwc_conv_fp64 import PARITY_MASKS

pytestmark = pytest.mark.gpu

G = 64                              # guard floats in front of and behind every buffer
RUN = [c for c in W.CASES if not c.refuse]
REFUSED = [c for c in W.CASES if c.refuse]


def _dev():
    return torch.device("cuda:0")


def _ff(numel):
    return torch.full((numel,), -1, dtype=torch.int32).view(torch.float32)


def _intact(t):
    return bool((t.view(torch.int32) == -1).all())


class _Operand:
    """an NCHW fp32 map as NHWC rows of `ld` floats, `off` floats into each row, inside 0xFF bytes"""

    def __init__(self, x, off, pad):
        n, c, h, w = x.shape
        self.ld, npx = off + c + pad, n * h * w
        flat = _ff(2 * G + npx * self.ld)
        flat[G:G + npx * self.ld].view(npx, self.ld)[:, off:off + c] = x.permute(0, 2, 3, 1).reshape(npx, c)
        self.before = flat.clone()
        self.buf = flat.to(_dev())
        self.ptr = ctypes.c_void_p(self.buf.data_ptr() + 4 * (G + off))
        self.dense = torch.empty(n, h, w, c).copy_(x.permute(0, 2, 3, 1))     # fresh: a 1-pixel map keeps its row stride of c

    def unchanged(self):
        return torch.equal(self.buf.cpu().view(torch.int32), self.before.view(torch.int32))


def _launch(case, entry):
    """one launch of `case` through entry "f32" (dn_conv_wgrad) | "sp" (dn_conv_wgrad_sp) | "spz" (dn_conv_wgrad_sp_z: dz only as
    SpTensor.from_nhwc(dz * lift)) -> (rc, dW block float32 on the CPU or None, the launch record)"""
    from disconet_amd import _lib, ops, train_ops
    lib = _lib.load()
    c, m = case, W.make(case)
    d = W.desc_of(c, ops.conv_desc)
    kk, c_in = c.k * c.k, c.c0 + c.c1
    src0 = _Operand(m.x0, c.off[0], c.pad[0])
    src1 = _Operand(m.x1, c.off[1], c.pad[1]) if c.c1 else None
    dz = _Operand(m.dz, c.off[2], c.pad[2])
    spec = W.arg_spec(c)
    for name, op in (("src0", src0), ("src1", src1), ("dz", dz)):
        assert spec[name][0] == (op is not None) and (op is None or op.ptr.value % 16 == spec[name][1])
    nbytes = (lib.dn_conv_wgrad_sp_workspace if c.eng == "sp" else lib.dn_conv_wgrad_workspace)(ctypes.byref(d))
    assert nbytes > 0 and nbytes % 16 == 0
    ws = torch.full((nbytes + 4096,), 0xFF, dtype=torch.uint8, device=_dev())
    total = c.cin_total or c_in
    full = _ff(2 * G + c.c_out * total * kk)
    block = full[G:G + c.c_out * total * kk].view(c.c_out, total, c.k, c.k)[:, c.ci_first:c.ci_first + c_in]
    if m.old is not None:
        block.copy_(m.old)
    dwbuf = full.to(_dev())
    dw = ctypes.c_void_p(dwbuf.data_ptr() + 4 * (G + c.ci_first * kk))
    p1 = src1.ptr if src1 else None
    before = train_ops.conv_wgrad_last_form()
    ops.sp_range_flags(reset=True)
    stream = train_ops._stream()
    if entry == "f32":
        rc = lib.dn_conv_wgrad(ctypes.byref(d), src0.ptr, p1, dz.ptr, train_ops._ptr(ws), dw, c.cin_total, int(c.accumulate), stream)
    elif entry == "sp":
        rc = lib.dn_conv_wgrad_sp(ctypes.byref(d), src0.ptr, p1, dz.ptr, train_ops._ptr(ws), dw, c.cin_total, int(c.accumulate),
                                  m.dz_lift, W.X_LIFT, stream)
    else:
        zsp = ops.SpTensor.from_nhwc(dz.dense.to(_dev()) * m.dz_lift)
        ops.sp_range_flags(reset=True)
        rc = lib.dn_conv_wgrad_sp_z(ctypes.byref(d), src0.ptr, p1, train_ops._ptr(zsp.data), train_ops._ptr(ws), dw, c.cin_total,
                                    int(c.accumulate), m.dz_lift, W.X_LIFT, stream)
    torch.cuda.synchronize()
    after = train_ops.conv_wgrad_last_form()
    # memory outside the result: operands whole, the workspace's tail, dW's guards and the other columns of a wider weight
    assert src0.unchanged() and dz.unchanged() and (src1 is None or src1.unchanged())
    assert bool((ws[nbytes:] == 0xFF).all()), "the workspace was written past dn_conv_wgrad*_workspace() bytes"
    out = dwbuf.cpu()
    assert _intact(out[:G]) and _intact(out[-G:])
    wide = out[G:-G].view(c.c_out, total, c.k, c.k)
    assert _intact(wide[:, :c.ci_first]) and _intact(wide[:, c.ci_first + c_in:])
    got = wide[:, c.ci_first:c.ci_first + c_in].contiguous()
    if rc != 0:
        assert after == before, "a refused call changed the launch record"
        assert _intact(got), "a refused call wrote dW"
        return rc, None, after
    assert ops.sp_range_flags(reset=True) & 5 == 0
    return rc, got, after


def _claim(case, zsp=False):
    claim = case.form_claim(zsp)
    claim["grid"] = -(-case.c_out // case.ct) * (-(-case.c0 // case.ct) + -(-case.c1 // case.ct)) * case.n_slices
    return claim


@pytest.mark.parametrize("case", RUN, ids=lambda c: c.name)
def test_kernel_is_the_claimed_one_and_inside_the_bound(case):
    entry = "sp" if case.eng == "sp" else "f32"
    rc, got, form = _launch(case, entry)
    assert rc == 0
    assert form == _claim(case), "the launch ran another kernel or plan than the case claims"
    ref, c = W.reference(case), W.c_of(case)
    r = W.worst(got, ref, c)
    print("RECORD %s %s worst err / (c A) = %.3f" % (case.name, sorted(form.items()), r))
    assert r <= 1.0, (r, W.breakdown(got, ref, c, case.c0))
    if case.vals == "zero":
        assert not bool(got.any())
    rc, again, _ = _launch(case, entry)
    assert rc == 0 and torch.equal(again.view(torch.int32), got.view(torch.int32)), "two launches, two results"
    if case.eng == "sp" and case.c_out % 16 == 0:
        rc, via_sp, form = _launch(case, "spz")
        print("RECORD %s %s the same bits" % (case.name, sorted(form.items())))
        assert rc == 0 and form == _claim(case, zsp=True)
        assert torch.equal(via_sp.view(torch.int32), got.view(torch.int32)), "the SP-dz entry gave other bits"


@pytest.mark.parametrize("case", REFUSED, ids=lambda c: c.name)
def test_misaligned_operand_is_refused_before_any_launch(case):
    rc, got, _ = _launch(case, "sp" if case.eng == "sp" else "f32")
    assert rc != 0 and got is None


# --- the weight transforms of the data gradient: exact, bit for bit against indexing -------------------------------
def _guarded_out(numel):
    buf = _ff(2 * G + numel).to(_dev())
    return buf, ctypes.c_void_p(buf.data_ptr() + 4 * G)


def _check_out(buf, want):
    out = buf.cpu()
    assert _intact(out[:G]) and _intact(out[-G:])
    assert torch.equal(out[G:-G].view(torch.int32), want.contiguous().view(-1).view(torch.int32))


# c_out, cin_total, ci_first, c_in: a column block in the middle; the last one is above the grid-stride cap of 4096 x 256
TRANSFORM_SHAPES = [(5, 11, 3, 6), (33, 40, 8, 32), (256, 520, 4, 512)]


@pytest.mark.parametrize("shape", TRANSFORM_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("k", [1, 3])
def test_dgrad_weights_is_the_flipped_transposed_column_block(shape, k):
    from disconet_amd import _lib, train_ops
    c_out, cin_total, ci_first, c_in = shape
    w = torch.randn(c_out, cin_total, k, k, generator=torch.Generator().manual_seed(c_out + k))
    buf, ptr = _guarded_out(c_in * c_out * k * k)
    wd = w.to(_dev())
    assert _lib.load().dn_conv_dgrad_weights(train_ops._ptr(wd), c_out, cin_total, ci_first, c_in, k, ptr, train_ops._stream()) == 0
    torch.cuda.synchronize()
    _check_out(buf, w[:, ci_first:ci_first + c_in].permute(1, 0, 2, 3).flip(2, 3))


@pytest.mark.parametrize("shape", TRANSFORM_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("parity", sorted(PARITY_MASKS))
def test_dgrad_class_weights_are_the_taps_of_the_parity_class(shape, parity):
    from disconet_amd import _lib, train_ops
    c_out, cin_total, ci_first, c_in = shape
    py, px = parity
    w = torch.randn(c_out, cin_total, 3, 3, generator=torch.Generator().manual_seed(c_out + 7))
    src = {0: {1: 1}, 1: {1: 2, 2: 0}}                       # parity -> {tap of the class: tap of the layer}
    want = torch.zeros(c_in, c_out, 3, 3)
    cut = w[:, ci_first:ci_first + c_in].permute(1, 0, 2, 3)
    for vy, ty in src[py].items():
        for vx, tx in src[px].items():
            want[:, :, vy, vx] = cut[:, :, ty, tx]
    buf, ptr = _guarded_out(c_in * c_out * 9)
    wd = w.to(_dev())
    mask = ctypes.c_int(0)
    assert _lib.load().dn_conv_dgrad_class_weights(train_ops._ptr(wd), c_out, cin_total, ci_first, c_in, py, px, ptr, ctypes.byref(mask),
                                                   train_ops._stream()) == 0
    torch.cuda.synchronize()
    _check_out(buf, want)
    assert mask.value == PARITY_MASKS[parity]
    assert {vy * 3 + vx for vy in src[py] for vx in src[px]} == {t for t in range(9) if mask.value >> t & 1}
