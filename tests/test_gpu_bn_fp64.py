"""Every BatchNorm training kernel (train_ops.hip: statistics, running update, apply, backward reduce, backward apply, the folds
and the channel sums) against the float64 reference of tests/bn_fp64.py, at the shapes that reach each edge of the host
dispatch -- and named: after every call dn_bn_train_last_form (the record the entry points themselves write) must equal the
case's claimed kernel class, U, flags, fold, workgroups and groups, so a dispatch change cannot move a case onto another kernel
unseen.  Every element is held to |got - ref| <= c A (A = 0 -> exactly 0); the SP copies are, bit for bit, tests/sp_format.py's
CPU split of the fp32 tensor the same launch wrote; the byte mask's bits are the reference's wherever |y_ref| > c A.  Outputs,
workspaces and the slack of strided operands hold 7.0 before the call: operands must come back unchanged, an output's
surroundings and a workspace's tail must still hold it.  No environment switch: DN_BN_LEGACY's forms stay with the
child-process A/B test of tests/test_gpu_train_ops.py.

Measured on the MI355X, the largest err / (c A) over the cases of each pass (1.0 is the bound; c = 4 yard, the float32
yardsticks are bn_fp64.YARD; the statistics: c = 4 on one fp32 rounding plus the worst case of the double sums):
    statistics   mean 0.241   var 0.248   fused running update 0.044 / 0.041
    running      mean 0.131   var 0.250
    apply        y 0.235      mask: no determined bit differs
    backward     dz 0.250     dgamma 0.250   dbeta 0.250   dbias 0.247   dz_sp (dz NULL) 0.055
(0.250: the kernel's bits are the float32 yardstick's on the case that sets it.)  First run of the statistics cases, on the
parent's kernels (z squared in fp32 before the double sum): the four `bigmean` cases missed the variance bound 47 to 6919 times
over (up to 2.7e-3 of the variance), the constant channel and the one-row group got a variance of the size of one rounding of
z^2 instead of 0; group_channel_sums now squares in double (profiles/HISTORY.md, profiles/bn_var_double.json)."""
import ctypes

import pytest
import torch

from tests import bn_fp64 as B

pytestmark = pytest.mark.gpu

G = 64                              # guard floats in front of and behind every buffer
BY_KIND = {kind: [k for k in B.CASES if k.kind == kind and not k.refuse] for kind in ("stats", "running", "apply", "bwd")}
REFUSED = [k for k in B.CASES if k.refuse]


def _dev():
    return torch.device("cuda:0")


class _Buf:
    """`numel` floats `off` floats past a 16-byte boundary, inside G floats of 7.0 on either side (the slack inside: also 7.0)"""

    def __init__(self, numel, off=0, fill=None, dtype=torch.float32):
        host = torch.full((2 * G + off + numel,), B.POISON, dtype=dtype)
        self.lo, self.hi = G + off, G + off + numel
        if fill is not None:
            host[self.lo:self.hi] = fill.reshape(-1)
        self.before = host.clone()
        self.dev = host.to(_dev())
        assert self.dev.data_ptr() % 16 == 0
        self.ptr = ctypes.c_void_p(self.dev.data_ptr() + self.dev.element_size() * self.lo)

    def view(self, shape, strides=None):
        return self.dev[self.lo:self.hi].view(shape) if strides is None else self.dev.as_strided(shape, strides, self.lo)

    def unchanged(self):
        return torch.equal(self.dev.cpu().view(torch.uint8), self.before.view(torch.uint8))

    def guards_intact(self):
        d = self.dev.cpu()
        return bool((d[:self.lo] == self.before[:self.lo]).all()) and bool((d[self.hi:] == self.before[self.hi:]).all())

    def get(self):
        return self.dev[self.lo:self.hi].cpu()


def _operand(rows2d, off, ld):
    """a strided operand: rows of ld floats, the channels `off` floats into each row, 7.0 everywhere else"""
    flat = B.embed(rows2d, off, ld)
    return _Buf(flat.numel() - off, off, fill=flat[off:])


def _workspace(nbytes):
    ws = torch.full((nbytes + 4096,), 7, dtype=torch.uint8, device=_dev())
    return ws, lambda: bool((ws[nbytes:] == 7).all())


def _record(*passes):
    from disconet_amd import train_ops
    return {p: train_ops.bn_last_form(p) for p in passes}


def _held(case):
    """the launch record of the case's passes against its claim"""
    claim = case.claim()
    got = _record(*claim)
    for p, want in claim.items():
        assert {f: got[p][f] for f in want} == want, (p, got[p], want)
    return got


def _report(case, r, rec):
    print("RECORD %s %s worst err / (c A): %s" % (case.name, {p: sorted(v.items()) for p, v in rec.items()},
                                                   {n: round(v, 3) for n, v in r.items()}))
    assert r and max(r.values()) <= 1.0, r


# --- statistics ------------------------------------------------------------------------------------------------
def _run_stats(case):
    from disconet_amd import _lib, train_ops
    lib, k, m = _lib.load(), case, B.make(case)
    Gn, R, c = k.groups, k.rpg, k.c
    z = _operand(m.z.reshape(-1, c), k.off, k.ldz)
    assert (z.ptr.value % 16 == 0) == (k.off % 4 == 0)
    nbytes = lib.dn_reduce_workspace_bytes(Gn, R, c)
    ws, tail_ok = _workspace(nbytes)
    mean, var = _Buf(Gn * c), _Buf(Gn * c)
    rm = rv = None
    stream = train_ops._stream()
    if k.sync:
        assert lib.dn_bn_train_stats_partial(z.ptr, Gn, R, c, k.ldz, train_ops._ptr(ws), nbytes, stream) == 0
        folded = ws[:Gn * 2 * c * 8].view(torch.float64)
        folded += m.sumsB.reshape(-1).to(_dev())                     # the all-reduce: the other rank's folded sums
        assert lib.dn_bn_train_stats_finish(train_ops._ptr(ws), Gn, k.norm_rows, c, mean.ptr, var.ptr, stream) == 0
    else:
        if k.running is not None:
            rm, rv = _Buf(c, fill=m.rm0), _Buf(c, fill=m.rv0)
        assert lib.dn_bn_train_stats(z.ptr, Gn, R, c, k.ldz, train_ops._ptr(ws), nbytes, mean.ptr, var.ptr, rm.ptr if rm else None,
                                     rv.ptr if rv else None, float(k.running or 0.0), stream) == 0
    torch.cuda.synchronize()
    assert z.unchanged() and tail_ok() and mean.guards_intact() and var.guards_intact()
    outs = {"mean": mean.get().view(Gn, c).double(), "var": var.get().view(Gn, c).double()}
    if rm is not None:
        assert rm.guards_intact() and rv.guards_intact()
        outs["rm"], outs["rv"] = rm.get().double(), rv.get().double()
    return outs


@pytest.mark.parametrize("case", BY_KIND["stats"], ids=lambda k: k.name)
def test_statistics_are_inside_the_bound_on_the_claimed_kernels(case):
    outs = _run_stats(case)
    rec = _held(case)
    assert float(outs["var"].min()) >= 0.0
    _report(case, B.judge(case, outs), rec)
    again = _run_stats(case)
    assert all(torch.equal(again[n], outs[n]) for n in outs), "two launches, two results"


# --- running statistics ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", BY_KIND["running"], ids=lambda k: k.name)
def test_running_update_follows_the_recurrence_in_the_order_given(case):
    from disconet_amd import train_ops
    k, m = case, B.make(case)
    n_stat, c = k.shape
    mean, var = _Buf(n_stat * c, fill=m.mean), _Buf(n_stat * c, fill=m.var)
    rm, rv = _Buf(c, fill=m.rm0), _Buf(c, fill=m.rv0)
    order = torch.tensor(k.order, dtype=torch.int32, device=_dev()) if k.order else None
    train_ops.bn_update_running(mean.view((n_stat, c)), var.view((n_stat, c)), k.rows, rm.view((c,)), rv.view((c,)), k.momentum, order)
    torch.cuda.synchronize()
    assert mean.unchanged() and var.unchanged() and rm.guards_intact() and rv.guards_intact()
    rec = _held(case)
    _report(case, B.judge(case, {"rm": rm.get().double(), "rv": rv.get().double()}), rec)


# --- apply ------------------------------------------------------------------------------------------------------
def _sp_tensor(shape):
    from disconet_amd import ops
    n, h, w, c = shape
    buf = _Buf(n * (c // 16) * 4 * h * w * 8, dtype=torch.float16)
    return ops.SpTensor(n, h, w, c, data=buf.view((n, c // 16, 4, h, w, 8))), buf


def _sp_get(buf):
    return buf.get().view(torch.uint8)


def _run_apply(case):
    from disconet_amd import _lib, ops, train_ops
    lib, k, m = _lib.load(), case, B.make(case)
    n, h, w, c = k.shape
    z = _operand(m.z.reshape(-1, c), k.off, k.ldz)
    mean, var, gamma, beta = (_Buf(t.numel(), fill=t) for t in (m.mean, m.var, m.gamma, m.beta))
    y = _Buf(k.total)
    mask = _Buf(k.total // 4, dtype=torch.uint8) if k.mask else None
    sp, spbuf = _sp_tensor(k.shape) if k.sp else (None, None)
    before = _record("apply")
    ops.sp_range_flags(reset=True)
    rc = lib.dn_bn_train_apply(z.ptr, mean.ptr, var.ptr, gamma.ptr, beta.ptr, B.EPS, k.relu, k.groups, k.rpg, c, k.ldz, y.ptr,
                               mask.ptr if mask else None, train_ops._ptr(sp.data) if sp else None, h * w if sp else 0, train_ops._stream())
    torch.cuda.synchronize()
    assert all(b.unchanged() for b in (z, mean, var, gamma, beta)) and y.guards_intact()
    assert (mask is None or mask.guards_intact()) and (spbuf is None or spbuf.guards_intact())
    if rc != 0:
        assert _record("apply") == before, "a refused call changed the launch record"
        assert y.unchanged() and (mask is None or mask.unchanged()), "a refused call wrote its outputs"
        return rc, None
    assert ops.sp_range_flags(reset=True) == 0
    y32 = y.get().view(k.groups, k.rpg, c)
    outs = {"y": y32.double()}
    if mask:
        outs["mask"] = mask.get()
        if k.relu:      # the mask and y of one launch agree wherever y says anything: y > 0 -> bit set
            assert not bool(((y32 > 0) & ~B.gate_of(outs["mask"], y32.shape)).any())
    if sp:
        assert torch.equal(_sp_get(spbuf), B.sp_bytes(y32.view(k.shape))), "y_sp is not the split of the y this launch wrote"
    return rc, outs


@pytest.mark.parametrize("case", BY_KIND["apply"], ids=lambda k: k.name)
def test_apply_is_inside_the_bound_on_the_claimed_kernel(case):
    rc, outs = _run_apply(case)
    assert rc == 0
    rec = _held(case)
    if case.mask:
        assert B.mask_free_share(case) <= B.MASK_FREE_CAP
    _report(case, B.judge(case, outs), rec)
    if case.vals == "gate":
        assert torch.equal(outs["y"][..., :3], torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64).expand_as(outs["y"][..., :3]))


@pytest.mark.parametrize("case", REFUSED, ids=lambda k: k.name)
def test_the_byte_mask_is_refused_where_the_scalar_kernel_runs(case):
    rc, outs = _run_apply(case)
    assert rc != 0 and outs is None


# --- backward ----------------------------------------------------------------------------------------------------
def _run_bwd(case):
    from disconet_amd import _lib, ops, train_ops
    lib, k, m = _lib.load(), case, B.make(case)
    n, h, w, c = k.shape
    Gn, R = k.groups, k.rpg
    off, ld = k.a_layout
    a_shape = m.dy_a.shape
    dy_a = _operand(m.dy_a.reshape(-1, a_shape[-1]), off, ld)
    an, ah, aw, ac = a_shape
    a_view = dy_a.view(a_shape, (ah * aw * ld, aw * ld, ld, 1))
    dy_b = _operand(m.dy_b.reshape(-1, c), 0, c + 4) if k.dyb else None
    b_view = dy_b.view((n, h, w, c), (h * w * (c + 4), w * (c + 4), c + 4, 1)) if k.dyb else None
    z, y = _Buf(k.total, fill=m.z), _Buf(k.total, fill=m.y)
    mean, var, gamma = (_Buf(t.numel(), fill=t) for t in (m.mean, m.var, m.gamma))
    maskb = _Buf(k.total // 4, fill=m.maskbytes, dtype=torch.uint8) if k.relu == 2 else None
    dgamma = _Buf(c, fill=m.old_dgamma if k.accumulate else None)
    dbeta = _Buf(c, fill=m.old_dbeta if k.accumulate else None)
    dz = _Buf(k.total) if k.want_dz else None
    dbias = _Buf(c) if k.bias else None
    sp, spbuf = _sp_tensor(k.shape) if k.sp else (None, None)
    nbytes = lib.dn_reduce_workspace_bytes(Gn, R, c)
    ws = train_ops._ws(_dev(), nbytes)
    ws.fill_(7)
    folds, small = None, []
    if k.bias == "deferred":      # 32 tiny channel sums in front: the bias fold is job 33, alone in the second launch
        folds = train_ops.DeferredFolds()
        for x in B.fold_jobs_inputs():
            out = _Buf(x.shape[1])
            train_ops.channel_sum(x.to(_dev()), out.view((x.shape[1],)), folds=folds)
            small.append((x, out, train_ops.bn_last_form("channel_sum")))
    sync = None
    if k.sync:
        sumsB = m.sumsB.reshape(-1).to(_dev())
        sync = lambda folded: folded.add_(sumsB)      # noqa: E731
    ops.sp_range_flags(reset=True)
    got = train_ops.bn_backward(a_view, maskb.view((k.total // 4,)) if maskb else y.view(k.shape), z.view(k.shape), mean.view((Gn, c)),
                                var.view((Gn, c)), gamma.view((c,)), B.EPS, dgamma.view((c,)), dbeta.view((c,)), relu=bool(k.relu),
                                dy_b=b_view, up_a={"up1": 1, "s2d": 2}.get(k.src, 0), accumulate=k.accumulate,
                                out=dz.view(k.shape) if dz else None, sync=sync, norm_rows=k.norm_rows if k.sync else None, sp_out=sp,
                                sp_lift=B.SP_LIFT, relu_mask=maskb.view((k.total // 4,)) if maskb else None,
                                dbias=dbias.view((c,)) if dbias else None, folds=folds, want_dz=k.want_dz)
    rec = _held(case)
    if folds is not None:
        folds.run()
    torch.cuda.synchronize()
    assert got is None or got.data_ptr() == dz.ptr.value
    assert ops.sp_range_flags(reset=True) == 0
    assert all(b.unchanged() for b in (dy_a, z, y, mean, var, gamma) + ((dy_b,) if dy_b else ()) + ((maskb,) if maskb else ()))
    assert all(b.guards_intact() for b in (dgamma, dbeta) + tuple(b for b in (dz, dbias, spbuf) if b is not None))
    assert bool((ws[nbytes:] == 7).all()), "the reduction wrote past dn_reduce_workspace_bytes() bytes"
    outs = {"dgamma": dgamma.get().double(), "dbeta": dbeta.get().double()}
    if dz:
        outs["dz"] = dz.get().view(Gn, R, c).double()
    if dbias:
        outs["dbias"] = dbias.get().double()
    if sp:
        if dz:
            assert torch.equal(_sp_get(spbuf), B.sp_bytes((dz.get() * B.SP_LIFT).view(k.shape))), "dz_sp is not the split of this launch's dz"
        outs["dz_sp"] = B.sp_values(_sp_get(spbuf), k.shape).view(Gn, R, c) / B.SP_LIFT
    if folds is not None:
        fm = train_ops.bn_last_form("fold_multi")
        assert (fm["fold"], fm["grid"], fm["groups"], fm["c"]) == (7, 1, 2, c), fm      # 33 jobs: 32 + 1, the last launch folds c channels
        for x, out, form in small:
            assert out.guards_intact()
            want = dict(cls=int(x.shape[1] % 4 == 0), u=4 if x.shape[1] % 4 == 0 else 1, fold=B.FOLD_DEFERRED, grid=1, c=x.shape[1])
            assert {f: form[f] for f in want} == want, form
            r = B.worst(out.get().double(), B.channel_sum_reference(x), B.MARGIN * B.P24)
            assert r <= 1.0, ("channel_sum job", tuple(x.shape), r)
    return outs, rec


@pytest.mark.parametrize("case", BY_KIND["bwd"], ids=lambda k: k.name)
def test_backward_is_inside_the_bound_on_the_claimed_kernels(case):
    outs, rec = _run_bwd(case)
    _report(case, B.judge(case, outs), rec)
    if case.vals == "gate" and case.want_dz:
        assert not bool(outs["dz"][..., :3].any())
    again, _ = _run_bwd(case)
    assert all(torch.equal(again[n], outs[n]) for n in outs), "two launches, two results"
