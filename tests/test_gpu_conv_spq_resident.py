"""The resident-weights form of conv_spq_kernel (conv_spq.hip, RES = 1: the class-private weights of the upsampled source in
registers, those of the second source in LDS, for the whole launch) against the streaming BN = 32 form it replaces on
conv8_1's layer class.

Per case, with output buffers pre-filled with 0xFF bytes: the forced resident form (dn_spconv_force_config(26)) equals the
forced streaming form (20) bit for bit on the SP output and on the fp32 rows, and stays inside the float64 bound of
tests/conv_fp64.py for its family; which form ran is read from dn_spconv_last_resident() beside dn_spconv_last_form().
Eligibility is asserted by shape: without a forced form the dispatch takes the resident form at <= 4 + 2 chunks,
c_out <= 32 and more work items than CUs, and not at c0 = 80, c1 = 48, c_out = 64 or with K slices.

Measured on the MI355X (21 tests, 3.4 s, CPU references included): every case bit-identical; the largest err / (c A) is
0.266 (ragged, pos, fp32 rows), the persistent case 0.195 (SP) / 0.230 (fp32 rows)."""
import ctypes

import pytest
import torch

from tests import conv_fp64 as C
from tests.conv_fp64 import Case

FORCE_STREAM, FORCE_RESIDENT = 20, 26          # enum SpForceId of disconet_amd/csrc/conv_sp.hip
Q = dict(up0=True, merge="quad")

# (case, epilogue): "sp" dn_spconv2d, "dual" dn_spconv2d_dual (SP + fp32 rows), "nhwc" dn_spconv2d_nhwc (fp32 rows only)
CASES = {
    "one tile, 4 + 2 chunks": (Case(1, 8, 32, 64, 32, c1=32, **Q), "dual"),
    "one tile, pos": (Case(1, 8, 32, 64, 32, c1=32, sign="pos", **Q), "sp"),
    "ragged both ways": (Case(2, 12, 40, 64, 32, c1=32, **Q), "dual"),
    "ragged, pos": (Case(2, 12, 40, 64, 32, c1=32, sign="pos", **Q), "nhwc"),
    "short K, c0 16 c1 4": (Case(2, 12, 40, 16, 32, c1=4, sign="pos", **Q), "dual"),
    "short K, c0 48 c1 16": (Case(2, 12, 40, 48, 32, c1=16, **Q), "dual"),
    "c0 48 c1 4": (Case(1, 8, 32, 48, 32, c1=4, **Q), "sp"),
    "no second source": (Case(2, 12, 40, 48, 32, **Q), "dual"),
    "partial output block": (Case(2, 12, 40, 64, 20, c1=32, **Q), "dual"),
    "partial block, pos": (Case(1, 8, 32, 16, 20, c1=16, sign="pos", **Q), "nhwc"),
    "ReLU off": (Case(2, 12, 40, 64, 32, c1=32, relu=False, **Q), "dual"),
    "ReLU off, pos": (Case(2, 12, 40, 48, 20, c1=16, relu=False, sign="pos", **Q), "dual"),
    # 33 x 8 x 4 = 1056 tiles on 512 resident workgroups: two or three tiles per workgroup
    "persistent": (Case(33, 64, 128, 16, 32, c1=4, seed=1, **Q), "dual"),
}


class _Layer:
    """the device operands of one case, packed once"""
    def __init__(self, case):
        from disconet_amd import ops
        c, m = case, C.make(case)
        self.case = c
        self.src0 = ops.SpTensor.from_nhwc(m.x0.permute(0, 2, 3, 1).contiguous().cuda())
        self.src1 = ops.SpTensor.from_nhwc(m.x1.permute(0, 2, 3, 1).contiguous().cuda()) if c.c1 else None
        self.d = ops.conv_desc(c.n, c.h, c.w, c.c0, c.c_out, 3, 1, c.relu, c1=c.c1, up0=True, math="sp")
        self.packed, wmul = ops.sp_pack_conv_weights(self.d, m.w1.cuda())
        assert wmul == m.wmul1
        self.sc, self.sh = (m.scale1 / wmul).cuda(), m.shift1.cuda()

    def buffers(self, epi):
        """-> (SP output or None, fp32 rows inside a wider tensor or None), every byte 0xFF"""
        from disconet_amd import ops
        c = self.case
        out = wide = None
        if epi != "nhwc":
            out = ops.SpTensor(c.n, c.h, c.w, c.c_out, device="cuda")
            out.data.view(torch.int16).fill_(-1)
        if epi != "sp":
            wide = torch.empty(c.n, c.h, c.w, c.c_out + 8, dtype=torch.float32, device="cuda")
            wide.view(torch.int32).fill_(-1)
        return out, wide

    def launch(self, epi, out, wide, kslices=1):
        from disconet_amd import ops, _lib
        lib, ptr, st, d = _lib.load(), ops._ptr, ops._stream, ctypes.byref(self.d)
        p1 = ptr(self.src1.data) if self.src1 is not None else None
        args = (ptr(self.src0.data), p1, ptr(self.packed), ptr(self.sc), ptr(self.sh))
        rows = wide[..., 4:4 + self.case.c_out] if wide is not None else None
        if kslices > 1:
            ops.check(lib.dn_spconv2d_ks(d, kslices, *args, ptr(out.data), None, 0, None, 0, st()), "dn_spconv2d_ks")
        elif epi == "sp":
            ops.check(lib.dn_spconv2d(d, *args, ptr(out.data), st()), "dn_spconv2d")
        elif epi == "dual":
            ops.check(lib.dn_spconv2d_dual(d, *args, ptr(out.data), ptr(rows), wide.stride(2), st()), "dn_spconv2d_dual")
        else:
            ops.check(lib.dn_spconv2d_nhwc(d, *args, ptr(rows), wide.stride(2), st()), "dn_spconv2d_nhwc")


def _forced(layer, epi, force):
    """one launch under a forced form -> (SP output, wide rows tensor, resident?, form, range flags)"""
    from disconet_amd import ops, _lib
    lib = _lib.load()
    out, wide = layer.buffers(epi)
    ops.sp_range_flags(reset=True)
    lib.dn_spconv_force_config(force)
    try:
        layer.launch(epi, out, wide)
    finally:
        lib.dn_spconv_force_config(-1)
    torch.cuda.synchronize()
    return out, wide, ops.sp_last_resident(), ops.sp_last_form(), ops.sp_range_flags(reset=True)


def _nchw(t):
    return t.detach().cpu().permute(0, 3, 1, 2).double()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_resident_equals_streaming_and_fp64(name):
    case, epi = CASES[name]
    layer = _Layer(case)
    ref = C.reference(case)
    out_r, wide_r, res_r, form_r, flags_r = _forced(layer, epi, FORCE_RESIDENT)
    out_s, wide_s, res_s, form_s, flags_s = _forced(layer, epi, FORCE_STREAM)
    assert res_r is True and res_s is False, (res_r, res_s)
    for form in (form_r, form_s):
        assert (form["family"], form["TH"], form["TW"], form["BN"], form["DEEP"], form["KSL"]) == (1, 8, 32, 32, 0, 0), form
    assert form_r["grid"] == form_s["grid"] and form_r["total_items"] == form_s["total_items"]
    if name == "persistent":
        assert form_r["total_items"] == 1056 and form_r["total_items"] > 2 * form_r["grid"], form_r
    assert not (flags_r & 5) and not (flags_s & 5), (flags_r, flags_s)
    c = case.c_out
    if out_r is not None:
        assert torch.equal(out_r.data.view(torch.int16), out_s.data.view(torch.int16)), "SP output differs from the streaming form"
        r = C.worst(_nchw(out_r.nhwc()), ref, C.c_of(case, False))
        print("RESIDENT %-24s SP   err / (c A) = %.3f" % (name, r))
        assert r <= 1.0, r
    if wide_r is not None:
        assert torch.equal(wide_r.view(torch.int32), wide_s.view(torch.int32)), "fp32 rows differ from the streaming form"
        b = wide_r.view(torch.int32)
        assert bool((b[..., :4] == -1).all()) and bool((b[..., 4 + c:] == -1).all()), "the rows' neighbours were written"
        r = C.worst(_nchw(wide_r[..., 4:4 + c]), ref, C.c_of(case, True))
        print("RESIDENT %-24s fp32 err / (c A) = %.3f" % (name, r))
        assert r <= 1.0, r


# 9 x 8 x 4 = 288 tiles: more work items than CUs (below that the one-step-per-chunk form takes the launch)
@pytest.mark.gpu
@pytest.mark.parametrize("what,case,kslices,resident", [
    ("4 + 2 chunks", Case(9, 64, 128, 64, 32, c1=32, **Q), 1, True),
    ("short K, c_out 20", Case(9, 64, 128, 16, 20, c1=4, **Q), 1, True),
    ("c0 = 80: five chunks", Case(9, 64, 128, 80, 32, c1=32, **Q), 1, False),
    ("c1 = 48: three chunks", Case(9, 64, 128, 64, 32, c1=48, **Q), 1, False),
    ("c_out = 64: two channel blocks", Case(9, 64, 128, 64, 64, c1=32, **Q), 1, False),
    ("K slices", Case(9, 64, 128, 64, 32, c1=32, **Q), 2, False),
    ("<= 256 work items", Case(2, 64, 128, 64, 32, c1=32, **Q), 1, False),
])
def test_dispatch_takes_the_resident_form_by_shape(what, case, kslices, resident):
    from disconet_amd import ops, _lib
    _lib.load().dn_spconv_force_config(-1)
    layer = _Layer(case)
    out, wide = layer.buffers("sp")
    layer.launch("sp", out, wide, kslices)
    torch.cuda.synchronize()
    form = ops.sp_last_form()
    assert form["family"] == 1, form
    assert ops.sp_last_resident() is resident, (what, form)
    if resident:
        assert (form["BN"], form["DEEP"], form["KSL"]) == (32, 0, 0), form


@pytest.mark.gpu
def test_graph_replay_equals_eager():
    from disconet_amd import _lib
    lib = _lib.load()
    case, epi = CASES["persistent"]
    layer = _Layer(case)
    eager_out, eager_wide, res, _, _ = _forced(layer, epi, FORCE_RESIDENT)
    assert res is True
    out, wide = layer.buffers(epi)
    lib.dn_spconv_force_config(FORCE_RESIDENT)
    try:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            layer.launch(epi, out, wide)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            layer.launch(epi, out, wide)
    finally:
        lib.dn_spconv_force_config(-1)
    out.data.view(torch.int16).fill_(-1)
    wide.view(torch.int32).fill_(-1)
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.data.view(torch.int16), eager_out.data.view(torch.int16))
    assert torch.equal(wide.view(torch.int32), eager_wide.view(torch.int32))
