"""tests/conv_fp64.py on the CPU: the float64 reference against torch's own float64 ops, the SP split, and -- what makes the
GPU file worth running -- the faithful emulation of the engine's arithmetic INSIDE the bound and every mutant of it OUTSIDE,
on every case family.  No GPU."""
import pytest
import torch
import torch.nn.functional as F

from tests import conv_fp64 as C

FAMS = sorted(C.FAMILIES)
TW = 8           # the narrowest pixel tile of the engine: the 12 x 20 maps of the families have two tile edges inside


def _exact_stage(w, scale, shift, relu, stride=1):
    """a Stage of unrounded float64 operands (lo = 0, no lift)"""
    return C.Stage(w.unsqueeze(0), torch.zeros_like(w).unsqueeze(0), scale, shift, relu, stride)


@pytest.mark.parametrize("stride,k,up0,c1,relu", [(1, 3, False, 0, True), (2, 3, False, 0, False), (1, 1, False, 0, True),
                                                  (1, 3, True, 5, True), (1, 3, False, 7, False)])
def test_conv64_is_torch_float64(stride, k, up0, c1, relu):
    """on unrounded operands conv64 IS conv2d / interpolate / cat / relu of torch in float64, bit for bit, and A is the
    same conv of the absolute values"""
    g = torch.Generator().manual_seed(5)
    n, h, w, c0, co = 2, 10, 14, 6, 9
    h0, w0 = (h // 2, w // 2) if up0 else (h, w)
    x0 = torch.randn(n, c0, h0, w0, generator=g, dtype=torch.float64)
    x1 = torch.randn(n, c1, h, w, generator=g, dtype=torch.float64) if c1 else None
    wt = torch.randn(co, c0 + c1, k, k, generator=g, dtype=torch.float64)
    sc, sh = torch.randn(co, generator=g, dtype=torch.float64), torch.randn(co, generator=g, dtype=torch.float64)
    z = lambda t: None if t is None else torch.zeros_like(t)
    ref = C.conv64(C.Operands(x0, z(x0), x1, z(x1), up0, _exact_stage(wt, sc, sh, relu, stride)))
    xin = F.interpolate(x0, scale_factor=(2, 2), mode="nearest") if up0 else x0
    if c1:
        xin = torch.cat((xin, x1), 1)
    want = F.conv2d(xin, wt, None, stride=stride, padding=k // 2) * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1)
    want_a = F.conv2d(xin.abs(), wt.abs(), None, stride=stride, padding=k // 2) * sc.abs().view(1, -1, 1, 1) + sh.abs().view(1, -1, 1, 1)
    assert torch.equal(ref.y, F.relu(want) if relu else want)
    assert torch.equal(ref.A, want_a)
    assert bool((ref.y.abs() <= ref.A * (1 + 1e-12)).all())


def test_conv64_second_stage_reads_the_sp_pair():
    """the fused 1x1 stage: the two torch ops with the hidden map rounded to its SP pair in between (conv_sp.hip splits the
    stage-1 tile before the 1x1 MFMAs), A carried through |w2|"""
    g = torch.Generator().manual_seed(6)
    x = torch.randn(1, 5, 6, 7, generator=g, dtype=torch.float64)
    w1 = torch.randn(8, 5, 3, 3, generator=g, dtype=torch.float64)
    w2 = torch.randn(3, 8, 1, 1, generator=g, dtype=torch.float64)
    one, zero = torch.ones(8, dtype=torch.float64), torch.zeros(8, dtype=torch.float64)
    op = C.Operands(x, torch.zeros_like(x), None, None, False, _exact_stage(w1, one, zero, True),
                    _exact_stage(w2, one[:3], zero[:3], False))
    ref = C.conv64(op)
    mid = F.relu(F.conv2d(x, w1, None, padding=1))
    assert torch.equal(ref.y, F.conv2d(C.sp_value(mid.float()), w2))
    assert torch.equal(ref.A, F.conv2d(F.conv2d(x.abs(), w1.abs(), None, padding=1), w2.abs()))
    assert not torch.equal(ref.y, F.conv2d(mid, w2))


def test_merged_tap_classes_are_the_plain_conv():
    """the class kernels of the tap-merged images: with weights whose sums are exact (small integers) the quad- and
    row-merged forms equal the plain 3x3 conv on the upsampled map, borders included"""
    g = torch.Generator().manual_seed(7)
    c0, c1, co = 16, 3, 5
    wt = torch.randint(-3, 4, (co, c0 + c1, 3, 3), generator=g).float()
    x0 = torch.randn(2, c0, 4, 6, generator=g).half().double()
    x1 = torch.randn(2, c1, 8, 12, generator=g).half().double()
    xin = torch.cat((F.interpolate(x0, scale_factor=(2, 2)), x1), 1)
    want = F.conv2d(xin, wt.double(), None, padding=1)
    for merge in ("quad", "rows"):
        hi, lo = C.packed_weights(wt, 1.0, merge, c0)
        assert hi.shape[0] == 4 and not bool(lo.any())
        st = C.Stage(hi, lo, torch.ones(co, dtype=torch.float64), torch.zeros(co, dtype=torch.float64), False)
        got = C.conv64(C.Operands(x0, torch.zeros_like(x0), x1, torch.zeros_like(x1), True, st)).y
        assert torch.equal(got, want), merge


def test_sp_split_round_trip_and_residual():
    g = torch.Generator().manual_seed(8)
    # exact in 22 bits: an 11-bit hi of binade e and a lo = k 2^(e - 21), |k| < 1024 (below half an ulp of hi)
    hi = torch.randn(4096, generator=g).half().double()
    hi = hi[hi.abs() >= 0.125]
    e = torch.frexp(hi)[1].double() - 1
    lo = torch.randint(-1023, 1024, hi.shape, generator=g).double() * 2.0 ** (e - 21)
    x = hi + lo
    assert torch.equal(C.sp_value(x), x)
    # any fp32 value above the f16 subnormal range: the residual is below 2^-22 |x|
    v = (torch.randn(1 << 16, generator=g) * torch.tensor(2.0) ** torch.randint(-2, 14, (1 << 16,), generator=g)).float()
    v = v[(v.abs() >= 2.0 ** -2) & (v.abs() <= 60000.0)]
    res = (C.sp_value(v) - v.double()).abs()
    assert bool((res <= C.P22 * v.double().abs()).all()), float((res / v.double().abs()).max())
    # the clamp, and the split of the lifted weights
    assert float(C.sp_value(torch.tensor([1e6, -1e6]))[0]) == C.F16_MAX
    w = torch.randn(64, 32, 3, 3, generator=g) * 0.01
    m = C.pow2_lift(w)
    assert 4096.0 <= float(w.abs().max()) * m < 8192.0
    wh, wl = C.packed_weights(w, m)
    assert float(((wh + wl)[0] - (w * m).double()).abs().max()) <= C.P22 * 8192.0


@pytest.mark.parametrize("family", FAMS)
def test_operands_carry_full_pairs(family):
    for case in C.FAMILIES[family]:
        assert C.lo_fraction(case) > 0.9, (case, C.lo_fraction(case))


@pytest.mark.parametrize("family", FAMS)
def test_recorded_c32_reproduces(family):
    got = C.measure_c32(family)
    print("c32 %s: measured %.3e, recorded %.3e" % (family, got, C.C32[family]))
    assert C.C32[family] / 2 <= got <= C.C32[family] * 2, (got, C.C32[family])


@pytest.mark.parametrize("family", sorted(C.E32))
def test_recorded_e32_reproduces(family):
    """the own yardstick of the un-sliced long-K chain (conv_fp64.E32): the faithful emulation's distance from float64
    reproduces, exceeds the family's c32 (else it would not be needed) and the K-sliced chain does not need it"""
    got = C.measure_e32(family)
    print("e32 %s: measured %.3e, recorded %.3e" % (family, got, C.E32[family]))
    assert C.E32[family] / 2 <= got <= C.E32[family] * 2, (got, C.E32[family])
    assert C.E32[family] > C.C32[family]
    for case in C.FAMILIES[family]:
        r = C.worst(C.engine32(C.make(case).op, kslices=4), C.reference(case), C.c_of(case, kslices=4))
        assert C.c_of(case, kslices=4) < C.c_of(case) and r <= 1.0, r


def _emulate(case, mutant=None, **kw):
    return C.engine32(C.make(case).op, mutant, tw=TW, spq=case.merge == "quad", **kw)


@pytest.mark.parametrize("family", FAMS)
def test_faithful_engine_passes_the_bound(family):
    """the engine's arithmetic as designed -- three products, fp32 accumulation in its order, fp32 affine, SP output --
    sits inside c A on every family, with the margin printed (-s); so does the fp32 output under its tighter constant"""
    for case in C.FAMILIES[family]:
        ref = C.reference(case)
        r = C.worst(_emulate(case), ref, C.c_of(case))
        r32 = C.worst(_emulate(case, out_f32=True), ref, C.c_of(case, out_f32=True))
        print("%s %s: err / (c A) = %.3f (SP), %.3f (fp32 out)" % (family, case, r, r32))
        assert r <= 1.0 and r32 <= 1.0, (case, r, r32)


@pytest.mark.parametrize("kslices,spq", [(2, False), (4, False), (2, True), (4, True)])
def test_k_sliced_engine_passes_the_bound(kslices, spq):
    """the slices' accumulators summed in slice order (conv_sp.hip's equal chunk shares, conv_spq.hip's equal work shares)"""
    assert C.ks_bounds(5, 4) == [0, 1, 2, 3, 5] and C.ks_bounds(6, 4) == [0, 1, 3, 4, 6] and C.ks_bounds(3, 2) == [0, 1, 3]
    assert C.ks_bounds(5, 4, c0g=3) == [0, 2, 3, 4, 5]
    case = C.Case(1, 12, 20, 48, 32, c1=44, up0=True, merge="quad", sign="pos") if spq else C.Case(1, 12, 20, 80, 64, sign="pos")
    r = C.worst(_emulate(case, kslices=kslices), C.reference(case), C.c_of(case))
    assert r <= 1.0, r


@pytest.mark.parametrize("mutant", C.MUTANTS)
@pytest.mark.parametrize("family", FAMS)
def test_every_mutant_fails_the_bound(family, mutant):
    """a kernel that loses a cross product, writes a zero lo half, reads one tap a pixel off at a tile edge or loses an
    octet of the last chunk is OUTSIDE c A on every case of every family meant to catch it -- the geometric ones by
    more than 100 x"""
    if mutant in C.NOT_MEANT.get(family, ()):
        # a hi-only source has no x_lo product: the mutant is the faithful engine, and must pass like it
        for case in C.FAMILIES[family]:
            assert torch.equal(_emulate(case, mutant), _emulate(case))
        return
    for case in C.FAMILIES[family]:
        r = C.worst(_emulate(case, mutant), C.reference(case), C.c_of(case))
        print("%s %s %s: err / (c A) = %.3g" % (family, mutant, case, r))
        assert r > (100.0 if mutant in C.GEOMETRIC else 1.0), (case, mutant, r)
