"""tests/nhwc_conv_fp64.py on the CPU: the float64 reference of the fp32-NHWC conv engine against torch's own float64 ops,
and -- what makes the GPU file worth running -- the faithful emulation of the engine's arithmetic INSIDE the bound and
every mutant of it OUTSIDE, on every case family, in both math modes.  No GPU."""
from functools import lru_cache

import pytest
import torch
import torch.nn.functional as F

from tests import conv_fp64 as C
from tests import nhwc_conv_fp64 as N
from tests.conv_fp64 import Case

FAMS = sorted(N.FAMILIES)
TWS = (8, 16, 32)       # the pixel tiles' widths


@lru_cache(maxsize=None)
def _faithful(layer):
    return N.engine(layer)          # the tile width only matters to tap_shift_edge


@pytest.mark.parametrize("math", [0, 1])
def test_reference_is_torch_float64_on_the_stored_operands(math):
    """y is conv2d / interpolate / cat / relu of torch in float64 on the operands as stored: the fp32 values (math 0), the
    clamped hi + lo of activations and of the UNLIFTED weights (math 1)"""
    layer = N.Layer(Case(2, 10, 14, 16, 9, c1=7, up0=True), math)
    m = C.make(layer.case)
    val = (lambda t: C.sp_value(t)) if math else (lambda t: t.double())
    xin = torch.cat((F.interpolate(val(m.x0), scale_factor=(2, 2), mode="nearest"), val(m.x1)), 1)
    want = F.conv2d(xin, val(m.w1), None, padding=1) * m.scale1.double().view(1, -1, 1, 1) + m.shift1.double().view(1, -1, 1, 1)
    want_a = F.conv2d(xin.abs(), val(m.w1).abs(), None, padding=1) * m.scale1.double().view(1, -1, 1, 1) + m.shift1.double().abs().view(1, -1, 1, 1)
    ref = N.reference(layer)
    assert torch.equal(ref.y, F.relu(want)) and torch.equal(ref.A, want_a)
    if math:
        # Kaiming-sized weights: nearly every lo half is an f16 subnormal (a multiple of 2^-24), and the pair differs from w
        wl = N.operands(layer).s1.wl
        assert float((wl.abs() < 2.0 ** -14).double().mean()) > 0.9 and torch.equal(wl, torch.round(wl * 2.0 ** 24) / 2.0 ** 24)
        assert not torch.equal(val(m.w1), m.w1.double())


def test_reference_zero_stuffed_source_and_tap_mask():
    """up0 = 2 is the conv of the zero-stuffed map; a tap mask is the conv with the other taps' weights zero -- in y and
    in A; the four parity masks hold 1, 2, 2 and 4 taps and together make the stride-2 data gradient's classes"""
    c = Case(1, 12, 20, 16, 8, up0=True, relu=False)
    m = C.make(c)
    ref = N.reference(N.Layer(c, 0, stuffed=True))
    z = torch.zeros(1, 16, 12, 20, dtype=torch.float64)
    z[:, :, ::2, ::2] = m.x0.double()
    aff = lambda t, sh: t * m.scale1.double().view(1, -1, 1, 1) + sh.view(1, -1, 1, 1)
    assert torch.equal(ref.y, aff(F.conv2d(z, m.w1.double(), None, padding=1), m.shift1.double()))
    assert sorted(bin(v).count("1") for v in N.PARITY_MASKS.values()) == [1, 2, 2, 4]
    c = Case(1, 12, 20, 16, 8, relu=False)
    m = C.make(c)
    for (py, px), mask in N.PARITY_MASKS.items():
        w = m.w1.double().clone()
        for t in range(9):
            if not (mask >> t) & 1:
                w[:, :, t // 3, t % 3] = 0.0
        assert {(t // 3, t % 3) for t in range(9) if (mask >> t) & 1} == {(ky, kx) for ky in ((1,), (1, 2))[py] for kx in ((1,), (1, 2))[px]}
        ref = N.reference(N.Layer(c, 0, tap_mask=mask))
        assert torch.equal(ref.y, aff(F.conv2d(m.x0.double(), w, None, padding=1), m.shift1.double()))
        assert torch.equal(ref.A, aff(F.conv2d(m.x0.double().abs(), w.abs(), None, padding=1), m.shift1.double().abs()).abs())


def test_chain0_order_is_the_kernels():
    """math 0: with operands whose products and sums are exact (small integers) the emulation is the conv itself, whatever
    the chunk size; and the pairs it adds are channels 8 s + t and 8 s + 4 + t of a chunk"""
    g = torch.Generator().manual_seed(3)
    x = torch.randint(-3, 4, (1, 21, 6, 9), generator=g).double()
    w = torch.randint(-3, 4, (5, 21, 3, 3), generator=g).double()
    s = C.Stage(w.unsqueeze(0), torch.zeros_like(w).unsqueeze(0), None, None, False)
    want = F.conv2d(x, w, None, padding=1)
    for kc in (8, 16):
        assert torch.equal(N._chain0(x, s, None, 32, kc).double(), want)


@pytest.mark.parametrize("family", FAMS)
def test_recorded_c32_reproduces(family):
    got = N.measure_c32(family)
    print("c32 %s: measured %.3e, recorded %.3e" % (family, got, N.C32[family]))
    assert N.C32[family] / 2 <= got <= N.C32[family] * 2, (got, N.C32[family])


@pytest.mark.parametrize("family", sorted(N.E32))
def test_recorded_e32_reproduces(family):
    """the long-K families' own yardstick: the faithful emulation's distance from float64 reproduces and exceeds the
    family's c32 (else it would not be needed); no other family has one"""
    got = N.measure_e32(family)
    print("e32 %s: measured %.3e, recorded %.3e" % (family, got, N.E32[family]))
    assert N.E32[family] / 2 <= got <= N.E32[family] * 2, (got, N.E32[family])
    assert N.E32[family] > N.C32[family] and "/longk/" in family


@pytest.mark.parametrize("family", FAMS)
def test_faithful_engine_passes_the_bound(family):
    """the engine's arithmetic as designed -- one fp32 accumulator over every chunk and tap in the kernel's order, two-product
    partials (math 0) or the three split products (math 1), the fp32 affine -- sits inside c A on every family"""
    for layer in N.FAMILIES[family]:
        r = N.worst(_faithful(layer), N.reference(layer), N.c_of(layer))
        print("%s %s: err / (c A) = %.3f" % (family, layer, r))
        assert r <= 1.0, (layer, r)


@pytest.mark.parametrize("mutant", N.MUTANTS)
@pytest.mark.parametrize("family", FAMS)
def test_every_mutant_fails_the_bound(family, mutant):
    """a kernel that loses a cross product, reads a tap a pixel off at the edge of an 8-, 16- or 32-wide tile, loses the last
    octet, multiplies a masked tap, reads the zero-stuffed source as an upsampled one or lets the next pixel's channels
    into a 13-channel source's last quad is OUTSIDE c A on every launch it can change -- the geometric ones by more than
    10 x -- and IS the faithful engine on the launches it cannot (nhwc_conv_fp64.not_meant says why)"""
    tried = 0
    for layer in N.FAMILIES[family]:
        ref, c = N.reference(layer), N.c_of(layer)
        for tw in (TWS if mutant == "tap_shift_edge" else (32,)):
            why = N.not_meant(mutant, layer, tw)
            if why is not None:
                assert torch.equal(N.engine(layer, mutant, tw), _faithful(layer)), (layer, mutant, why)
                continue
            r = N.worst(N.engine(layer, mutant, tw), ref, c)
            print("%s %s tw %d %s: err / (c A) = %.3g" % (family, mutant, tw, layer, r))
            assert r > (10.0 if mutant in N.GEOMETRIC else 1.0), (layer, mutant, tw, r)
            tried += 1
    print("%s %s: %d launches" % (family, mutant, tried))


def test_every_mutant_is_caught_somewhere():
    """no mutant is exempt everywhere: each meets a launch it can change in at least one family of each math mode it
    exists in, and tap_shift_edge at every tile width"""
    for mutant in N.MUTANTS:
        for math in (0, 1):
            if mutant in ("drop_xhi_wlo", "drop_xlo_whi") and math == 0:
                continue
            for tw in (TWS if mutant == "tap_shift_edge" else (32,)):
                assert any(N.not_meant(mutant, layer, tw) is None for fam in FAMS for layer in N.FAMILIES[fam] if layer.math == math), \
                    (mutant, math, tw)
