"""A float64 reference of the fp32-NHWC conv engine (disconet_amd/csrc/conv_mfma.hip: dn_conv2d, dn_conv2d_taps,
dn_conv2d_post1x1), a CPU emulation of the engine's own arithmetic with switches that break it on purpose, and the bound
that separates the two.  Plain torch on the CPU, no GPU import; everything the SP engine's file already has (the split,
the bound's arithmetic, Case and its seeded tensors, the split-f16 chain) is imported from tests/conv_fp64.py.  TEST
infrastructure: tests/test_nhwc_conv_fp64_cpu.py shows on the CPU that the faithful emulation passes the bound and that
every mutant fails it; tests/test_gpu_nhwc_conv_fp64.py holds every tile form of the engine to the same bound.

Operands as stored.  math 0 (exact fp32): x and w are the fp32 values themselves.  math 1 (split-f16): x is clamped to
+-65504 and split hi = half(x), lo = half(x - hi) while it is staged (store_chunk); w is clamped and split at pack time
WITH NO LIFT (dn_conv_pack_weights takes w as given), so for Kaiming-sized weights the lo half is an f16 subnormal
and carries fewer bits -- torch's .half() rounds the same way, and the reference is computed on hi + lo of both.

The layer.  y = float64 conv on those operands, * scale + shift, ReLU.  up0 = 1: source 0 nearest-upsampled x2;
up0 = 2 (Layer.stuffed): source 0 zero-stuffed, its values on even (iy, ix) only; tap_mask: an unselected tap contributes
nothing to y or to A.  The fused 1x1 stage reads the hi/lo pair of the clamped fp32 stage-1 value (the epilogue of
conv_mfma_kernel) and A is carried through |w2~|, exactly as conv_fp64.conv64 does it.

The bound.  |got - y| <= c A per element, A = |scale| (|x~| conv |w~|) + |shift|; an element with A = 0 must be exact.
c = 4 yard (math 0), 4 yard + 2^-22 (math 1: the dropped lo x lo product), + another 2^-22 for the fused stage.  yard is
C32 of the layer's family -- what torch's float32 CPU conv loses against y on the same operands, measured here with
`python -m tests.nhwc_conv_fp64` -- and 4 is conv_fp64.MARGIN.  The long-K families have a yardstick of their own where the
faithful emulation of the engine's chain exceeds c32, for a stated reason: E32 below."""
from dataclasses import dataclass, replace
from functools import lru_cache

import torch
import torch.nn.functional as F

from tests import conv_fp64 as C
from tests.conv_fp64 import (Case, MARGIN, Operands, P22, Stage, _chain, _view, assemble, conv64, engine32,  # noqa: F401
                             sp_split, torch32, worst)

FULL = 0x1ff
# the tap masks of the parity-phase stride-2 data gradient (dn_conv_dgrad_class_weights): class (py, px) -> bits ky * 3 + kx
PARITY_MASKS = {(0, 0): 0x010, (0, 1): 0x030, (1, 0): 0x090, (1, 1): 0x1b0}


@dataclass(frozen=True)
class Layer:
    """one launch of the engine: the layer (conv_fp64.Case; up0 = True: source 0 is h/2 x w/2), the math mode, whether
    source 0 is read zero-stuffed (up0 = 2) instead of nearest-upsampled, and the tap mask (dn_conv2d_taps)"""
    case: Case
    math: int
    stuffed: bool = False
    tap_mask: int = FULL

    def __post_init__(self):
        assert self.math in (0, 1) and 0 < self.tap_mask <= FULL
        assert not self.stuffed or self.case.up0
        assert not self.case.post or self.math == 1
        assert self.case.src == "sp" and not self.case.merge and not self.case.stem


# --- operands as stored -------------------------------------------------------------------------
def _pair(v, math):
    """fp32 values -> (hi, lo) float64 as the engine holds them"""
    if math == 1:
        return sp_split(v)
    d = v.float().double()
    return d, torch.zeros_like(d)


def stuff(x):
    """[n, c, h, w] -> [n, c, 2h, 2w]: the values on even (iy, ix), zero elsewhere"""
    out = x.new_zeros(x.shape[0], x.shape[1], 2 * x.shape[2], 2 * x.shape[3])
    out[:, :, ::2, ::2] = x
    return out


def _masked(w, mask):
    w = w.clone()
    for t in range(9):
        if w.shape[-1] == 3 and not (mask >> t) & 1:
            w[..., t // 3, t % 3] = 0.0
    return w


def _operands(layer, tap_mask=None, stuffed=None):
    c, m = layer.case, C.make(layer.case)
    tap_mask = layer.tap_mask if tap_mask is None else tap_mask
    stuffed = layer.stuffed if stuffed is None else stuffed
    x0h, x0l = _pair(m.x0, layer.math)
    up0 = bool(c.up0)
    if stuffed:
        x0h, x0l, up0 = stuff(x0h), stuff(x0l), False
    x1h, x1l = _pair(m.x1, layer.math) if c.c1 else (None, None)
    wh, wl = _pair(m.w1, layer.math)
    s1 = Stage(_masked(wh, tap_mask).unsqueeze(0), _masked(wl, tap_mask).unsqueeze(0), m.scale1.double(), m.shift1.double(),
               c.relu, c.stride)
    s2 = None
    if c.post:
        w2h, w2l = _pair(m.w2, 1)
        s2 = Stage(w2h.unsqueeze(0), w2l.unsqueeze(0), m.scale2.double(), m.shift2.double(), bool(c.post[2]))
    return Operands(x0h, x0l, x1h, x1l, up0, s1, s2, False)


@lru_cache(maxsize=None)
def operands(layer):
    return _operands(layer)


@lru_cache(maxsize=None)
def reference(layer):
    """-> conv_fp64.Ref(y, A) of the layer, float64 on the operands as stored"""
    return conv64(operands(layer))


# --- the engine's arithmetic, and ways to get it wrong ------------------------------------------------
# from conv_fp64: drop_xhi_wlo / drop_xlo_whi (math 1: a lost cross product), tap_shift_edge (the middle row's right tap one
# pixel further in the last column of every tw-wide tile), drop_octet (the last populated 8 channels lost).  New here:
# masked_tap_multiplied (one zero bit of tap_mask ignored), stuffed_parity_ignored (up0 = 2 read like up0 = 1),
# tail_quad_next_pixel (the dword path of a source whose c0 is no multiple of 4: the channels that fill its last quad
# are the next pixel's first ones, and meet a NON-zero weight -- the weights of the channels they really are).
MUTANTS = ("drop_xhi_wlo", "drop_xlo_whi", "tap_shift_edge", "drop_octet", "masked_tap_multiplied", "stuffed_parity_ignored",
           "tail_quad_next_pixel")
GEOMETRIC = ("tap_shift_edge", "drop_octet", "masked_tap_multiplied", "stuffed_parity_ignored", "tail_quad_next_pixel")


def not_meant(mutant, layer, tw):
    """why `mutant` cannot change this launch (None: it can, and must then fail the bound) -- the exemptions, as
    conv_fp64.NOT_MEANT writes them down"""
    c = layer.case
    wo = (c.w + 2 * (c.k // 2) - c.k) // c.stride + 1
    if mutant in ("drop_xhi_wlo", "drop_xlo_whi") and layer.math == 0:
        return "exact fp32 has no cross products"
    if mutant == "tap_shift_edge" and wo <= tw:
        return "no tile ends inside the map: right of its last column the tap and the shifted tap both read padding"
    if mutant == "tap_shift_edge" and c.k == 3 and not (layer.tap_mask >> 5) & 1:
        return "the shifted tap is masked out"
    if mutant == "masked_tap_multiplied" and (c.k != 3 or layer.tap_mask == FULL):
        return "every tap is selected"
    if mutant == "stuffed_parity_ignored" and not layer.stuffed:
        return "source 0 is not zero-stuffed"
    if mutant == "tail_quad_next_pixel" and (c.c0 % 4 == 0 or c.c1 or c.up0):
        return "the source's last quad is whole"
    return None


def kc_of(layer):
    """channels per chunk of the instantiations the dispatch holds: 16 for 3x3 (8 for stride 2 in fp32), 32 for 1x1"""
    c = layer.case
    return 32 if c.k == 1 else (8 if c.stride == 2 and layer.math == 0 else 16)


def _chain0(x, s, mutant, tw, kc):
    """math 0: ONE fp32 accumulator per output over all chunks and taps, never K-sliced.  v_mfma_f32_32x32x2_f32 adds
    a partial of 2 products per instruction; a lane reads k = 8 s + 4 h + {0..3} of the chunk, so instruction t of step s
    holds channels 8 s + t and 8 s + 4 + t.  Order: chunk (kc channels), tap, s, t."""
    n, cin, h, w = x.shape
    k = s.wh.shape[-1]
    pad, st = k // 2, s.stride
    ho, wo = (h + 2 * pad - k) // st + 1, (w + 2 * pad - k) // st + 1
    wt = s.wh[0]
    if mutant == "drop_octet":
        x = x.clone()
        x[:, 8 * ((cin - 1) // 8):] = 0.0
    xp = F.pad(x, (pad, pad + 1, pad, pad))
    edge = (torch.arange(wo) % tw == tw - 1).view(1, 1, 1, -1)

    def tap(cs, ty, tx, shift=0):
        return xp[:, cs, ty:ty + st * (ho - 1) + 1:st, tx + shift:tx + shift + st * (wo - 1) + 1:st]

    acc = torch.zeros(n, wt.shape[0], ho, wo, dtype=torch.float32)
    for g in range((cin + kc - 1) // kc):
        for ty in range(k):
            for tx in range(k):
                if not bool(wt[:, kc * g:kc * g + kc, ty, tx].any()):
                    continue                              # a masked tap: nothing is issued
                for s8 in range(kc // 8):
                    for t in range(4):
                        cs = [ch for ch in (kc * g + 8 * s8 + t, kc * g + 8 * s8 + 4 + t) if ch < cin]
                        if not cs:
                            continue                      # past the layer's channels: zero weights
                        v = tap(cs, ty, tx)
                        if mutant == "tap_shift_edge" and ty == pad and tx == k - 1:
                            v = torch.where(edge, tap(cs, ty, tx, 1), v)
                        acc = (acc.double() + torch.einsum("oc,nchw->nohw", wt[:, cs, ty, tx], v)).float()
    return acc


def engine(layer, mutant=None, tw=32):
    """A CPU emulation of the engine -> float64 [n, c, h, w].  math 1 is conv_fp64.engine32 with one K slice, no lift and
    an fp32 output (chunks of 16, per tap w_lo x_hi, w_hi x_lo, w_hi x_hi); math 0 is _chain0, the fp32 fma of the affine,
    ReLU."""
    assert mutant is None or mutant in MUTANTS
    mask, stuffed = layer.tap_mask, layer.stuffed
    if mutant == "masked_tap_multiplied" and mask != FULL:
        mask |= [1 << t for t in range(9) if not (mask >> t) & 1][0]
    if mutant == "stuffed_parity_ignored":
        stuffed = False
    op = _operands(layer, mask, stuffed)
    if mutant == "tail_quad_next_pixel" and not_meant(mutant, layer, tw) is None:
        # NHWC, one image: the dwords after a pixel's c0 channels are the next pixel's channels 0 .. (zero past the image)
        nx = 4 - layer.case.c0 % 4
        def nxt(t):
            n, c, h, w = t.shape
            flat = F.pad(t[:, :nx].reshape(n, nx, h * w), (0, 1))[:, :, 1:]
            return torch.cat((t, flat.reshape(n, nx, h, w)), 1)
        s = op.s1
        op = replace(op, x0h=nxt(op.x0h), x0l=nxt(op.x0l),
                     s1=replace(s, wh=torch.cat((s.wh, s.wh[:, :, :nx]), 2), wl=torch.cat((s.wl, s.wl[:, :, :nx]), 2)))
    inner = mutant if mutant in C.MUTANTS else None
    if layer.math == 1:
        return engine32(op, inner, tw=tw, out_f32=True)
    s = op.s1
    x = assemble(op.x0h, op.x1h, op.up0)
    acc = _chain0(x, s, inner, tw, kc_of(layer))
    v = (acc.double() * _view(s.scale) + _view(s.shift)).float()            # one rounding: the epilogue's fma
    return (v.clamp(min=0.0) if s.relu else v).double()


# --- case families ------------------------------------------------------------------------------------
def family_of(layer):
    c = layer.case
    if c.post:
        kind = "post"
    elif c.c0 + c.c1 >= 512:
        kind = "longk"
    elif layer.stuffed:
        kind = "stuffed"
    elif layer.tap_mask != FULL:
        kind = "taps"
    elif c.up0:
        kind = "up"
    elif c.k == 1:
        kind = "s1"
    elif c.stride == 2:
        kind = "s3s2"
    else:
        kind = "s3"
    return "m%d/%s/%s" % (layer.math, kind, c.sign)


_UP = dict(up0=True)
_KINDS = {
    # 36 wide: the last column of an 8-, a 16- and a 32-pixel tile is inside the map; 13 channels: the dword path
    "s3": [(Case(1, 12, 36, 16, 32), {}), (Case(1, 12, 20, 80, 64), {}), (Case(1, 12, 20, 13, 32), {})],
    "s3s2": [(Case(1, 13, 21, 44, 64, stride=2), {})],
    "s1": [(Case(1, 12, 36, 128, 64, k=1), {}), (Case(1, 12, 20, 48, 12, k=1, relu=False), {})],
    "up": [(Case(1, 12, 36, 48, 32, c1=44, **_UP), {}), (Case(1, 12, 20, 16, 32, c1=12, **_UP), {})],
    "stuffed": [(Case(1, 12, 36, 16, 32, relu=False, **_UP), dict(stuffed=True)),
                (Case(1, 14, 22, 48, 12, relu=False, **_UP), dict(stuffed=True))],
    "taps": [(Case(1, 12, 36, 16, 32, relu=False), dict(tap_mask=m)) for m in PARITY_MASKS.values()],
    "post": [(Case(1, 12, 36, 44, 64, post=(48, 48, False, False)), {}), (Case(1, 12, 20, 16, 64, post=(48, 12, False, True)), {})],
    # conv5_1's K: 512 upsampled + 256 -> 32
    "longk": [(Case(1, 8, 8, 512, 32, c1=256, **_UP), {})],
}
FAMILIES = {}
for _kind, _cases in _KINDS.items():
    for _math in (0, 1):
        if _kind == "post" and _math == 0:
            continue                                      # the fused stage is split-f16 only
        for _sign in ("randn", "pos"):
            FAMILIES["m%d/%s/%s" % (_math, _kind, _sign)] = [Layer(replace(c, sign=_sign), _math, **kw) for c, kw in _cases]
for _fam, _layers in FAMILIES.items():
    assert all(family_of(l) == _fam for l in _layers), _fam


def measure_c32(family):
    """max over the family's layers and outputs of |conv_float32(x~, w~) - y| / A"""
    return max(worst(torch32(operands(l)), reference(l), 1.0) for l in FAMILIES[family])


def measure_e32(family):
    """the same distance for the faithful emulation of the engine's own chain"""
    return max(worst(engine(l), reference(l), 1.0) for l in FAMILIES[family])


# Measured with `python -m tests.nhwc_conv_fp64` (torch CPU float32 conv against conv64 on the operands as stored; the
# figure moves a little with torch's conv algorithm and thread count: tests/test_nhwc_conv_fp64_cpu.py fails at a factor 2).
C32 = {
    "m0/s3/randn": 2.232e-07, "m0/s3/pos": 8.379e-07, "m1/s3/randn": 2.362e-07, "m1/s3/pos": 8.390e-07,
    "m0/s3s2/randn": 1.113e-07, "m0/s3s2/pos": 6.139e-07, "m1/s3s2/randn": 9.645e-08, "m1/s3s2/pos": 5.710e-07,
    "m0/s1/randn": 1.982e-07, "m0/s1/pos": 4.525e-07, "m1/s1/randn": 1.995e-07, "m1/s1/pos": 4.531e-07,
    "m0/up/randn": 1.957e-07, "m0/up/pos": 1.033e-06, "m1/up/randn": 2.201e-07, "m1/up/pos": 9.164e-07,
    "m0/stuffed/randn": 2.325e-07, "m0/stuffed/pos": 5.296e-07, "m1/stuffed/randn": 2.116e-07, "m1/stuffed/pos": 4.746e-07,
    "m0/taps/randn": 2.184e-07, "m0/taps/pos": 5.235e-07, "m1/taps/randn": 2.129e-07, "m1/taps/pos": 4.860e-07,
    "m1/post/randn": 3.129e-08, "m1/post/pos": 5.200e-07,
    "m0/longk/randn": 2.078e-08, "m0/longk/pos": 4.170e-07, "m1/longk/randn": 1.772e-08, "m1/longk/pos": 3.842e-07,
}

# The long-K layer (768 input channels, 3x3) takes the emulation's own distance from float64 as its yardstick where
# that exceeds c32.  Reason, arithmetic and intended: the engine keeps ONE fp32 accumulator per output across all chunks and
# taps and never K-slices -- in math 0 it adds 3456 two-product MFMA partials in sequence (math 1: 1296 sixteen-product
# partials); with every product of one sign the accumulator grows monotonically and each rounding is relative to the
# running sum, a random walk that torch's blocked float32 conv (the c32 of the family) does not take.  Built the same
# way as c32: max |engine - y| / A of the faithful CPU emulation over the family's layers, never from a GPU result.
# With signed operands the same walk is relative to partial sums of size sqrt(k), far below A, yet still above what the
# blocked float32 conv loses on 6912 terms (2e-8 A): all four long-K families exceed their c32 and take E32.
# On the MI355X the 768 -> 32 layer measured 1.8e-7 A in fp32 with signed operands (2.2 x its c32 bound, 0.55 x this one)
# and 2.9e-6 A in split-f16 with all-positive ones (1.65 x and 0.39 x); the GPU's figures are reported, never used.
E32 = {
    "m0/longk/randn": 8.270e-08, "m0/longk/pos": 2.907e-06, "m1/longk/randn": 5.973e-08, "m1/longk/pos": 1.827e-06,
}


def c_of(layer):
    fam = family_of(layer)
    yard = max(C32[fam], E32.get(fam, 0.0))
    return MARGIN * yard + (P22 if layer.math == 1 else 0.0) + (P22 if layer.case.post else 0.0)


if __name__ == "__main__":
    for fam in FAMILIES:
        print('    "%s": %.3e,' % (fam, measure_c32(fam)))
    for fam in FAMILIES:
        if "/longk/" in fam:
            print('    E32 "%s": %.3e,' % (fam, measure_e32(fam)))
