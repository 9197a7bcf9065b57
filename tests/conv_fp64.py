"""A float64 reference of the split-planar ("SP") conv engine (disconet_amd/csrc/conv_sp.hip, conv_spq.hip,
conv_pre_pair.inl), a CPU emulation of the engine's own arithmetic with switches that break it on purpose, the bound
that separates the two, and the seeded cases the conv tests share.  Plain torch on the CPU, no GPU import.  TEST
infrastructure: tests/test_conv_fp64_cpu.py shows on the CPU that the faithful emulation passes the bound and that every
mutant fails it; tests/test_gpu_conv_fp64.py holds every tile form of the engine to the same bound.

Operands as stored.  The engine never sees x and w: it sees the SP pairs hi = half(x), lo = half(x - hi) of the activations
(sp_layout.h) and of the lifted weights w * wmul (ops._pow2_lift; for the tap-merged up-conv images the pair of the fp32
SUM of the merged taps).  The reference is computed on those values, x~ = hi + lo and w~, so the bound judges the kernel
and not the rounding of its inputs.

The bound.  |got - y| <= c * A per element, A = |scale| (|x~| conv |w~|) + |shift| -- the worst-case magnitude of the
chain that produced the element, so a lost product or a wrong tap shows whatever the cancellation in y.  ReLU is
1-Lipschitz: |relu(a) - relu(b)| <= |a - b|, so comparing post-ReLU values against the pre-ReLU A is the pre-ReLU
comparison wherever y sits within c * A of zero and never looser elsewhere; the same holds stage by stage for the
two-stage forms, whose A is the first stage's A carried through |w2~| (every hidden |value| <= its A).
c = 4 * c32 + 2^-21 (SP output) or 4 * c32 + 2^-22 (fp32 output): c32 is what torch's float32 CPU conv loses against
float64 on the same operands, measured per case family (C32 below, `python -m tests.conv_fp64` prints them), 4 the margin
this project gives a float32 yardstick, 2^-22 the dropped lo * lo term and 2^-22 the rounding of the output to an SP pair.
One family has a yardstick of its own, for a stated reason: E32 below."""
import math
from dataclasses import dataclass, replace
from functools import lru_cache

import torch
import torch.nn.functional as F

P21, P22 = 2.0 ** -21, 2.0 ** -22
F16_MAX = 65504.0
MARGIN = 4.0            # on c32: the margin of the float32 yardstick (as for Adam in test_gpu_loss_optim_fp64.py)


# --- operands as stored -------------------------------------------------------------------------
def _half(v):
    """float64 tensor of fp32-representable values -> the nearest binary16, as float64 (one rounding)"""
    return v.float().half().double()


def sp_split(x):
    """x (fp32 values) -> (hi, lo) float64: hi = half(x), lo = half(x - hi) after the clamp to +-65504 (sp_layout.h,
    sp_device.h :: split4; x - hi is exact in fp32)"""
    x = torch.as_tensor(x)
    v = x.float().double()
    assert torch.equal(v, x.double()), "sp_split takes values that fp32 holds exactly"
    v = v.clamp(-F16_MAX, F16_MAX)
    hi = _half(v)
    return hi, _half(v - hi)


def sp_value(x):
    hi, lo = sp_split(x)
    return hi + lo


def pow2_lift(weight):
    """ops._pow2_lift: the power of two that lifts max |w| into [2^12, 2^13)"""
    m = float(weight.detach().abs().max())
    if not (m > 0.0) or m != m or m == float("inf"):
        return 1.0
    return float(2.0 ** max(-20, min(30, 12 - math.floor(math.log2(m)))))


# taps of a 3x3 kernel on a x2 nearest-upsampled map that read the same source pixel, per output parity p and merged
# tap a (conv_spq.hip :: spq_pack_weights_kernel, conv_sp.hip :: sp_pack_weights_up_kernel)
_R = {(0, 0): (0,), (0, 1): (1, 2), (1, 0): (0, 1), (1, 1): (2,)}


def packed_weights(w, wmul, merge=None, c0=None):
    """w [c_out, c_in, k, k] fp32, wmul -> (hi, lo) float64 [classes, c_out, c_in, k, k]: the pairs of the packed image.
    merge None: one class, every tap its own pair.  merge "quad" / "rows": the tap-merged images of a layer whose first
    c0 channels are upsampled -- four classes (output parity py + 2 px); a group of taps that read one source pixel is
    summed in fp32 in the pack kernel's order and stored as ONE pair, held here on the group's first tap (the others
    zero: on the upsampled map the group's taps see the same value and are inside the map together)."""
    w32 = w.detach().float()
    if merge is None:
        classes = [w32]
    else:
        assert merge in ("quad", "rows") and w32.shape[-1] == 3 and c0
        classes = []
        for cls in range(4):
            py, px = cls & 1, cls >> 1
            m = w32.clone()
            m[:, :c0] = 0.0
            for a in (0, 1):
                rows = _R[(py, a)]
                for cols in ([_R[(px, 0)], _R[(px, 1)]] if merge == "quad" else [(0,), (1,), (2,)]):
                    v = torch.zeros(w32.shape[0], c0)
                    for dy in rows:
                        for dx in cols:
                            v = v + w32[:, :c0, dy, dx]
                    m[:, :c0, rows[0], cols[0]] = v
            classes.append(m)
    v = (torch.stack(classes) * float(wmul)).double().clamp(-F16_MAX, F16_MAX)
    hi = _half(v)
    return hi, _half(v - hi)


@dataclass
class Stage:
    """one conv + affine (+ ReLU) as the engine holds it: wh / wl [classes, c_out, c_in, k, k] float64 (lifted),
    scale = the fp32 scale / wmul, shift"""
    wh: torch.Tensor
    wl: torch.Tensor
    scale: torch.Tensor
    shift: torch.Tensor
    relu: bool
    stride: int = 1


@dataclass
class Operands:
    x0h: torch.Tensor            # [n, c0, h0, w0] float64 (h0 = h / 2 when up0)
    x0l: torch.Tensor
    x1h: torch.Tensor            # [n, c1, h, w] or None
    x1l: torch.Tensor
    up0: bool
    s1: Stage
    s2: Stage = None             # fused second stage (1x1: dn_spconv2d_post1x1; 3x3: the stem pair), fed the SP pair of stage 1
    ahi: bool = False            # source 0 is hi-only / a bit grid: the engine runs no x_lo product


@dataclass
class Ref:
    y: torch.Tensor
    A: torch.Tensor


def assemble(x0, x1=None, up0=False):
    x = x0.repeat_interleave(2, 2).repeat_interleave(2, 3) if up0 else x0
    return x if x1 is None else torch.cat((x, x1), 1)


def _conv_cls(x, w, stride):
    """conv of x with class kernels w [classes, ...]: class py + 2 px at output pixels of that parity"""
    pad = w.shape[-1] // 2
    if w.shape[0] == 1:
        return F.conv2d(x, w[0], None, stride=stride, padding=pad)
    assert stride == 1 and pad == 1 and x.shape[2] % 2 == 0 and x.shape[3] % 2 == 0
    xp = F.pad(x, (1, 1, 1, 1))
    out = x.new_empty(x.shape[0], w.shape[1], x.shape[2], x.shape[3])
    for c in range(4):              # a class lives on one output parity: its conv at stride 2 from that offset
        py, px = c & 1, c >> 1
        out[:, :, py::2, px::2] = F.conv2d(xp[:, :, py:, px:], w[c], None, stride=2)
    return out


def _view(t):
    return t.view(1, -1, 1, 1)


def conv64(op):
    """-> Ref(y, A): the layer in float64 on the operands as stored.  A second stage reads the SP pair of the first
    stage's fp32 output, as the kernels do (conv_sp.hip: split4 before the 1x1 MFMAs; conv_pre_pair.inl: the patch in
    LDS), and A is carried through it."""
    x = assemble(op.x0h + op.x0l, None if op.x1h is None else op.x1h + op.x1l, op.up0)
    s = op.s1
    w = s.wh + s.wl
    y = _conv_cls(x, w, s.stride) * _view(s.scale) + _view(s.shift)
    A = _conv_cls(x.abs(), w.abs(), s.stride) * _view(s.scale.abs()) + _view(s.shift.abs())
    if s.relu:
        y = y.clamp(min=0.0)
    if op.s2 is None:
        return Ref(y, A)
    s = op.s2
    w = s.wh + s.wl
    mid = sp_value(y.float())
    y = _conv_cls(mid, w, s.stride) * _view(s.scale) + _view(s.shift)
    A = _conv_cls(A, w.abs(), s.stride) * _view(s.scale.abs()) + _view(s.shift.abs())
    if s.relu:
        y = y.clamp(min=0.0)
    return Ref(y, A)


def torch32(op):
    """the same layer with torch's float32 CPU conv on the same operands (x~, w~ are exact in fp32): the yardstick"""
    x = assemble(op.x0h + op.x0l, None if op.x1h is None else op.x1h + op.x1l, op.up0).float()
    for s in (op.s1, op.s2):
        if s is None:
            break
        x = _conv_cls(x, (s.wh + s.wl).float(), s.stride) * _view(s.scale.float()) + _view(s.shift.float())
        if s.relu:
            x = x.clamp(min=0.0)
    return x.double()


# --- the engine's arithmetic, and ways to get it wrong ------------------------------------------------
MUTANTS = ("drop_xhi_wlo", "drop_xlo_whi", "zero_out_lo", "tap_shift_edge", "drop_octet")
GEOMETRIC = ("tap_shift_edge", "drop_octet")


def ks_bounds(ngroups, kslices, c0g=None):
    """first chunk of every K slice.  conv_sp.hip: equal shares of the chunks; conv_spq.hip (c0g given): equal shares of
    the work, a chunk of the upsampled source counting 4 merged taps and one of the second source 9"""
    S = kslices
    if S == 1:
        return [0, ngroups]
    if c0g is None:
        return [s * ngroups // S for s in range(S)] + [ngroups]
    c1g = ngroups - c0g
    wtot = 4 * c0g + 9 * c1g
    before = lambda g: 4 * g if g <= c0g else 4 * c0g + 9 * (g - c0g)
    b = [0]
    for sl in range(1, S):
        g = b[-1] + 1
        while g < ngroups - (S - 1 - sl) - 1 and before(g) * S < wtot * sl:
            g += 1
        b.append(g)
    return b + [ngroups]


def _chain(xh, xl, s, mutant, tw, bounds, skip_xlo):
    """fp32 accumulator of one stage: per K slice from zero, per 16-channel chunk, per tap, the products w_lo x_hi,
    w_hi x_lo, w_hi x_hi in the kernel's order, each a 16-term MFMA partial (taken exact) added to the fp32 accumulator;
    the slices' accumulators added in slice order"""
    n, cin, h, w = xh.shape
    k = s.wh.shape[-1]
    pad, st = k // 2, s.stride
    ho, wo = (h + 2 * pad - k) // st + 1, (w + 2 * pad - k) // st + 1
    nch = (cin + 15) // 16
    if mutant == "drop_octet":
        xh, xl = xh.clone(), xl.clone()
        xh[:, 16 * (nch - 1) + 8:] = 0.0
        xl[:, 16 * (nch - 1) + 8:] = 0.0
    xp = [F.pad(t, (pad, pad + 1, pad, pad)) for t in (xh, xl)]     # one spare column right: the shifted tap
    ncls = s.wh.shape[0]
    col = torch.arange(wo)
    edge = (col % tw == tw - 1).view(1, 1, 1, -1)
    par = [None] * 4
    if ncls == 4:
        yy, xx = torch.meshgrid(torch.arange(ho), torch.arange(wo), indexing="ij")
        par = [((yy & 1) == (c & 1)) & ((xx & 1) == (c >> 1)) for c in range(4)]

    def tap(t, cs, ty, tx, shift=0):
        return t[:, cs, ty:ty + st * (ho - 1) + 1:st, tx + shift:tx + shift + st * (wo - 1) + 1:st]

    total = None
    for si in range(len(bounds) - 1):
        acc = torch.zeros(n, s.wh.shape[1], ho, wo, dtype=torch.float32)
        for g in range(bounds[si], bounds[si + 1]):
            cs = slice(16 * g, min(16 * g + 16, cin))
            for ty in range(k):
                for tx in range(k):
                    for prod in range(3):
                        if (prod == 0 and mutant == "drop_xhi_wlo") or (prod == 1 and (mutant == "drop_xlo_whi" or skip_xlo)):
                            continue
                        wt = (s.wl if prod == 0 else s.wh)[:, :, cs, ty, tx]
                        if not bool(wt.any()):
                            continue                      # a merged group's other taps (and padding): nothing is issued
                        src = xp[1 if prod == 1 else 0]
                        v = tap(src, cs, ty, tx)
                        if mutant == "tap_shift_edge" and ty == pad and tx == k - 1:
                            v = torch.where(edge, tap(src, cs, ty, tx, 1), v)
                        if ncls == 1:
                            p = torch.einsum("oc,nchw->nohw", wt[0], v)
                        else:
                            p = torch.zeros(acc.shape, dtype=torch.float64)
                            for c in range(4):
                                p = torch.where(par[c], torch.einsum("oc,nchw->nohw", wt[c], v), p)
                        acc = (acc.double() + p).float()
        total = acc if total is None else (total.double() + acc.double()).float()
    return total


def engine32(op, mutant=None, tw=32, kslices=1, spq=False, out_f32=False):
    """A CPU emulation of the engine: _chain per stage, the fp32 fma of the affine, ReLU, the output split to an SP pair
    (out_f32: the fp32 value, the engine's NHWC outputs) -> float64 [n, c, h, w].  mutant: one of MUTANTS --
    drop_xhi_wlo / drop_xlo_whi lose one cross product (of every stage), zero_out_lo writes a zero lo half,
    tap_shift_edge reads the middle row's right tap one pixel further in the last column of every tw-wide tile,
    drop_octet loses channels 8..15 of the last chunk (first stage)."""
    assert mutant is None or mutant in MUTANTS
    xh = assemble(op.x0h, op.x1h, op.up0)
    xl = assemble(op.x0l, op.x1l, op.up0)
    for i, s in enumerate((op.s1, op.s2)):
        if s is None:
            break
        nch = (xh.shape[1] + 15) // 16
        c0g = (op.x0h.shape[1] + 15) // 16 if spq else None
        bounds = ks_bounds(nch, kslices if i == 0 else 1, c0g)
        acc = _chain(xh, xl, s, mutant if i == 0 or mutant not in GEOMETRIC else None, tw, bounds, op.ahi and i == 0)
        v = (acc.double() * _view(s.scale) + _view(s.shift)).float()        # one rounding: the epilogue's fma
        if s.relu:
            v = v.clamp(min=0.0)
        xh, xl = sp_split(v)
    if out_f32:
        return v.double()
    return xh if mutant == "zero_out_lo" else xh + xl


# --- the bound ------------------------------------------------------------------------------------
def bound_c(c32, out_f32=False):
    return MARGIN * c32 + (P22 if out_f32 else P21)


def worst(got, ref, c):
    """max over elements of |got - y| / (c A); <= 1 passes.  An element with A = 0 (nothing fed it) must be exact."""
    err = (got.double() - ref.y).abs()
    lim = c * ref.A
    r = torch.where(lim > 0, err / lim.clamp(min=1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    return float(r.max())


# --- cases ------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    """one layer: n images of h x w (the conv's input size; source 0 is h/2 x w/2 when up0), c0 (+ c1) -> c_out.
    sign "randn": signed activations and weights; "pos": |randn| + 0.01 and |w| -- every product has one sign, so a lost
    one adds up.  src: "sp" full pairs, "hi" values exact in binary16, "bits" a 0/1 occupancy grid.
    merge: the packed image of an up-conv (None / "quad" / "rows").  post: (c_out2, split, relu2, block_diag) of the
    fused 1x1 stage; stem: c_out of the second 3x3 layer of the stem pair."""
    n: int
    h: int
    w: int
    c0: int
    c_out: int
    k: int = 3
    stride: int = 1
    c1: int = 0
    up0: bool = False
    relu: bool = True
    sign: str = "randn"
    src: str = "sp"
    merge: str = None
    post: tuple = None
    stem: int = 0
    seed: int = 0


@dataclass
class Made:
    case: Case
    op: Operands
    x0: torch.Tensor             # fp32 NCHW, as generated
    x1: torch.Tensor
    w1: torch.Tensor             # fp32 OIHW, unlifted
    wmul1: float
    scale1: torch.Tensor         # fp32, unlifted (the kernel takes scale / wmul)
    shift1: torch.Tensor
    w2: torch.Tensor = None
    wmul2: float = 1.0
    scale2: torch.Tensor = None
    shift2: torch.Tensor = None


def _kaiming(g, c_out, c_in, k, pos):
    w = torch.randn(c_out, c_in, k, k, generator=g) * (2.0 / (c_in * k * k)) ** 0.5
    return w.abs() if pos else w


def _stage(w, merge, c0, scale, shift, relu, stride=1):
    wmul = pow2_lift(w)
    wh, wl = packed_weights(w, wmul, merge, c0)
    return Stage(wh, wl, (scale / wmul).double(), shift.double(), relu, stride), wmul


@lru_cache(maxsize=None)
def make(case):
    """-> Made: seeded tensors of `case` and the operands as the engine stores them"""
    c = case
    g = torch.Generator().manual_seed(1000003 * c.seed + 7919 * c.c0 + 131 * c.c_out + 17 * c.h + c.w + 5 * c.c1)
    pos = c.sign == "pos"
    h0, w0 = (c.h // 2, c.w // 2) if c.up0 else (c.h, c.w)

    def act(ch, hh, ww):
        x = torch.randn(c.n, ch, hh, ww, generator=g)
        return x.abs() + 0.01 if pos else x
    if c.src == "bits":
        x0 = (torch.rand(c.n, c.c0, h0, w0, generator=g) < 0.3).float()
        x0[0, :, 0, 0] = 1.0                      # corners: the halo of the patch is zero padding
        x0[-1, :, -1, -1] = 1.0
    elif c.src == "hi":
        x0 = act(c.c0, h0, w0).half().float()
    else:
        x0 = act(c.c0, h0, w0)
    x1 = act(c.c1, c.h, c.w) if c.c1 else None
    w1 = _kaiming(g, c.c_out, c.c0 + c.c1, c.k, pos)
    scale1 = torch.rand(c.c_out, generator=g) + 0.5
    shift1 = torch.randn(c.c_out, generator=g) * 0.1
    s1, wmul1 = _stage(w1, c.merge, c.c0, scale1, shift1, c.relu, c.stride)
    x0h, x0l = sp_split(x0)
    x1h, x1l = sp_split(x1) if c.c1 else (None, None)
    m = Made(c, Operands(x0h, x0l, x1h, x1l, c.up0, s1, None, c.src != "sp"), x0, x1, w1, wmul1, scale1, shift1)
    if c.post or c.stem:
        if c.post:
            c2, split, relu2, block_diag = c.post
            w2 = _kaiming(g, c2, c.c_out, 1, pos)
            if block_diag:                        # rows < split read hidden channels 0..31, the rest 32..63
                w2[:split, 32:] = 0.0
                w2[split:, :32] = 0.0
        else:
            c2, relu2 = c.stem, True
            w2 = _kaiming(g, c2, c.c_out, 3, pos)
        m.w2 = w2
        m.scale2 = torch.rand(c2, generator=g) + 0.5
        m.shift2 = torch.randn(c2, generator=g) * 0.1
        m.op.s2, m.wmul2 = _stage(w2, None, None, m.scale2, m.shift2, bool(relu2))
    return m


@lru_cache(maxsize=None)
def reference(case):
    return conv64(make(case).op)


def lo_fraction(case):
    """fraction of the stored operands of `case` whose lo half is not zero (full-pair sources and weights)"""
    m = make(case)
    parts = [m.op.s1.wl[m.op.s1.wh != 0]]
    if case.src == "sp":
        parts.append(m.op.x0l.reshape(-1))
    if m.op.x1l is not None:
        parts.append(m.op.x1l.reshape(-1))
    v = torch.cat([p.reshape(-1) for p in parts])
    return float((v != 0).double().mean())


# --- case families: the CPU file runs these; the GPU file takes its constant from the family of its case ----------
def family_of(case):
    if case.stem:
        kind = "stem"
    elif case.post:
        kind = "post"
    elif case.src != "sp":
        kind = "hi"
    elif case.c0 + case.c1 >= 512:
        kind = "longk"
    elif case.up0:
        kind = "up"
    elif case.k == 1:
        kind = "s1"
    elif case.stride == 2:
        kind = "s3s2"
    else:
        kind = "s3"
    return kind + "/" + case.sign


def _both(*cases):
    return {sign: [replace(c, sign=sign) for c in cases] for sign in ("randn", "pos")}


_FAMILY_CASES = {
    "s3": _both(Case(1, 12, 20, 16, 32), Case(1, 12, 20, 80, 64)),
    "s3s2": _both(Case(1, 13, 21, 44, 64, stride=2)),
    "s1": _both(Case(1, 12, 20, 128, 64, k=1), Case(1, 12, 20, 48, 12, k=1, relu=False)),
    "up": _both(Case(1, 12, 20, 48, 32, c1=44, up0=True, merge="quad"), Case(1, 12, 20, 16, 32, c1=12, up0=True, merge="rows")),
    "hi": _both(Case(1, 12, 20, 13, 32, src="hi"), Case(1, 12, 20, 13, 32, src="bits")),
    "post": _both(Case(1, 12, 20, 44, 64, post=(48, 48, False, False)), Case(1, 12, 20, 16, 64, post=(48, 12, False, True))),
    "stem": _both(Case(1, 12, 20, 13, 32, src="bits", stem=32)),
    "longk": _both(Case(1, 16, 16, 768, 32)),
}
FAMILIES = {kind + "/" + sign: cases for kind, by_sign in _FAMILY_CASES.items() for sign, cases in by_sign.items()}

# mutants a family is not meant to catch: a hi-only source has no x_lo product to lose
NOT_MEANT = {"hi/randn": ("drop_xlo_whi",), "hi/pos": ("drop_xlo_whi",)}


def measure_c32(family):
    """max over the family's cases and outputs of |conv_float32(x~, w~) - y| / A"""
    worst32 = 0.0
    for case in FAMILIES[family]:
        ref = reference(case)
        worst32 = max(worst32, worst(torch32(make(case).op), ref, 1.0))
    return worst32


# Measured with `python -m tests.conv_fp64` (torch CPU float32 conv against conv64 on the operands as stored; the
# figure moves a little with torch's conv algorithm and thread count: tests/test_conv_fp64_cpu.py fails at a factor 2).
C32 = {
    "s3/randn": 1.744e-07, "s3/pos": 8.286e-07,
    "s3s2/randn": 9.443e-08, "s3s2/pos": 6.116e-07,
    "s1/randn": 1.760e-07, "s1/pos": 3.931e-07,
    "up/randn": 2.770e-07, "up/pos": 8.281e-07,
    "hi/randn": 1.564e-07, "hi/pos": 6.154e-07,
    "post/randn": 2.703e-08, "post/pos": 4.765e-07,
    "stem/randn": 2.665e-08, "stem/pos": 9.758e-07,
    "longk/randn": 1.875e-08, "longk/pos": 4.649e-07,
}


# The un-sliced long-K layer takes a yardstick of its own (all-positive operands only).  Reason, arithmetic and intended:
# the engine keeps ONE fp32 accumulator per output and adds 48 chunks x 9 taps x 3 products = 1296 MFMA partials to it in
# sequence; with every product positive the accumulator grows monotonically and each of the 1296 roundings is relative to
# the running sum, a random walk that torch's blocked float32 conv (the c32 of this family) does not take.  The K-sliced
# form of the same layer (four chains of a quarter of the length, what the product runs on its long-K layers) stays on
# c32.  Built the same way as c32: max |engine32 - y| / A of the faithful CPU emulation over the family's cases
# (`python -m tests.conv_fp64`), x MARGIN.  On the MI355X the 768 -> 32 case measured 3.1e-6 A un-sliced (1.34 x the c32
# constant 2.34e-6, 0.35 x this one); in four slices it stays below 0.34 x the c32 constant.
E32 = {
    "longk/pos": 2.100e-06,
}


def measure_e32(family):
    return max(worst(engine32(make(case).op, spq=case.merge == "quad"), reference(case), 1.0) for case in FAMILIES[family])


def c_of(case, out_f32=False, kslices=1):
    fam = family_of(case)
    yard = C32[fam]
    if kslices == 1:
        yard = max(yard, E32.get(fam, 0.0))
    return bound_c(yard, out_f32)


if __name__ == "__main__":
    for fam in FAMILIES:
        print('    "%s": %.3e,' % (fam, measure_c32(fam)))
    for fam in E32:
        print('    E32 "%s": %.3e,' % (fam, measure_e32(fam)))
