"""A float64 reference of the conv weight gradient (disconet_amd/csrc/conv_wgrad.hip, wgrad_sp.inl), a CPU emulation of the
kernels' own summation with switches that break it on purpose, the bound that separates the two, and the seeded cases the
weight-gradient tests share.  Plain torch on the CPU, no GPU import.  TEST infrastructure: tests/test_wgrad_fp64_cpu.py
shows on the CPU that the faithful emulation passes the bound, that every mutant fails it on the cases meant to catch it and
that every case's claimed plan is what dn_conv_wgrad_plan returns; tests/test_gpu_wgrad_fp64.py holds every kernel to the
same bound and the launch record (dn_conv_wgrad_last_form) to the case's claim.

Operands as stored.  The fp32 kernels see the fp32 values.  The split-f16 ("SP") kernels see hi = half(v * lift),
lo = half(v * lift - hi) after the clamp to +-65504, for dz (dz_lift: the rule of train.py, largest element near 2^8) and for
x (x_lift = 16); the reference is the float64 sum on v~ = (hi + lo) / lift, so the bound judges the kernel and not the
rounding of its inputs.

The bound.  |got - dW| <= c * A per element, A = sum |dz~| |x~| over the same pixels and tap; an element with A = 0 (a tap
that sees only padding, an all-zero dz) must be exactly 0.  accumulate onto a non-zero dW adds |old| to A and one fp32
rounding (2^-24) to c.  c = MARGIN * yard for the fp32 kernels and MARGIN * yard + 2^-22 for the SP kernels (the dropped
lo * lo product).  yard is what a float32 CPU evaluation of the same sum (torch matmul) loses against the float64
reference, normalised by A, measured per case family: YARD below, `python -m tests.wgrad_fp64` prints the table.  No family
needed a yardstick of its own: the faithful emulation of the kernels' chain stays below MARGIN * yard everywhere
(test_wgrad_fp64_cpu.py asserts it), so there is no counterpart of conv_fp64.E32 here.

The emulation.  fp32 accumulation ordered at the granularity of (tile, wave) partial sums, a partial itself taken exact
(inside one partial the order is free): a slice walks tiles slice, slice + n_slices, ... in order, every wave adding the
partial of its rows of the tile (32-channel blocks: a quarter of the rows each; 64-channel blocks: a wave owns a quadrant
over all pixels of the tile) to its fp32 accumulator; the four waves of a 32-channel block add in wave order; the slices add
as wgrad_reduce_kernel adds them: wave g walks slices g, g + 4, ... in two alternating chains plus a tail, then
(w0 + w1) + (w2 + w3), then the power-of-two scale.  SP: split operands, three products per partial."""
import math
from dataclasses import dataclass
from functools import lru_cache

import torch

from tests.conv_fp64 import MARGIN, P22, Ref, assemble, sp_split, worst  # noqa: F401

P24 = 2.0 ** -24
X_LIFT = 16.0

# form -> (engine, ksize, stride, block, TH): the kernel instantiation and the rows of its pixel tile (16 columns everywhere)
FORMS = {
    "F32-3x3s1": ("f32", 3, 1, 32, 8), "F32-3x3s2": ("f32", 3, 2, 32, 4), "F32-1x1": ("f32", 1, 1, 32, 8),
    "F64": ("f32", 3, 1, 64, 4),
    "SP64s1": ("sp", 3, 1, 64, 4), "SP32s1": ("sp", 3, 1, 32, 8), "SP64s2": ("sp", 3, 2, 64, 1), "SP32s2": ("sp", 3, 2, 32, 4),
}


@dataclass(frozen=True)
class Case:
    """One launch.  n images of h x w (the conv's input size; source 0 is h/2 x w/2 when up0), c0 (+ c1) -> c_out by `form`.
    vals: "randn" mixed-sign x | "relu" x >= 0, half zeros | "grid" a 5 %-dense 0/1 x | "small" dz ~ 1e-4 | "zero" dz = 0 |
    "max" one |dz * lift| = 65504.  off = (off0, off1, offz): floats in front of each operand's channels inside its row,
    pad = floats behind them (ld = off + c + pad): off % 4 == 0 is a channel slice of a wider tensor, off = 1 a misaligned one.
    cin_total / ci_first: dW is a column block of a wider weight.  n_tiles, n_slices, lens (tiles of the first and the last
    slice): the plan this case claims -- with the form's block and tile rows, what dn_conv_wgrad_plan must return.
    vec: the (vec0, vec1, vecz) flags the launch record must show.  refuse: the entry point must return an error."""
    name: str
    form: str
    n: int
    h: int
    w: int
    c0: int
    c_out: int
    n_tiles: int
    n_slices: int
    lens: tuple = None
    c1: int = 0
    up0: bool = False
    vals: str = "randn"
    off: tuple = (0, 0, 0)
    pad: tuple = (0, 0, 0)
    cin_total: int = 0
    ci_first: int = 0
    accumulate: bool = False
    vec: tuple = (1, 1, 1)
    refuse: bool = False
    heavy: bool = False          # too long for the mutant sweep of the CPU file (the faithful emulation still runs)

    @property
    def eng(self):
        return FORMS[self.form][0]

    @property
    def k(self):
        return FORMS[self.form][1]

    @property
    def stride(self):
        return FORMS[self.form][2]

    @property
    def ct(self):
        return FORMS[self.form][3]

    @property
    def TH(self):
        return FORMS[self.form][4]

    @property
    def ld(self):
        return tuple(o + c + p for o, c, p in zip(self.off, (self.c0, self.c1, self.c_out), self.pad))

    @property
    def out_hw(self):
        pad = self.k // 2
        return (self.h + 2 * pad - self.k) // self.stride + 1, (self.w + 2 * pad - self.k) // self.stride + 1

    def plan_claim(self):
        ho, wo = self.out_hw
        return dict(ct=self.ct, TH=self.TH, TW=16, h_out=ho, w_out=wo, n_tiles=self.n_tiles, n_slices=self.n_slices,
                    taps=self.k * self.k)

    def form_claim(self, zsp=False):
        sp = self.eng == "sp"
        vec = self.vec if not sp else (self.vec[0], self.vec[0], 1)
        return dict(entry=(2 if zsp else 1) if sp else 0, ks=self.k, stride=self.stride, block=self.ct, zsp=int(zsp),
                    vec0=vec[0], vec1=vec[1], vecz=vec[2], n_slices=self.n_slices)


def desc_of(case, conv_desc):
    """the dn_conv_desc of the case (conv_desc: disconet_amd.ops.conv_desc; host side, no GPU)"""
    ld = case.ld
    return conv_desc(case.n, case.h, case.w, case.c0, case.c_out, ksize=case.k, stride=case.stride, relu=False, c1=case.c1,
                     up0=case.up0, ld0=ld[0], ld1=ld[1] if case.c1 else 0, ldo=ld[2])


def arg_spec(case):
    """what the GPU test hands the entry point: per pointer argument whether it is given and its byte offset mod 16.  A
    refused case must be refused for its layout, never for a missing pointer (tests/test_wgrad_fp64_cpu.py)."""
    s = {"src0": (True, 4 * case.off[0] % 16), "src1": (case.c1 > 0, 4 * case.off[1] % 16), "dz": (True, 4 * case.off[2] % 16),
         "workspace": (True, 0), "dw": (True, 0)}
    return s


# --- operands ---------------------------------------------------------------------------------------
@dataclass
class Made:
    case: Case
    x0: torch.Tensor             # fp32 NCHW as generated ([n, c0, h/2, w/2] when up0)
    x1: torch.Tensor
    dz: torch.Tensor             # fp32 [n, c_out, h_out, w_out]
    dz_lift: float
    old: torch.Tensor            # fp32 [c_out, c_in, k, k]: what dW holds before an accumulating launch (None otherwise)
    sx: torch.Tensor             # float64 [n, c_in, h, w]: the gathered input as stored (upsampled, concatenated)
    sdz: torch.Tensor            # float64: dz as stored


def lift_of(dz):
    """train.py's rule: the power of two that brings the largest |dz| into [2^8, 2^9)"""
    m = float(dz.abs().max())
    return 1.0 if not m > 0.0 else float(2.0 ** (8 - math.floor(math.log2(m))))


def stored(v, lift, sp):
    if not sp:
        return v.double()
    hi, lo = sp_split(v * lift)
    return (hi + lo) / lift


@lru_cache(maxsize=None)
def make(case):
    c = case
    g = torch.Generator().manual_seed(7919 * sum(map(ord, c.name)) + 131 * c.c0 + 17 * c.h + c.w)
    h0, w0 = (c.h // 2, c.w // 2) if c.up0 else (c.h, c.w)
    ho, wo = c.out_hw

    def act(ch, hh, ww):
        if c.vals == "grid":
            return (torch.rand(c.n, ch, hh, ww, generator=g) < 0.05).float()
        x = torch.randn(c.n, ch, hh, ww, generator=g)
        return x.clamp(min=0.0) if c.vals == "relu" else x
    x0 = act(c.c0, h0, w0)
    if c.vals == "grid":
        x0[0, :, 0, 0] = 1.0          # the corners: the halo of the patch is zero padding there
        x0[-1, :, -1, -1] = 1.0
    x1 = act(c.c1, c.h, c.w) if c.c1 else None
    dz = torch.randn(c.n, c.c_out, ho, wo, generator=g)
    if c.vals == "small":
        dz = dz * 1e-4
    elif c.vals == "zero":
        dz = torch.zeros_like(dz)
    lift = lift_of(dz) if c.vals != "max" else 2.0 ** 6
    if c.vals == "max":               # randn stays below 2^3: one element is lifted onto the largest binary16 exactly
        dz[0, 0, 0, 0] = 65504.0 / lift
        dz[-1, -1, -1, -1] = -65504.0 / lift
    sp = c.eng == "sp"
    sx = assemble(stored(x0, X_LIFT, sp), stored(x1, X_LIFT, sp) if c.c1 else None, c.up0)
    sdz = stored(dz, lift, sp)
    old = None
    if c.accumulate:                  # 10^3 times the gradient's typical magnitude (sqrt(pixels) for randn operands)
        old = torch.randn(c.c_out, c.c0 + c.c1, c.k, c.k, generator=g) * (1e3 * math.sqrt(c.n * ho * wo))
    return Made(c, x0, x1, dz, lift, old, sx, sdz)


def _taps(case, sx, fn):
    """fn(ky, kx, xs) for every tap, xs [n, c_in, h_out, w_out] = the input pixel each output pixel sees through the tap"""
    k, s = case.k, case.stride
    ho, wo = case.out_hw
    xp = torch.nn.functional.pad(sx, (k // 2,) * 4)
    return [[fn(ky, kx, xp[:, :, ky:ky + s * (ho - 1) + 1:s, kx:kx + s * (wo - 1) + 1:s]) for kx in range(k)] for ky in range(k)]


def _oi(dz, xs):
    """sum over pixels: [n, co, h, w] x [n, ci, h, w] -> [co, ci]"""
    co, ci = dz.shape[1], xs.shape[1]
    return dz.permute(1, 0, 2, 3).reshape(co, -1) @ xs.permute(1, 0, 2, 3).reshape(ci, -1).t()


def _stack(rows):
    return torch.stack([torch.stack(r, -1) for r in rows], -2)         # [co, ci, ky, kx]


@lru_cache(maxsize=None)
def reference(case):
    """-> Ref(y, A): dW [c_out, c_in, k, k] in float64 on the operands as stored (plus the old dW of an accumulating launch)"""
    m = make(case)
    y = _stack(_taps(case, m.sx, lambda ky, kx, xs: _oi(m.sdz, xs)))
    A = _stack(_taps(case, m.sx.abs(), lambda ky, kx, xs: _oi(m.sdz.abs(), xs)))
    if m.old is not None:
        y, A = y + m.old.double(), A + m.old.double().abs()
    return Ref(y, A)


def float32_sum(case):
    """the same sum by torch's float32 CPU matmul on the same operands (exact in fp32): the yardstick"""
    m = make(case)
    y = _stack(_taps(case, m.sx.float(), lambda ky, kx, xs: _oi(m.sdz.float(), xs))).double()
    return y if m.old is None else (m.old + y.float()).double()


# --- the kernels' arithmetic, and ways to get it wrong -------------------------------------------------------
MUTANTS = ("halo_col", "halo_row", "skip_last_tile", "drop_slice", "drop_chain_tail", "drop_lo_hi", "drop_hi_lo", "swap_dz_pair",
           "ignore_last_co_block", "ignore_last_ci_block", "concat_as_upsampled", "transpose_tap", "scale_dz_only", "overwrite")
_GEOMETRIC = ("halo_col", "halo_row", "drop_lo_hi", "drop_hi_lo", "swap_dz_pair", "concat_as_upsampled")     # change the partials


def tiles_of(case):
    ho, wo = case.out_hw
    return (wo + 15) // 16, (ho + case.TH - 1) // case.TH


def targets(mutant, case):
    """is `case` meant to catch `mutant`?  (False: the mutant cannot change this launch, or only by an amount that the case's
    values do not guarantee.)"""
    c = case
    tx, ty = tiles_of(c)
    if c.refuse or c.vals == "zero":
        return False
    if c.heavy and mutant in _GEOMETRIC:
        return False
    return {
        "halo_col": c.k == 3 and tx >= 2,                       # the column behind tile 0 is inside the map
        "halo_row": c.k == 3 and ty >= 2,
        "skip_last_tile": True,
        "drop_slice": c.n_slices >= 2,
        "drop_chain_tail": c.n_slices % 8 != 0,                 # with 8 k slices every wave's chains are even: no tail
        "drop_lo_hi": c.eng == "sp",
        "drop_hi_lo": c.eng == "sp" and c.vals != "grid",       # a 0/1 grid has no lo half
        "swap_dz_pair": not (c.k == 1 and c.up0 and not c.c1),  # 1x1 on an upsampled map: the pair's pixels read the same source pixel
        "ignore_last_co_block": c.c_out % c.ct != 0,
        "ignore_last_ci_block": (c.c1 or c.c0) % c.ct != 0,
        "concat_as_upsampled": c.c1 > 0 and c.up0 and c.h > 2,
        "transpose_tap": c.k == 3 and c.out_hw != (1, 1) and (c.h, c.w) != (1, 1),
        "scale_dz_only": c.eng == "sp",
        "overwrite": c.accumulate,
    }[mutant]


def _f32(v):
    return v.float()


def _partials(case, mutant):
    """-> [taps][T, W, co, ci] float64: the (tile, wave) partial sums, exact.  SP: on the lifted split operands, the three
    products summed (inside one partial the order is free)."""
    c, m = case, make(case)
    sp = c.eng == "sp"
    tx, ty = tiles_of(c)
    ho, wo = c.out_hw
    W = 4 if c.ct == 32 else 1
    rg = c.TH // W

    def tiled(t):                                      # [n, ch, ho, wo] -> [n, ty, tx, W, ch, rg * 16]
        t = torch.nn.functional.pad(t, (0, tx * 16 - wo, 0, ty * c.TH - ho))
        n, ch = t.shape[:2]
        return t.reshape(n, ch, ty, W, rg, tx, 16).permute(0, 2, 5, 3, 1, 4, 6).reshape(n, ty, tx, W, ch, rg * 16)

    def gathered(parts0, parts1):
        x1 = parts1
        if mutant == "concat_as_upsampled" and parts1 is not None:
            x1 = parts1[:, :, :c.h // 2, :c.w // 2].repeat_interleave(2, 2).repeat_interleave(2, 3)
        return assemble(parts0, x1, c.up0)

    if sp:
        zh, zl = sp_split(m.dz * m.dz_lift)
        x0h, x0l = sp_split(m.x0 * X_LIFT)
        x1h, x1l = sp_split(m.x1 * X_LIFT) if c.c1 else (None, None)
        prods = [(zh, gathered(x0h, x1h)), (zh, gathered(x0l, x1l)), (zl, gathered(x0h, x1h))]
        if mutant == "drop_hi_lo":
            del prods[1]
        if mutant == "drop_lo_hi":
            del prods[2]
    else:
        prods = [(m.dz.double(), gathered(m.x0.double(), None if m.x1 is None else m.x1.double()))]

    out = [None] * (c.k * c.k)
    for dzv, xv in prods:
        if mutant == "swap_dz_pair":                   # the two pixels of every pair of a row change places
            dzv = torch.nn.functional.pad(dzv, (0, tx * 16 - wo))
            dzv = dzv.reshape(*dzv.shape[:3], -1, 2).flip(-1).reshape(*dzv.shape[:3], -1)[..., :wo]
        dt = tiled(dzv)

        def tap(ky, kx, xs):
            if mutant == "halo_col" and (ky, kx) == (1, c.k - 1):
                xs = xs.clone()
                xs[0, :, :c.TH, 15] = 0.0               # tile 0 never loaded the patch column behind its last pixel
            if mutant == "halo_row" and (ky, kx) == (c.k - 1, 1):
                xs = xs.clone()
                xs[0, :, c.TH - 1, :16] = 0.0
            p = (dt @ tiled(xs).transpose(-1, -2)).reshape(-1, W, dt.shape[4], xs.shape[1])
            i = ky * c.k + kx
            out[i] = p if out[i] is None else out[i] + p
        _taps(c, xv, tap)
    return out


@lru_cache(maxsize=2)
def _faithful_partials(case):
    return _partials(case, None)


def _reduce(case, P, mutant):
    """one tap's partials [T, W, co, ci] -> dW [co, ci] float32 the way the slices, waves and the reduce kernel add"""
    T, W = P.shape[:2]
    S = case.n_slices
    acc = torch.zeros((S, W) + tuple(P.shape[2:]), dtype=torch.float32)
    for r in range((T + S - 1) // S):                  # round r: slice s takes tile r S + s
        k = min(S, T - r * S)
        acc[:k] = _f32(acc[:k].double() + P[r * S:r * S + k])
    part = acc[:, 0]
    for w in range(1, W):                              # the four waves of a 32-channel block, in wave order
        part = _f32(part.double() + acc[:, w].double())
    wsum = []
    for g in range(4):
        s0 = torch.zeros_like(part[0])
        s1 = torch.zeros_like(part[0])
        sl = g
        while sl + 4 < S:
            if not (mutant == "drop_slice" and sl == 1):
                s0 = _f32(s0.double() + part[sl].double())
            s1 = _f32(s1.double() + part[sl + 4].double())
            sl += 8
        if sl < S and mutant != "drop_chain_tail" and not (mutant == "drop_slice" and sl == 1):
            s0 = _f32(s0.double() + part[sl].double())
        wsum.append(_f32(s0.double() + s1.double()))
    a, b = _f32(wsum[0].double() + wsum[1].double()), _f32(wsum[2].double() + wsum[3].double())
    return _f32(a.double() + b.double())


def emulate(case, mutant=None):
    """A CPU emulation of the launch -> dW float64 [c_out, c_in, k, k]; mutant: one of MUTANTS"""
    assert mutant is None or mutant in MUTANTS
    c, m = case, make(case)
    P = _partials(c, mutant) if mutant in _GEOMETRIC else _faithful_partials(c)
    if mutant == "skip_last_tile":                     # slice 0 = tiles 0, S, 2 S, ...: its last one is never added (+ 0: exact)
        last = ((c.n_tiles - 1) // c.n_slices) * c.n_slices
        P = [p.clone() for p in P]
        for p in P:
            p[last] = 0.0
    taps = [_reduce(c, p, mutant) for p in P]
    scale = 1.0
    if c.eng == "sp":
        scale = 1.0 / m.dz_lift if mutant == "scale_dz_only" else 1.0 / (m.dz_lift * X_LIFT)
    dw = _f32(torch.stack(taps, -1).double() * scale).reshape(c.c_out, c.c0 + c.c1, c.k, c.k)
    if mutant == "transpose_tap":
        dw = dw.transpose(2, 3).contiguous()
    if mutant == "ignore_last_co_block":
        dw[(c.c_out - 1) // c.ct * c.ct:] = 0.0
    if mutant == "ignore_last_ci_block":
        last = c.c1 or c.c0
        dw[:, c.c0 + c.c1 - last + (last - 1) // c.ct * c.ct:] = 0.0
    if m.old is not None and mutant != "overwrite":
        dw = _f32(m.old.double() + dw.double())
    return dw.double()


# --- the bound ----------------------------------------------------------------------------------------
def family_of(case):
    return case.eng + "/" + ("randn" if case.vals == "zero" else case.vals)


# Measured with `python -m tests.wgrad_fp64`: max over the family's cases and elements of |float32_sum - dW| / A (torch's
# float32 CPU matmul against the float64 reference on the operands as stored; the figure moves a little with torch's matmul
# blocking and thread count: tests/test_wgrad_fp64_cpu.py fails at a factor 2).
YARD = {
    "f32/randn": 3.227e-07,      # emulation 1.058e-07
    "f32/relu": 2.145e-07,       # emulation 8.094e-08
    "f32/grid": 1.172e-07,       # emulation 9.499e-08
    "f32/small": 2.372e-07,      # emulation 6.115e-08
    "sp/randn": 3.417e-07,       # emulation 2.050e-07
    "sp/relu": 2.418e-07,        # emulation 9.906e-08
    "sp/grid": 1.324e-07,        # emulation 9.120e-08
    "sp/small": 2.350e-07,       # emulation 5.543e-08
    "sp/max": 8.400e-07,         # emulation 1.510e-07
}


def measure_yard(family):
    return max(worst(float32_sum(c), reference(c), 1.0) for c in CASES if family_of(c) == family and not c.refuse)


def measure_emulation(family):
    return max(worst(emulate(c), reference(c), 1.0) for c in CASES if family_of(c) == family and not c.refuse)


def c_of(case):
    return MARGIN * YARD[family_of(case)] + (P22 if case.eng == "sp" else 0.0) + (P24 if case.accumulate else 0.0)


def breakdown(got, ref, c, c0):
    """worst err / (c A) per tap and per source: what a failing test prints"""
    k = ref.y.shape[-1]
    per_tap = [round(worst(got[:, :, t // k, t % k], Ref(ref.y[:, :, t // k, t % k], ref.A[:, :, t // k, t % k]), c), 3)
               for t in range(k * k)]
    per_src = [round(worst(got[:, s], Ref(ref.y[:, s], ref.A[:, s]), c), 3)
               for s in (slice(0, c0), slice(c0, None)) if ref.y[:, s].numel()]
    return dict(per_tap=per_tap, per_source=per_src)


# --- cases ---------------------------------------------------------------------------------------
def _ch(form):
    return 64 if FORMS[form][3] == 64 else 32


def _case(name, form, n, h, w, n_tiles, n_slices, lens=None, c0=None, c_out=None, **kw):
    c = _ch(form)
    return Case(form + ":" + name, form, n, h, w, c if c0 is None else c0, c if c_out is None else c_out, n_tiles, n_slices,
                lens, **kw)


def _tile_cases():
    out = []
    for form, (eng, k, s, ct, TH) in FORMS.items():
        inp = (lambda ho, wo: (ho, wo)) if s == 1 else (lambda ho, wo: (2 * ho - 1, 2 * wo - 1))
        out.append(_case("partial-tile", form, 1, *inp(3, 5), n_tiles=(3 + TH - 1) // TH, n_slices=1))
        out.append(_case("exact-tile", form, 1, *((TH, 16) if s == 1 else (2 * TH, 32)), n_tiles=1, n_slices=1))
        out.append(_case("2x2-tiles-plus-1", form, 1, *inp(TH + 1, 17), n_tiles=4, n_slices=1))
        if s == 2:
            out.append(_case("odd-7x9", form, 1, 7, 9, n_tiles=(4 + TH - 1) // TH, n_slices=1))
        out.append(_case("1x1-map", form, 2, 1, 1, n_tiles=2, n_slices=1))
        out.append(_case("1x20-map", form, 1, 1, 20, n_tiles=2 if s == 1 else 1, n_slices=1))
        if form in ("F32-3x3s1", "F32-3x3s2", "F32-1x1", "F64", "SP64s1", "SP32s1"):
            out.append(_case("2x2-over-1x1", form, 2, 2, 2, n_tiles=2, n_slices=1, up0=True))
        # three tiles per image, three images: the tile -> image split crosses image boundaries inside both slices
        out.append(_case("3-images-of-3-tiles", form, 3, *((TH, 33) if s == 1 else (2 * TH, 65)), n_tiles=9, n_slices=2, lens=(5, 4)))
    return out


def _slice_cases():
    out = []
    for form in ("F32-3x3s1", "F64", "SP32s1", "SP64s1"):
        TH = FORMS[form][4]
        sp = FORMS[form][0] == "sp"

        def row(T, S, lens):
            return _case("%d-tiles-%d-slices" % (T, S), form, 1, TH, 16 * T, n_tiles=T, n_slices=S, lens=lens)
        out += [row(1, 1, (1, 1)), row(3, 1, (3, 3)), row(7, 1, (7, 7)), row(9, 2, (5, 4))]
        if not sp:
            # every residue of n_slices mod 8; 4 S + 1 tiles: the first slice is one tile longer than the others
            out += [row(4 * S + 1, S, (5, 4)) for S in (3, 4, 5, 6, 7, 8, 9, 11)]
        else:
            out += [row(4 * S + 1, S, (5, 4)) for S in (3, 5, 7)]
            # 9 .. 15 tiles-worth of slices round down to 8; 16 stays
            out += [row(37, 8, (5, 4)), row(47, 8, (6, 5)), row(63, 8, (8, 7)), row(64, 16, (4, 4))]
    # 512 / (n_cot * n_cit) binds: 8 x 8 blocks leave 8 slices where the tiles would give 9
    out.append(_case("block-bound", "F32-1x1", 1, 48, 96, n_tiles=36, n_slices=8, lens=(5, 4), c0=256, c_out=256))
    out.append(_case("block-bound", "SP32s2", 1, 48, 192, n_tiles=36, n_slices=8, lens=(5, 4), c0=224, c_out=288, heavy=True))
    return out


def _channel_cases():
    out = []
    for form in ("F32-3x3s1", "F32-3x3s2", "F32-1x1"):
        for co in (1, 12, 20, 33):
            out.append(_case("c_out-%d" % co, form, 2, 6, 18, n_tiles=4 if form != "F32-3x3s2" else 2, n_slices=1, c_out=co,
                             vec=(1, 1, int(co % 4 == 0))))
    for form in ("F32-3x3s1", "F32-3x3s2", "F32-1x1", "SP32s1"):
        for c0 in (8, 13, 36):
            out.append(_case("c0-%d" % c0, form, 2, 6, 18, n_tiles=4 if form != "F32-3x3s2" else 2, n_slices=1, c0=c0,
                             vals="grid" if c0 == 13 else "randn", vec=(int(c0 % 4 == 0), 1, 1)))
    out += [
        _case("c_out-72", "F64", 1, 5, 18, n_tiles=4, n_slices=1, c_out=72),
        _case("c_out-96", "F64", 1, 5, 18, n_tiles=4, n_slices=1, c_out=96),
        _case("c_out-80", "SP64s1", 1, 5, 18, n_tiles=4, n_slices=1, c_out=80),
        _case("c_out-48-c0-72", "SP32s1", 1, 9, 18, n_tiles=4, n_slices=1, c0=72, c_out=48),
        _case("c_out-48", "SP32s2", 1, 9, 35, n_tiles=4, n_slices=1, c_out=48),
        _case("up-concat-32+4", "F32-3x3s1", 2, 10, 18, n_tiles=8, n_slices=2, lens=(4, 4), c1=4, up0=True),
        _case("up-concat-32+36", "F32-3x3s1", 2, 10, 18, n_tiles=8, n_slices=2, lens=(4, 4), c1=36, up0=True),
        _case("up-concat-64+64", "F64", 2, 6, 18, n_tiles=8, n_slices=2, lens=(4, 4), c1=64, up0=True),
        _case("up-concat-64+64", "SP64s1", 2, 6, 18, n_tiles=8, n_slices=2, lens=(4, 4), c1=64, up0=True),
        _case("up-concat-64+32", "SP32s1", 2, 10, 18, n_tiles=8, n_slices=2, lens=(4, 4), c0=64, c1=32, up0=True),
        # 64 + 32 -> 64: c1 is no multiple of 64, the fp32 engine must stay on the 32-channel blocks
        _case("up-concat-64+32-to-64", "F32-3x3s1", 2, 10, 18, n_tiles=8, n_slices=2, lens=(4, 4), c0=64, c1=32, c_out=64, up0=True),
    ]
    return out


def _layout_cases():
    out = []
    # channel slices of wider tensors at 16-byte aligned offsets, every operand at once
    for form, c0, c1 in (("F32-3x3s1", 32, 36), ("F64", 64, 64), ("SP64s1", 64, 64), ("SP32s1", 64, 32)):
        TH = FORMS[form][4]
        out.append(_case("slices-of-wider", form, 2, TH + 2, 18, n_tiles=8, n_slices=2, lens=(4, 4), c0=c0, c1=c1, up0=True,
                         off=(4, 8, 4), pad=(4, 4, 12)))
    # one operand one float off 16 bytes: dword loads on the kernels that have them (the flag is read from the record) ...
    for form in ("F32-3x3s1", "F32-3x3s2", "F32-1x1"):
        nt = 4 if form != "F32-3x3s2" else 2
        out.append(_case("src0-off-1", form, 2, 6, 18, n_tiles=nt, n_slices=1, off=(1, 0, 0), vec=(0, 1, 1)))
        out.append(_case("dz-off-1", form, 2, 6, 18, n_tiles=nt, n_slices=1, off=(0, 0, 1), vec=(1, 1, 0)))
        out.append(_case("src1-off-1-ld1-wider", form, 2, 6, 18, n_tiles=nt, n_slices=1, c1=8, off=(0, 1, 0), pad=(0, 3, 0), vec=(1, 0, 1)))
    out.append(_case("src0-off-1", "SP32s1", 2, 6, 18, n_tiles=4, n_slices=1, off=(1, 0, 0), vec=(0, 0, 1)))
    # 64 -> 64 with rows of 65 floats: the plans themselves fall back to the 32-channel blocks and their dword loads
    out.append(_case("64-channels-odd-ld0", "F32-3x3s1", 1, 5, 18, n_tiles=2, n_slices=1, c0=64, c_out=64, off=(1, 0, 0), vec=(0, 1, 1)))
    out.append(_case("64-channels-odd-ld0", "SP32s1", 1, 5, 18, n_tiles=2, n_slices=1, c0=64, c_out=64, off=(1, 0, 0), vec=(0, 0, 1)))
    # ... and a refusal before any launch on those that cannot: rows of 4 k floats (the plan keeps its form), the base one float off
    A, B, Z = dict(off=(1, 0, 0), pad=(3, 0, 0)), dict(off=(0, 1, 0), pad=(0, 3, 0)), dict(off=(0, 0, 1), pad=(0, 0, 3))
    out += [
        _case("dz-off-1", "SP32s1", 2, 6, 18, n_tiles=4, n_slices=1, refuse=True, **Z),
        _case("src0-off-1-concat", "SP32s1", 2, 6, 18, n_tiles=4, n_slices=1, c1=32, refuse=True, **A),
        _case("src0-off-1", "F64", 1, 5, 18, n_tiles=4, n_slices=1, refuse=True, **A),
        _case("src1-off-1", "F64", 1, 5, 18, n_tiles=4, n_slices=1, c1=64, refuse=True, **B),
        _case("dz-off-1", "F64", 1, 5, 18, n_tiles=4, n_slices=1, refuse=True, **Z),
        _case("src0-off-1", "SP64s1", 1, 5, 18, n_tiles=4, n_slices=1, refuse=True, **A),
        _case("dz-off-1", "SP64s1", 1, 5, 18, n_tiles=4, n_slices=1, refuse=True, **Z),
        _case("src0-off-1", "SP64s2", 1, 5, 35, n_tiles=6, n_slices=1, refuse=True, **A),
        _case("src0-off-1", "SP32s2", 1, 9, 35, n_tiles=4, n_slices=1, refuse=True, **A),
    ]
    for form in ("F32-1x1", "F32-3x3s1", "SP32s1", "F64"):
        c = _ch(form)
        out.append(_case("column-block", form, 1, 9, 18, n_tiles=4 if c == 32 else 6, n_slices=1, cin_total=c + 20, ci_first=8))
        out.append(_case("accumulate", form, 1, 9, 18, n_tiles=4 if c == 32 else 6, n_slices=1, accumulate=True))
    return out


def _value_cases():
    out = []
    for form in ("F32-3x3s1", "F32-3x3s2", "F64", "SP64s1", "SP32s1", "SP64s2", "SP32s2"):
        s, TH = FORMS[form][2], FORMS[form][4]
        hw = (9, 18) if s == 1 else (17, 35)
        nt = 2 * ((9 + TH - 1) // TH)
        for vals in ("relu", "small", "zero"):
            out.append(_case(vals, form, 1, *hw, n_tiles=nt, n_slices=max(1, nt // 4), lens=None, vals=vals))
    out.append(_case("dz-at-65504", "SP64s1", 1, 9, 18, n_tiles=6, n_slices=1, vals="max"))
    out.append(_case("dz-at-65504", "SP32s2", 1, 17, 35, n_tiles=6, n_slices=1, vals="max"))
    return out


CASES = _tile_cases() + _slice_cases() + _channel_cases() + _layout_cases() + _value_cases()
assert len({c.name for c in CASES}) == len(CASES)


def slice_lengths(n_tiles, n_slices):
    """tiles of the first and of the last slice (slice s takes tiles s, s + n_slices, ...)"""
    return (n_tiles + n_slices - 1) // n_slices, (n_tiles - (n_slices - 1) + n_slices - 1) // n_slices


if __name__ == "__main__":
    for fam in YARD:
        print('    "%s": %.3e,      # emulation %.3e' % (fam, measure_yard(fam), measure_emulation(fam)))
