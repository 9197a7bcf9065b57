"""Every kernel instantiation the fp32-NHWC conv engine (disconet_amd/csrc/conv_mfma.hip: dn_conv2d, dn_conv2d_taps,
dn_conv2d_post1x1) can launch, against the float64 reference of tests/nhwc_conv_fp64.py, at the shapes that reach each
part of that instantiation -- and named: after every launch ops.nhwc_last_form() (the record launch<>() itself writes,
dn_conv_last_form) must equal the row's form, so a retune of one bias in kCfgs that moves a layer class onto another tile
fails here instead of passing on another kernel.

One table (ROWS): form, how it is reached, runs.  The nine tile ids are pinned with dn_conv_force_config(id) in both
math modes (T3S2_64x64 is KC 8 in fp32 and KC 16 in split-f16: two instantiations), the fused 1x1 stage has one form:
19 instantiations, and a guard parses the DN_CONV_CASE lines, the T3S2 case and the post1x1 launch of conv_mfma.hip and
fails if one of them has no row.  The `KC == 8 && kSplit` branch of the kernel (mfma_f32_32x32x8f16) is instantiated by
no product launch -- split-f16 stride 2 takes KC 16 -- so it has no row.  The forms the baseline's layers select get a
row by shape as well, at the smallest shape whose cost (ceil(blocks / 256) x tile area x bias) selects them unforced.

Per launch: the output pre-filled with 0xFF bytes (an unwritten piece is a NaN) inside a wider tensor whose neighbouring
columns must keep their bytes; |got - y| <= c A per element with c = 4 yard (+ 2^-22 in split-f16, + 2^-22 for the fused
stage) of the layer's family; sources as channel slices of wider tensors whose foreign columns hold 3e38 where the run
says so (they meet exact-zero weights in the last chunk and must contribute exactly nothing).

Measured on the MI355X (38 rows, 313 launches; the file takes about 5 s, CPU references included; every recorded form
equalled its row and no row missed the bound): the largest err / (c A) of each row, which every row also prints
(pytest -s)
    forced, f32 / f16x3:
        T3_256x32 0.554 / 0.386; T3_256x64 0.452 / 0.243; T3_128x64 0.473 / 0.305; T3_64x64 0.568 / 0.291
        T3S2_64x64 0.815 / 0.340; T1_256x32 0.433 / 0.244; T1_256x64 0.480 / 0.215; T1_128x128 0.399 / 0.221
        T1_64x64 0.418 / 0.224
    post1x1 0.126; work-item order 0.298 / 0.169
    by shape, f32 / f16x3:
        T3_64x64 0.209 / 0.077; T3_256x32 0.262 / 0.151; T3_128x64 0.315 / 0.165; T3S2_64x64 0.263 / 0.165
        T1_64x64 0.233 / 0.118; T1_256x64 0.184 / 0.134; T1_256x32 0.349 / 0.185; long K 0.554 / 0.386; T3_256x64 - / 0.164
The largest figure, 0.815, is the persistent-loop run of the fp32 stride-2 tile: signed operands, 5.2 M outputs held to a
yardstick measured on a 4928-output family.  The long-K layer (768 -> 32) sits at 0.554 (f32, signed) and 0.386 (f16x3,
all-positive) of its emulation-based yardstick (nhwc_conv_fp64.E32); against c32 alone those would be 2.2 and 1.65."""
import os
import re
from dataclasses import dataclass, replace

import pytest
import torch

from tests import conv_fp64 as C
from tests import nhwc_conv_fp64 as N
from tests.conv_fp64 import Case
from tests.nhwc_conv_fp64 import FULL, PARITY_MASKS, Layer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FORM_KEYS = ("KS", "STRIDE", "TH", "TW", "BN", "KC", "MATH", "POST")
ENTRY = {"conv": 0, "taps": 1, "post": 2}

# enum CfgId of conv_mfma.hip -> (KS, STRIDE, TH, TW, BN, KC in fp32, KC in split-f16)
TILES = {"T3_256x32": (3, 1, 8, 32, 32, 16, 16), "T3_256x64": (3, 1, 8, 32, 64, 16, 16), "T3_128x64": (3, 1, 8, 16, 64, 16, 16),
         "T3_64x64": (3, 1, 8, 8, 64, 16, 16), "T3S2_64x64": (3, 2, 8, 8, 64, 8, 16), "T1_256x32": (1, 1, 8, 32, 32, 32, 32),
         "T1_256x64": (1, 1, 8, 32, 64, 32, 32), "T1_128x128": (1, 1, 8, 16, 128, 32, 32), "T1_64x64": (1, 1, 8, 8, 64, 32, 32)}
POST_FORM = (3, 1, 8, 32, 64, 16, 1, 1)


def form_of(tile, math):
    ks, st, th, tw, bn, kc0, kc1 = TILES[tile]
    return (ks, st, th, tw, bn, kc1 if math else kc0, math, 0)


@dataclass(frozen=True)
class Run:
    """one launch: the layer, the entry point, and where its tensors sit.  pad0 / pad1: foreign columns (3e38) before and
    after a source's own in a wider tensor (a column before moves the base off 16-byte alignment); opad: columns either
    side of the output's own; taps: parity = the (py, px) the output goes to in dx[:, py::2, px::2, :];
    persistent: the launch must hold more work items than workgroups"""
    layer: Layer
    entry: str = "conv"
    pad0: tuple = (0, 0)
    pad1: tuple = (0, 0)
    opad: tuple = (4, 4)
    parity: tuple = (0, 0)
    persistent: bool = False


@dataclass
class Row:
    name: str
    form: tuple
    force: object            # a key of TILES, or None: reached by shape (why says which cost term decides)
    why: str
    runs: list


# --- runs per form ------------------------------------------------------------------------------------
def std_runs(tile, math):
    """The smallest cases that reach each part of a TH x TW pixel, BN channel tile with chunk KC: maps of exactly one
    tile, 3 x 5 and ragged right and bottom (stride 2: odd input sizes); K loops of one chunk (the prologue is the last
    chunk), two, five, a partial last chunk (c0 % KC != 0, c0 % 4 == 0) and 13 channels (dword loads; 3x3 only);
    c_out = BN, BN + 8, 12 (a 64- or 128-wide tile then reads rows past the padded weight count), 1 (scalar stores), 36;
    concat with c0 / KC even and odd, c1 % KC != 0, an upsampled source 0; both signs, ReLU on and off; sources with row
    strides wider than their channels, a base off 16-byte alignment, an output stride that is no multiple of 4"""
    ks, s, th, tw, bn, kc0, kc1 = TILES[tile]
    kc = kc1 if math else kc0
    one = (th * s, tw * s)
    rag = ((th + 3) * s + (s - 1), (tw + 5) * s + (s - 1))
    part = kc + 4
    kw = dict(k=ks, stride=s)
    L = lambda case, **o: Layer(case, math, **o)
    runs = [
        Run(L(Case(2, one[0], one[1], kc, bn, sign="pos", **kw))),
        Run(L(Case(1, 3, 5, 13 if ks == 3 else part, 12, **kw))),
        Run(L(Case(1, rag[0], rag[1], 2 * kc, bn + 8, **kw))),
        Run(L(Case(1, rag[0], rag[1], 5 * kc, 1, sign="pos", **kw))),
        Run(L(Case(2, rag[0], rag[1], part, 36, relu=False, **kw))),
        Run(L(Case(1, one[0], one[1], 5 * kc, bn + 8, sign="pos", **kw))),
        # row strides: foreign 3e38 columns behind the source's own, an output stride of c + 9
        Run(L(Case(1, rag[0], rag[1], part, 12, sign="pos", **kw)), pad0=(0, 12), opad=(4, 5)),
        # the base 4 bytes off: dword loads of a source whose c0 is a multiple of 4
        Run(L(Case(1, 3, 5, kc, 12, relu=False, **kw)), pad0=(1, 3)),
    ]
    if ks == 3:
        even = ((th + 4) * s, (tw + 6) * s)
        runs += [Run(L(Case(1, rag[0], rag[1], 16, bn, c1=4, **kw)), pad0=(0, 16), pad1=(0, 4)),
                 Run(L(Case(1, one[0], one[1], 32, 12, c1=36, sign="pos", **kw))),
                 Run(L(Case(1, rag[0], rag[1], 13, bn + 8, sign="pos", **kw)), pad0=(0, 3))]
        if s == 1:
            runs += [Run(L(Case(1, even[0], even[1], 16, 36, c1=12, up0=True, **kw))),
                     Run(L(Case(1, even[0], even[1], 32, bn, c1=20, up0=True, sign="pos", relu=False, **kw)), pad0=(0, 4))]
    return runs


def taps_runs(tile, math):
    """dn_conv2d_taps: the four parity masks of dn_conv_dgrad_class_weights and every tap, into dx[:, py::2, px::2, :] --
    16-byte aligned (vector stores: opad 4) and at a 4-byte offset (scalar stores: opad 1); ragged maps"""
    ks, s, th, tw, bn, kc0, kc1 = TILES[tile]
    h, w = th + 3, tw + 5
    runs = []
    for i, ((py, px), mask) in enumerate(list(PARITY_MASKS.items()) + [((1, 0), FULL), ((1, 1), PARITY_MASKS[(1, 1)])]):
        sign = "pos" if i % 2 else "randn"
        runs.append(Run(Layer(Case(1, h, w, 20, 12 if i % 3 else bn + 8, relu=False, sign=sign), math, tap_mask=mask), "taps",
                        opad=((4, 4), (1, 7))[(i + (i == 5)) % 2], parity=(py, px)))
    return runs


def stuffed_runs(tile, math):
    """up0 = 2: source 0 read zero-stuffed -- an odd and an even source map, ragged against the tile"""
    ks, s, th, tw, bn, kc0, kc1 = TILES[tile]
    return [Run(Layer(Case(1, th + 6, tw + 6, 20, 12, up0=True, relu=False), math, stuffed=True)),
            Run(Layer(Case(1, th + 4, tw + 8, 32, bn + 8, up0=True, relu=False, sign="pos"), math, stuffed=True), pad0=(0, 4))]


def order_runs(tile, math):
    """the work-item decode (xcd_order = 2): spatial_items in {7, 8, 9, 17} x 1, 2, 3 channel blocks, ragged edges so
    that every item is distinguishable; 7 items run the remainder-only branch, 9 and 17 both branches"""
    ks, s, th, tw, bn, kc0, kc1 = TILES[tile]
    runs = []
    for items, (n, ty, tx) in ((7, (1, 1, 7)), (8, (2, 2, 2)), (9, (1, 3, 3)), (17, (1, 17, 1))):
        for ncb in (1, 2, 3):
            runs.append(Run(Layer(Case(n, ty * th - 3, tx * tw - 3, 16, ncb * bn - 24, sign="pos" if (items + ncb) % 2 else "randn"), math)))
    return runs


# more work items than resident workgroups (256 CUs x 2 or 3 by the tiles' LDS), 16 input channels, the smallest maps
# that get there: the record's grid is what the test asserts against
PERSISTENT = {
    "T3_256x32": Case(4, 200, 256, 16, 32, seed=1),               # 800 items of 8 x 32
    "T3_256x64": Case(4, 136, 256, 16, 64, c1=4, seed=1),         # 544; the concat layer: src_switch between two tiles
    "T3_128x64": Case(5, 128, 128, 16, 64, seed=1),               # 640 items of 8 x 16
    "T3_64x64": Case(5, 128, 128, 16, 64, seed=1),                # 1280 items of 8 x 8
    "T3S2_64x64": Case(5, 255, 255, 16, 64, stride=2, seed=1),    # 1280
    "T1_256x64": Case(4, 136, 256, 16, 64, k=1, seed=1),          # 544
}
LONG_K = Case(1, 8, 8, 512, 32, c1=256, up0=True)                  # conv5_1: 512 upsampled + 256 -> 32 on an 8 x 8 map


def forced_row(tile, math):
    ks, s = TILES[tile][:2]
    runs = std_runs(tile, math)
    if ks == 3 and s == 1:
        runs += taps_runs(tile, math) + stuffed_runs(tile, math)
    if tile in PERSISTENT and math == (0 if tile in ("T3_128x64", "T3S2_64x64", "T1_256x64") else 1):
        runs.append(Run(Layer(PERSISTENT[tile], math), persistent=True))
    if tile == "T3_256x32":
        runs += [Run(Layer(replace(LONG_K, sign=sign), math)) for sign in ("randn", "pos")]
    return Row("%s %s" % (tile, "f16x3" if math else "f32"), form_of(tile, math), tile, "forced", runs)


def post_runs():
    """dn_conv2d_post1x1: (c_out2, split) in {(64, 64), (48, 12), (4, 4)}, two outputs wider than their columns, relu2 on
    and off, maps of one tile, 3 x 5 and ragged, stage-1 K of one chunk, five and a partial one, a block-diagonal w2"""
    L = lambda case: Layer(case, 1)
    return [Run(L(Case(2, 8, 32, 16, 64, post=(64, 64, False, False), sign="pos")), "post"),
            Run(L(Case(1, 3, 5, 20, 64, post=(48, 12, True, True))), "post"),
            Run(L(Case(1, 11, 37, 80, 64, post=(4, 4, False, False), sign="pos")), "post"),
            Run(L(Case(1, 11, 37, 20, 64, post=(48, 12, False, True), sign="pos")), "post", pad0=(0, 12)),
            Run(L(Case(1, 11, 37, 16, 64, post=(64, 64, True, False), relu=False)), "post"),
            Run(L(Case(1, 8, 32, 80, 64, c1=4, post=(48, 12, False, False))), "post")]


ROWS = [forced_row(tile, math) for tile in TILES for math in (0, 1)]
ROWS += [
    Row("post1x1", POST_FORM, None, "dn_conv2d_post1x1 has one form", post_runs()),
    Row("work-item order f32", form_of("T3_64x64", 0), "T3_64x64", "forced", order_runs("T3_64x64", 0)),
    Row("work-item order f16x3", form_of("T3_128x64", 1), "T3_128x64", "forced", order_runs("T3_128x64", 1)),
]
# by shape: what the cost model itself selects (256 CUs; cost = ceil(blocks / 256) x tile area x bias, ties to the earlier)
for _m in (0, 1):
    _t = "f16x3" if _m else "f32"
    ROWS += [
        Row("T3_64x64 by shape " + _t, form_of("T3_64x64", _m), None, "one round for every tile: the smallest tile area wins",
            [Run(Layer(Case(1, 12, 20, 16, 32), _m))]),
        Row("T3_256x32 by shape " + _t, form_of("T3_256x32", _m), None,
            "c_out 32 on 65 tiles of 8 x 32: the 260 tiles of 8 x 8 need two rounds, the 64-wide tiles waste half their channels",
            [Run(Layer(Case(5, 100, 30, 16, 32, sign="pos"), _m))]),
        Row("T3_128x64 by shape " + _t, form_of("T3_128x64", _m), None,
            "maps 14 wide, c_out 64, 129 tiles of 8 x 16: 258 blocks of 8 x 32 x 32 or of 8 x 8 x 64 need two rounds",
            [Run(Layer(Case(3, 340, 14, 16, 64), _m))]),
        Row("T3S2_64x64 by shape " + _t, form_of("T3S2_64x64", _m), None, "stride 2 has one candidate",
            [Run(Layer(Case(1, 13, 21, 16, 32, stride=2, sign="pos"), _m))]),
        Row("T1_64x64 by shape " + _t, form_of("T1_64x64", _m), None, "one round for every tile: the smallest tile area wins",
            [Run(Layer(Case(1, 12, 20, 32, 64, k=1), _m))]),
        Row("T1_256x64 by shape " + _t, form_of("T1_256x64", _m), None,
            "c_out 64 on 195 tiles of 8 x 32: one round, where 780 tiles of 8 x 8 need four (a tie on cost, the earlier candidate)",
            [Run(Layer(Case(5, 100, 90, 16, 64, k=1, sign="pos"), _m))]),
        Row("T1_256x32 by shape " + _t, form_of("T1_256x32", _m), None,
            "c_out 32 on 129 tiles of 8 x 32: one round of half the area, where 516 tiles of 8 x 8 need three",
            [Run(Layer(Case(3, 340, 30, 16, 32, k=1), _m))]),
        Row("long K by shape " + _t, form_of("T3_64x64", _m), None, "an 8 x 8 map: one tile of 8 x 8",
            [Run(Layer(replace(LONG_K, sign=sign), _m)) for sign in ("randn", "pos")]),
    ]
ROWS.append(Row("T3_256x64 by shape f16x3", form_of("T3_256x64", 1), None,
                "c_out 64 on 129 tiles of 8 x 32: one round at bias 0.90, where the 32-channel and the 8 x 16 tiles need two and "
                "the 8 x 8 tile three (in fp32 its bias is 1.00 and it never beats T3_256x32 strictly)",
                [Run(Layer(Case(3, 340, 30, 16, 64), 1))]))
ROW = {r.name: r for r in ROWS}
assert len(ROW) == len(ROWS)


# --- the guard on the table itself (no GPU) ---------------------------------------------------------------
def _dispatch_forms():
    """every instantiation the product launches, read off conv_mfma.hip: the DN_CONV_CASE lines (both math modes each),
    the T3S2 case's two launches and the launch of dn_conv2d_post1x1"""
    with open(os.path.join(ROOT, "disconet_amd", "csrc", "conv_mfma.hip")) as f:
        text = f.read()
    forms = set()
    for m in re.finditer(r"^\s*DN_CONV_CASE\(\w+,\s*([0-9, ]+)\)", text, re.M):
        v = [int(t) for t in m.group(1).split(",")]
        for math in (0, 1):
            forms.add(tuple(v[:6]) + (math, 0))
    for m in re.finditer(r"\blaunch<([0-9, ]+)>\(a, \*d", text):
        v = [int(t) for t in m.group(1).split(",")] + [0, 0, 0]
        assert v[10] == 0, "an ablation kernel in the product's dispatch"
        forms.add(tuple(v[:6]) + (v[11], v[12]))
    return forms


def test_table_lists_every_form_of_the_dispatch():
    """every kernel instantiation conv2d_impl and dn_conv2d_post1x1 launch has a row (one added to the dispatch shows up
    here as missing): 9 ids x 2 math modes -- T3S2_64x64 with KC 8 and KC 16 -- and the one POST form, 19 in all.  The
    kernel's `KC == 8 && kSplit` branch (mfma_f32_32x32x8f16) is instantiated by none of them.  Every forced row holds both
    operand signs, ReLU on and off, and no row is skipped or expected to fail."""
    table = {r.form for r in ROWS}
    found = _dispatch_forms()
    assert len(found) == 19, sorted(found)
    assert not (found - table), sorted(found - table)
    assert not (table - found), sorted(table - found)
    assert not any(f[5] == 8 and f[6] == 1 for f in found)
    assert {form_of(t, m) for t in TILES for m in (0, 1)} | {POST_FORM} == found
    from disconet_amd import ops
    assert list(TILES) == sorted(ops.NHWC_CFG, key=ops.NHWC_CFG.get)
    for r in ROWS:
        if r.force is not None and r.why == "forced" and not r.name.startswith("work-item"):
            assert {run.layer.case.sign for run in r.runs} == {"randn", "pos"}, r.name
            assert {run.layer.case.relu for run in r.runs} == {True, False}, r.name
        for run in r.runs:
            assert N.family_of(run.layer) in N.C32, run
    for tile in PERSISTENT:
        assert any(run.persistent for m in (0, 1) for run in ROW["%s %s" % (tile, ("f32", "f16x3")[m])].runs), tile
    for name in ("test_form",):
        assert not [mk for mk in getattr(globals()[name], "pytestmark", []) if mk.name in ("skip", "skipif", "xfail")]


# --- running a row ------------------------------------------------------------------------------------
class _Wide:
    """`c` own columns of an NHWC tensor of c + before + after columns; the allocation has 64 floats of slack behind it, so
    the last chunk of the last pixel stays inside it wherever the columns start.  fill: the foreign columns' value, or
    None: every byte 0xFF"""
    def __init__(self, nhwc_shape, c, before, after, fill, own=None):
        n, h, w = nhwc_shape
        ld = before + c + after
        flat = torch.empty(n * h * w * ld + 64, dtype=torch.float32, device="cuda")
        if fill is None:
            flat.view(torch.int32).fill_(-1)
        else:
            flat.fill_(fill)
        self.wide = flat[:n * h * w * ld].view(n, h, w, ld)
        self.view = self.wide[..., before:before + c]
        self.ld, self.c, self.before = ld, c, before
        if own is not None:
            self.view.copy_(own)

    def untouched(self):
        b = self.wide.view(torch.int32)
        return bool((b[..., :self.before] == -1).all()) and bool((b[..., self.before + self.c:] == -1).all())


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().cuda()


def _nchw(t):
    return t.detach().cpu().permute(0, 3, 1, 2).double()


def run_one(run):
    """launch `run` -> (problems, err / (c A), form dict)"""
    from disconet_amd import ops
    layer = run.layer
    c, m = layer.case, C.make(layer.case)
    ref, cc = N.reference(layer), N.c_of(layer)
    problems = []
    s0 = _Wide((c.n,) + tuple(m.x0.shape[2:]), c.c0, run.pad0[0], run.pad0[1], 3e38, _nhwc(m.x0))
    s1 = _Wide((c.n, c.h, c.w), c.c1, run.pad1[0], run.pad1[1], 3e38, _nhwc(m.x1)) if c.c1 else None
    math = "f16x3" if layer.math else "f32"
    up0 = 2 if layer.stuffed else int(bool(c.up0))
    d = ops.conv_desc(c.n, c.h, c.w, c.c0, c.c_out, c.k, c.stride, c.relu, c1=c.c1, up0=up0, ld0=s0.ld,
                      ld1=s1.ld if s1 else None, math=math)
    packed = ops.pack_conv_weights(d, m.w1.cuda())      # the full weights: a masked tap's are there, and must not be used
    sc, sh = m.scale1.cuda(), m.shift1.cuda()
    ho, wo = ops.conv_out_hw(d)
    src1 = s1.view if s1 else None
    if run.entry == "post":
        c2, split, relu2, _ = c.post
        packed2 = ops.pack_post1x1_weights(m.w2.reshape(c2, 64).cuda())
        oa = _Wide((c.n, ho, wo), split, 0, 4, None)
        ob = _Wide((c.n, ho, wo), c2 - split, 0, 8, None) if split < c2 else None
        ops.conv2d_post1x1(d, s0.view, packed, sc, sh, packed2, m.scale2.cuda(), m.shift2.cuda(), c2, split, relu2,
                           oa.wide, ob.wide if ob else None, src1=src1)
        got = _nchw(oa.view if ob is None else torch.cat((oa.view, ob.view), -1))
        clean = oa.untouched() and (ob is None or ob.untouched())
    elif run.entry == "taps":
        py, px = run.parity
        dx = _Wide((c.n, 2 * ho, 2 * wo), c.c_out, run.opad[0], run.opad[1], None)
        d.ldo = dx.ld
        ops.conv2d_taps(d, s0.view, packed, sc, sh, dx.view[:, py::2, px::2, :], layer.tap_mask)
        got = _nchw(dx.view[:, py::2, px::2, :])
        b = dx.view.view(torch.int32)
        clean = dx.untouched() and all(bool((b[:, qy::2, qx::2, :] == -1).all()) for qy in (0, 1) for qx in (0, 1) if (qy, qx) != (py, px))
    else:
        o = _Wide((c.n, ho, wo), c.c_out, run.opad[0], run.opad[1], None)
        d.ldo = o.ld
        ops.conv2d(d, s0.view, packed, sc, sh, src1=src1, out=o.view)
        got = _nchw(o.view)
        clean = o.untouched()
    torch.cuda.synchronize()
    form = ops.nhwc_last_form()
    if not clean:
        problems.append("bytes outside the output's own columns / pixels were written")
    if form["entry"] != ENTRY[run.entry]:
        problems.append("entry point %d recorded, %d called" % (form["entry"], ENTRY[run.entry]))
    r = N.worst(got, ref, cc)
    if not r <= 1.0:
        err = torch.nan_to_num((got - ref.y).abs() / ref.A.clamp(min=1e-300), nan=float("inf"))
        k = int(err.argmax())
        problems.append("err / (c A) = %.3g (c = %.3e; %d NaN; worst element %s: got %r want %r A %r)"
                        % (r, cc, int(torch.isnan(got).sum()), tuple(int(v) for v in torch.unravel_index(torch.tensor(k), err.shape)),
                           float(got.reshape(-1)[k]), float(ref.y.reshape(-1)[k]), float(ref.A.reshape(-1)[k])))
    if run.persistent and not form["grid"] < form["total_items"]:
        problems.append("not a persistent-loop case: %d items on %d workgroups" % (form["total_items"], form["grid"]))
    return problems, r, form


def run_row(row):
    """-> (problems, worst ratio, its run): every run of the row under its force id, the recorded form checked after each"""
    from disconet_amd import ops
    problems, worst, at = [], 0.0, None
    want = dict(zip(FORM_KEYS, row.form))
    ops.nhwc_force_config(row.force)
    try:
        for run in row.runs:
            bad, r, form = run_one(run)
            got = {k: form[k] for k in FORM_KEYS}
            if got != want:
                bad.append("ran %r, the row is %r" % ({k: v for k, v in got.items() if v != want[k]},
                                                      {k: v for k, v in want.items() if v != got[k]}))
            if r >= worst:
                worst, at = r, run
            problems += ["%s: %s" % (run, b) for b in bad]
    finally:
        ops.nhwc_force_config(-1)
    return problems, worst, at


@pytest.mark.gpu
@pytest.mark.parametrize("name", [r.name for r in ROWS])
def test_form(name):
    problems, worst, at = run_row(ROW[name])
    print("FORM %-26s %3d runs, largest err / (c A) = %.3f  (%s)" % (name, len(ROW[name].runs), worst, at))
    assert not problems, "\n".join(problems)
