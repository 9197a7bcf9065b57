"""Every tile form the split-planar conv engine can launch, against the float64 reference of tests/conv_fp64.py, at the
shapes that reach each part of that form's kernel -- and named: after every launch ops.sp_last_form() (the record the
launchers themselves write, dn_spconv_last_form) must equal the row's form, so a change to the cost model or to a bias
that moves a form out of this file fails here instead of passing on another kernel.

One table (ROWS): form, how it is reached, cases.  Forms of the cost model's menu are pinned with
dn_spconv_force_config(id); forms the force switch disables -- the weight-stationary 8 x 32 x 32 tile, three weight
stages on the 8 x 8 tiles, the choices of conv_spq.hip and of the K-sliced launcher -- are reached by shape, and the row
says why the shape selects them.  Two forms depend on process-wide state read once (DN_SP_B3, dn_spconv_set_upmode) and
run in a child process.

Per case: output buffers pre-filled with 0xFF bytes (an unwritten piece is a NaN), |got - y| <= c A per element with
c = 4 c32 + 2^-21 (SP output) / 2^-22 (fp32 output) of the case's family (tests/conv_fp64.py), the range flags clean,
fp32 rows written into a channel slice of a wider tensor whose neighbours must keep their bytes.

Measured on the MI355X (47 rows, 305 launches; the file takes about 20 s, CPU references included): the largest
err / (c A) of each row, which every row also prints (pytest -s)
    S3_256x64 0.298        S3_256x32 0.353          S3_256x32 stationary 0.225   S3_128x64 0.298
    S3_64x64 NB3 0.231     S3_64x64 NB2 0.231       S3_64x64 forced 0.267        S3S2_128x64 0.374
    S3S2_64x64 NB3 0.346   S3S2_64x64 NB2 0.346     S3S2_64x64 forced 0.312      S3_256x64_T9 0.298
    S3_128x64_T9 0.298     S3_64x64_T9 0.353        S3S2_64x64_T9 0.312          S3S2_128x64_T9 0.374
    S3_64x64_T9 by shape 0.283   S3_512x64 0.301    S3_256x128 0.286
    S1_256x64 0.215        S1_64x64 0.205           S1_256x64_C1 0.220
    hi-only stationary 0.158     hi-only streaming 0.166    bit-grid 0.236
    POST1 streaming 0.161  POST1 stationary 0.153   POST2 heads 0.157
    KSL S3_256x32 0.335    KSL S3_128x64 / S3_64x64 / S3_64x64_T9 / S3_128x64_T9 0.111
    KSL S3S2_128x64 / S3S2_64x64 / S3S2_64x64_T9 / S3S2_128x64_T9 0.162
    SPQ BN32 0.337         SPQ BN32 by shape 0.203  SPQ BN64 0.276   SPQ BN64 by shape 0.138   SPQ deep 0.307
    SPQ KSL 0.288          SPQ KSL deep 0.107       UPM S3_256x32 0.279   UPM S3_128x64 0.257   stem pair 0.141
The one case that missed c = 4 c32 + 2^-21: the un-sliced 768-channel all-positive layer, 3.1e-6 A on the plain tiles
(1.34 x the c32 constant) and 3.0e-6 A on conv_spq (1.28 x) -- the rounding of one fp32 accumulator over 1296 MFMA
partials in sequence, not a lost term; that family is judged against the emulation's own distance from float64
(conv_fp64.E32, 0.35 above), its K-sliced form against c32 like everything else."""
import json
import os
import re
import subprocess
import sys
from dataclasses import dataclass

import pytest
import torch

from tests import conv_fp64 as C
from tests.conv_fp64 import Case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# enum SpCfgId of disconet_amd/csrc/conv_sp.hip, in its order: what dn_spconv_force_config takes
CFG = {"S3_256x64": 0, "S3_256x32": 1, "S3_128x64": 2, "S3_64x64": 3, "S3S2_128x64": 4, "S3S2_64x64": 5, "S1_256x64": 6,
       "S1_64x64": 7, "S3_256x64_T9": 8, "S3_512x64": 9, "S3_256x128": 10, "S1_256x64_C1": 11, "S3_256x32_ST": 12,
       "S3_64x64_T9": 13, "S3_128x64_T9": 14, "S3S2_64x64_T9": 15, "S3S2_128x64_T9": 16,
       # conv_spq.hip (spconv2d_impl): 20 = BN 32, 21 = BN 64, 22 = the one-step-per-chunk (DEEP) form
       "SPQ_32": 20, "SPQ_64": 21, "SPQ_DEEP": 22}

FORM_KEYS = ("family", "KS", "STRIDE", "TH", "TW", "BN", "TG", "CA", "POST", "BSTAT", "UPM", "AHI", "KSL", "NB", "DEEP")


def sp(KS=3, STRIDE=1, TH=8, TW=32, BN=64, TG=3, CA=1, POST=0, BSTAT=0, UPM=0, AHI=0, KSL=0, NB=2):
    """a conv_sp_kernel instantiation (family 0)"""
    return (0, KS, STRIDE, TH, TW, BN, TG, CA, POST, BSTAT, UPM, AHI, KSL, NB, 0)


def spq(BN=32, DEEP=0, KSL=0):
    """a conv_spq_kernel instantiation (family 1): the 8 x 32 tile, the quad-merged image (UPM 2)"""
    return (1, 3, 1, 8, 32, BN, 0, 1, 0, 0, 2, 0, KSL, 0, DEEP)


STEM = (2, 3, 1, 16, 32, 32, 0, 0, 0, 1, 0, 2, 0, 0, 0)      # conv_pre_pair_kernel


@dataclass(frozen=True)
class Run:
    """one launch: the layer, the epilogue ("sp" dn_spconv2d, "dual" dn_spconv2d_dual, "nhwc" dn_spconv2d_nhwc; fused
    stage: "sp" one SP output, "f32" fp32 output(s); stem: "sp"), K slices (dn_spconv2d_ks; ws: with a workspace, and
    then tiles must really be split), persistent: more than two rounds of work items per resident workgroup"""
    case: Case
    epi: str = "sp"
    kslices: int = 1
    ws: bool = True
    persistent: bool = False


@dataclass
class Row:
    name: str
    form: tuple
    force: object            # a key of CFG, or None: reached by shape (why says how)
    why: str
    runs: list
    child: str = ""          # "" / "b3" (DN_SP_B3=0) / "upm" (dn_spconv_set_upmode(1)): process-wide state, a child process
    tools_only: bool = False


# --- cases per form ------------------------------------------------------------------------------------
def std_runs(th, tw, bn, k=3, stride=1, ca=1, persistent=None, extra=()):
    """The smallest cases that reach each part of a (th x tw pixel, bn channel) tile: maps of exactly one tile, smaller
    than a tile (3 x 5) and ragged right and bottom (stride 2: odd input sizes); K loops of one A group (prologue = last
    step), two, five chunks (steady state) and a partial last chunk; c_out = bn, bn + 8 (a partial second block), 12, and
    1 (4 for fp32 rows); concat with both chunk parities (3x3); the three epilogues; both operand families.
    ca: chunks per A stage of the 1x1 tiles -- the chunk count stays a multiple, or the forced tile is not offered."""
    s = stride
    one = (th * s, tw * s)
    rag = ((th + 3) * s + (s - 1), (tw + 5) * s + (s - 1))
    k1, k2 = 16 * ca, 32 * ca
    k5 = {1: 80, 2: 96, 4: 128}[ca]
    p1, p2 = {1: (13, 40), 2: (24, 56), 4: (52, 120)}[ca]
    kw = dict(k=k, stride=stride)
    runs = [
        Run(Case(2, one[0], one[1], k1, bn, sign="pos", **kw), "sp"),
        Run(Case(1, 3, 5, p1, 12, **kw), "dual"),
        Run(Case(1, rag[0], rag[1], k2, bn + 8, **kw), "nhwc"),
        Run(Case(1, rag[0], rag[1], k5, 1, sign="pos", **kw), "sp"),
        Run(Case(2, rag[0], rag[1], p2, 4, relu=False, **kw), "nhwc"),
        Run(Case(1, one[0], one[1], k5, bn + 8, sign="pos", **kw), "dual"),
    ]
    if k == 3:
        runs += [Run(Case(1, rag[0], rag[1], 16, bn, c1=4, **kw), "sp"),
                 Run(Case(1, one[0], one[1], 48, 12, c1=36, sign="pos", **kw), "dual")]
    if persistent:
        n, h, w = persistent
        runs.append(Run(Case(n, h, w, k1, bn, seed=1, **kw), "sp", persistent=True))
    return runs + list(extra)


LONG_K = Case(1, 16, 16, 768, 32, sign="pos")                      # conv5_1's K at a 16 x 16 map
LONG_K_UP = Case(1, 16, 16, 512, 32, c1=256, up0=True, merge="quad", sign="pos")


def ks_runs(stride=1, extra=()):
    """K-sliced launches: 5 and 6 chunks in 4 slices (unequal shares), 3 chunks in 2; with a workspace (small launches
    are then split tile by tile: n_split > 0) and without (every tile whole); ragged maps, a partial channel block"""
    s = stride
    rag = (11 * s + (s - 1), 37 * s + (s - 1))
    kw = dict(stride=stride)
    return [Run(Case(1, rag[0], rag[1], 80, 72, sign="pos", **kw), "sp", 4, True),
            Run(Case(1, rag[0], rag[1], 80, 72, sign="pos", **kw), "sp", 4, False),
            Run(Case(2, 8 * s, 32 * s, 96, 64, **kw), "dual", 4, True),
            Run(Case(1, 3, 5, 40, 12, **kw), "sp", 2, True),
            Run(Case(1, rag[0], rag[1], 48, 12, c1=36, **kw), "nhwc", 2, False),
            Run(Case(1, rag[0], rag[1], 16, 64, c1=4, sign="pos", **kw), "sp", 2, True)] + list(extra)


def spq_runs(bn, persistent=None, ks=0, extra=()):
    """the quad-merged up-conv: even maps (the source is half the size), one tile, smaller, a ragged tile; one and three
    chunks of the upsampled source, none / a partial / three chunks of the second"""
    q = dict(up0=True, merge="quad")
    if ks:
        return [Run(Case(1, 12, 38, 48, bn + 8, c1=36, sign="pos", **q), "sp", 4, True),
                Run(Case(1, 12, 38, 48, bn + 8, c1=36, sign="pos", **q), "sp", 4, False),
                Run(Case(2, 8, 32, 80, bn, c1=16, **q), "dual", 4, True),
                Run(Case(1, 4, 6, 32, 12, c1=4, **q), "sp", 2, True),
                Run(Case(1, 12, 38, 16, 4, c1=36, relu=False, **q), "nhwc", 2, False)] + list(extra)
    runs = [Run(Case(2, 8, 32, 16, bn, sign="pos", **q), "sp"),
            Run(Case(1, 4, 6, 16, 12, c1=4, **q), "dual"),
            Run(Case(1, 12, 38, 48, bn + 8, c1=36, **q), "nhwc"),
            Run(Case(1, 12, 38, 16, 1, c1=4, sign="pos", **q), "sp"),
            Run(Case(2, 12, 38, 80, 4, relu=False, **q), "nhwc"),
            Run(Case(1, 8, 32, 48, bn + 8, c1=36, sign="pos", **q), "dual")]
    if persistent:
        n, h, w = persistent
        runs.append(Run(Case(n, h, w, 16, bn, seed=1, **q), "sp", persistent=True))
    return runs + list(extra)


def upm_runs(bn):
    q = dict(up0=True, merge="rows")
    return [Run(Case(2, 8, 32, 16, bn, sign="pos", **q), "sp"),
            Run(Case(1, 4, 6, 16, 12, c1=4, **q), "dual"),
            Run(Case(1, 12, 38, 48, bn + 8, c1=36, **q), "nhwc"),
            Run(Case(1, 12, 38, 80, 1, c1=4, sign="pos", **q), "sp"),
            Run(Case(1, 8, 16, 48, bn + 8, c1=36, sign="pos", **q), "dual")]


def src_runs(src, c_ins, c_outs):
    """hi-only / bit-grid sources: 3x3 stride-1 single-source layers"""
    (ka, kb, kc), (oa, ob, oc) = c_ins, c_outs
    return [Run(Case(2, 8, 32, ka, oa, src=src, sign="pos"), "sp"),
            Run(Case(1, 3, 5, kb, ob, src=src), "dual"),
            Run(Case(1, 11, 37, kc, oc, src=src), "sp"),
            Run(Case(2, 11, 37, kb, oa, src=src, sign="pos", relu=False), "dual"),
            Run(Case(5, 64, 128, ka, oa, src=src, seed=1), "sp")]


def post_runs(c_ins, block_diag=False):
    """the fused 1x1 stage behind a 64-channel 3x3: one SP output, one fp32 output, two fp32 outputs"""
    ka, kb, kc = c_ins
    if block_diag:       # the heads: two fp32 outputs, rows < split on hidden channels 0..31
        return [Run(Case(2, 8, 32, ka, 64, post=(48, 12, False, True), sign="pos"), "f32"),
                Run(Case(1, 3, 5, kb, 64, post=(8, 4, False, True)), "f32"),
                Run(Case(1, 11, 37, kc, 64, post=(64, 32, True, True)), "f32"),
                Run(Case(33, 64, 128, ka, 64, post=(48, 12, False, True), seed=1), "f32", persistent=True)]
    return [Run(Case(2, 8, 32, ka, 64, post=(48, 48, False, False), sign="pos"), "sp"),
            Run(Case(1, 3, 5, kb, 64, post=(12, 12, True, False)), "sp"),
            Run(Case(1, 11, 37, kc, 64, post=(1, 1, False, False), sign="pos"), "sp"),
            Run(Case(1, 11, 37, kb, 64, post=(64, 64, True, False)), "f32"),
            Run(Case(1, 11, 37, ka, 64, post=(48, 12, False, False), sign="pos"), "f32"),
            Run(Case(1, 8, 32, kc, 64, post=(8, 4, False, False)), "f32")]


STEM_RUNS = [Run(Case(2, 16, 32, 13, 32, src="bits", stem=32, sign="pos")),
             Run(Case(1, 5, 3, 7, 32, src="bits", stem=20)),
             Run(Case(1, 19, 37, 16, 32, src="bits", stem=32)),
             Run(Case(2, 19, 37, 13, 32, src="bits", stem=16, sign="pos")),
             Run(Case(33, 64, 128, 13, 32, src="bits", stem=32, seed=1), persistent=True)]

# resident workgroups are 256 CUs x 1..3: the persistent cases hold more than two rounds of items for every form that
# shares the tile (the launch's own record is what the test asserts against)
P_8x8, P_8x16, P_8x32, P_16x32 = (25, 64, 64), (25, 64, 128), (33, 64, 128), (33, 64, 128)
P_S2_8x8, P_S2_8x16 = (17, 128, 128), (17, 128, 128)

# shapes that make the cost model itself choose (256 CUs; cost = rounds x tile area x bias):
#  * c_out = 32 on >= 256 tiles of 8 x 32: S3_256x32 (half the channel block of the 64-wide tiles is wasted, and the
#    smaller pixel tiles need 2 / 4 rounds); two chunks of input fit the weight-stationary form beside a second workgroup
ST_RUNS = [Run(Case(4, 128, 128, 16, 32, sign="pos"), "sp"), Run(Case(4, 125, 123, 13, 32), "dual"),
           Run(Case(4, 125, 123, 32, 12), "nhwc"), Run(Case(4, 128, 128, 24, 1, sign="pos"), "sp"),
           Run(Case(4, 125, 123, 16, 4, c1=4, relu=False), "nhwc"),
           Run(Case(17, 128, 128, 16, 32, seed=1), "sp", persistent=True)]
#  * maps 8 pixels wide: the 8 x 16 and 8 x 32 tiles waste half / three quarters of their pixels, so the 8 x 8 tile
#    wins; more than 256 work items, so the all-nine-taps variant is not swapped in
B3_RUNS = [Run(Case(33, 64, 8, 16, 64, sign="pos"), "sp"), Run(Case(33, 61, 7, 13, 64), "dual"),
           Run(Case(33, 61, 7, 80, 64), "nhwc"), Run(Case(20, 61, 7, 40, 72, sign="pos"), "sp"),
           Run(Case(33, 64, 8, 16, 64, c1=4), "sp"), Run(Case(200, 64, 8, 16, 64, seed=1), "sp", persistent=True)]
B3S2_RUNS = [Run(Case(33, 128, 16, 16, 64, stride=2, sign="pos"), "sp"), Run(Case(33, 123, 15, 13, 64, stride=2), "dual"),
             Run(Case(33, 123, 15, 80, 64, stride=2), "nhwc"), Run(Case(20, 123, 15, 40, 72, stride=2, sign="pos"), "sp"),
             Run(Case(33, 128, 16, 16, 64, c1=4, stride=2), "sp"),
             Run(Case(140, 128, 16, 16, 64, stride=2, seed=1), "sp", persistent=True)]

ROWS = [
    # ---- conv_sp, plain 3x3
    Row("S3_256x64", sp(), "S3_256x64", "forced", std_runs(8, 32, 64, persistent=P_8x32)),
    Row("S3_256x32", sp(BN=32), "S3_256x32", "forced (a forced id never takes the stationary form)",
        std_runs(8, 32, 32, persistent=P_8x32, extra=[Run(LONG_K, "sp")])),
    Row("S3_256x32 stationary", sp(BN=32, BSTAT=1), None, "c_out <= 32 on >= 256 tiles of 8 x 32, <= 2 chunks", ST_RUNS),
    Row("S3_128x64", sp(TW=16), "S3_128x64", "forced", std_runs(8, 16, 64, persistent=P_8x16)),
    Row("S3_64x64 NB3", sp(TW=8, NB=3), None, "maps 8 pixels wide, > 256 work items", B3_RUNS),
    Row("S3_64x64 NB2", sp(TW=8), None, "the same shapes under DN_SP_B3=0", B3_RUNS, child="b3"),
    Row("S3_64x64 forced", sp(TW=8), "S3_64x64", "forced (two weight stages)", std_runs(8, 8, 64)),
    Row("S3S2_128x64", sp(STRIDE=2, TW=16), "S3S2_128x64", "forced", std_runs(8, 16, 64, stride=2, persistent=P_S2_8x16)),
    Row("S3S2_64x64 NB3", sp(STRIDE=2, TW=8, NB=3), None, "output maps 8 pixels wide, > 256 work items", B3S2_RUNS),
    Row("S3S2_64x64 NB2", sp(STRIDE=2, TW=8), None, "the same shapes under DN_SP_B3=0", B3S2_RUNS, child="b3"),
    Row("S3S2_64x64 forced", sp(STRIDE=2, TW=8), "S3S2_64x64", "forced (two weight stages)",
        std_runs(8, 8, 64, stride=2, persistent=P_S2_8x8)),
    Row("S3_256x64_T9", sp(TG=9), "S3_256x64_T9", "forced", std_runs(8, 32, 64, persistent=P_8x32)),
    Row("S3_128x64_T9", sp(TW=16, TG=9), "S3_128x64_T9", "forced", std_runs(8, 16, 64, persistent=P_8x16)),
    Row("S3_64x64_T9", sp(TW=8, TG=9), "S3_64x64_T9", "forced", std_runs(8, 8, 64, persistent=P_8x8, extra=[Run(LONG_K, "sp")])),
    Row("S3S2_64x64_T9", sp(STRIDE=2, TW=8, TG=9), "S3S2_64x64_T9", "forced", std_runs(8, 8, 64, stride=2, persistent=P_S2_8x8)),
    Row("S3S2_128x64_T9", sp(STRIDE=2, TW=16, TG=9), "S3S2_128x64_T9", "forced", std_runs(8, 16, 64, stride=2, persistent=P_S2_8x16)),
    Row("S3_64x64_T9 by shape", sp(TW=8, TG=9), None, "<= 256 work items: the deep variant of the cheapest tile",
        [Run(Case(2, 32, 32, 32, 64), "sp"), Run(Case(1, 16, 16, 80, 64, sign="pos"), "dual")]),
    Row("S3_512x64", sp(TH=16), "S3_512x64", "forced; no product path", std_runs(16, 32, 64, persistent=P_16x32), tools_only=True),
    Row("S3_256x128", sp(BN=128), "S3_256x128", "forced; no product path", std_runs(8, 32, 128, persistent=(17, 64, 128)),
        tools_only=True),
    # ---- 1x1
    Row("S1_256x64", sp(KS=1, TG=1, CA=2), "S1_256x64", "forced; even chunk counts", std_runs(8, 32, 64, k=1, ca=2, persistent=P_8x32)),
    Row("S1_64x64", sp(KS=1, TW=8, TG=1, CA=4), "S1_64x64", "forced; chunk counts that are multiples of 4",
        std_runs(8, 8, 64, k=1, ca=4, persistent=P_8x8)),
    Row("S1_256x64_C1", sp(KS=1, TG=1), "S1_256x64_C1", "forced; any chunk count", std_runs(8, 32, 64, k=1, persistent=P_8x32)),
    # ---- hi-only and bit-grid sources: spconv2d_impl takes them before the cost model
    Row("hi-only stationary", sp(BN=32, BSTAT=1, AHI=1), None, "hi-only source, <= 3 chunks and c_out <= 32: the weights fit",
        src_runs("hi", (16, 13, 40), (32, 12, 1))),
    Row("hi-only streaming", sp(BN=32, AHI=1), None, "hi-only source, c_out > 32 or >= 4 chunks",
        src_runs("hi", (16, 13, 80), (40, 64, 32))),
    Row("bit-grid", sp(BN=32, BSTAT=1, AHI=2), None, "bit-grid source (<= 32 channels, c_out <= 32)",
        src_runs("bits", (16, 13, 29), (32, 12, 1))),
    # ---- fused 1x1 stage
    Row("POST1 streaming", sp(POST=1), None, ">= 3 chunks of input: the weights do not fit beside the second stage",
        post_runs((48, 40, 80))),
    Row("POST1 stationary", sp(POST=1, BSTAT=1), None, "<= 2 chunks of input", post_runs((16, 13, 32))),
    Row("POST2 heads", sp(POST=2), None, "block-diagonal second stage", post_runs((16, 40, 80), block_diag=True)),
    # ---- K-sliced conv_sp
    Row("KSL S3_256x32", sp(BN=32, KSL=1), "S3_256x32", "forced", ks_runs(extra=[Run(LONG_K, "sp", 4, True)])),
    Row("KSL S3_128x64", sp(TW=16, KSL=1), "S3_128x64", "forced", ks_runs()),
    Row("KSL S3_64x64", sp(TW=8, KSL=1), "S3_64x64", "forced", ks_runs()),
    Row("KSL S3_64x64_T9", sp(TW=8, TG=9, KSL=1), None, "small launches: even the slices leave CUs idle -> the deep variant",
        ks_runs()),
    Row("KSL S3_128x64_T9", sp(TW=16, TG=9, KSL=1), "S3_128x64_T9", "forced", ks_runs()),
    Row("KSL S3S2_128x64", sp(STRIDE=2, TW=16, KSL=1), "S3S2_128x64", "forced", ks_runs(stride=2)),
    Row("KSL S3S2_64x64", sp(STRIDE=2, TW=8, KSL=1), "S3S2_64x64", "forced", ks_runs(stride=2)),
    Row("KSL S3S2_64x64_T9", sp(STRIDE=2, TW=8, TG=9, KSL=1), None, "small stride-2 launches -> the deep variant", ks_runs(stride=2)),
    Row("KSL S3S2_128x64_T9", sp(STRIDE=2, TW=16, TG=9, KSL=1), "S3S2_128x64_T9", "forced", ks_runs(stride=2)),
    # ---- conv_spq: the default form of a layer whose first source is upsampled
    Row("SPQ BN32", spq(32), "SPQ_32", "forced", spq_runs(32, persistent=(33, 64, 128), extra=[Run(LONG_K_UP, "sp")])),
    Row("SPQ BN32 by shape", spq(32), None, "c_out = 32 on 288 tiles: more items than CUs, fewer than BN = 64 asks for",
        [Run(Case(9, 64, 128, 16, 32, c1=4, up0=True, merge="quad"), "sp")]),
    Row("SPQ BN64", spq(64), "SPQ_64", "forced", spq_runs(64)),
    Row("SPQ BN64 by shape", spq(64), None, "c_out = 64 on 1056 tiles (>= 4 x 256 items of 64 channels)",
        [Run(Case(33, 64, 128, 16, 64, up0=True, merge="quad", seed=1), "sp", persistent=True)]),
    Row("SPQ deep", spq(32, DEEP=1), None, "<= 256 work items", spq_runs(32)),
    Row("SPQ KSL", spq(32, KSL=1), "SPQ_32", "forced", spq_runs(32, ks=1, extra=[Run(LONG_K_UP, "sp", 4, True)])),
    Row("SPQ KSL deep", spq(32, DEEP=1, KSL=1), None, "small launches: tiles x slices <= 256", spq_runs(32, ks=1)),
    # ---- the row-merged up-conv image (dn_spconv_set_upmode(1)): another packed image for the whole process
    Row("UPM S3_256x32", sp(BN=32, UPM=1), "S3_256x32", "forced, upmode 1", upm_runs(32), child="upm"),
    Row("UPM S3_128x64", sp(TW=16, UPM=1), "S3_128x64", "forced, upmode 1", upm_runs(64), child="upm"),
    # ---- the stem pair
    Row("stem pair", STEM, None, "dn_spconv2d_pre_pair", STEM_RUNS),
]
ROW = {r.name: r for r in ROWS}
assert len(ROW) == len(ROWS)

# instantiations of the dispatch no call can reach: spconv2d_impl's row-merged switch lists S3_256x64, which select_cfg
# never returns for a row-merged layer (its candidates are S3_256x32 and S3_128x64, forced or not)
UNREACHABLE = {sp(UPM=1)}


# --- the guard on the table itself (no GPU) ---------------------------------------------------------------
def _dispatch_forms():
    """every non-ablation instantiation the three launchers are called with, read off the sources: conv_sp.hip's tile
    table (the SP_TILE rows), its form definitions (struct NAME : BASE { static constexpr int FLAG = v; }) and the
    launch_form<FORM, tiles...> call sites that pair them; conv_spq.hip's launch_spq<...> lists"""
    forms = set()
    csrc = os.path.join(ROOT, "disconet_amd", "csrc")
    with open(os.path.join(csrc, "conv_sp.hip")) as f:
        text = f.read()
    tiles = {}
    for m in re.finditer(r"^SP_TILE\((\w+),[^,]+,\s*\w+,\s*(?:Geom<([0-9, ]+)>|Tile<(\w+)>::G)\);", text, re.M):
        tiles[m.group(1)] = [int(t) for t in m.group(2).split(",")] if m.group(2) else tiles[m.group(3)]
    assert {k: i for i, k in enumerate(tiles)} == {k: v for k, v in CFG.items() if v < len(tiles)}, list(tiles)
    flags = {}
    for m in re.finditer(r"^struct (\w+)(?: : (\w+))? \{ static constexpr int ([^;]+); \};", text, re.M):
        flags[m.group(1)] = dict(flags[m.group(2)]) if m.group(2) else {}
        flags[m.group(1)].update((k.strip(), int(v)) for k, v in (kv.split("=") for kv in m.group(3).split(",")))
    for m in re.finditer(r"\blaunch_form<(\w+), ([\w,\s]+)>\(", text):
        if m.group(1) == "F":            # the helpers themselves; ablations go through launch_ablation<>
            continue
        f = flags[m.group(1)]
        assert f["ABL"] == 0, m.group(0)
        for tile in m.group(2).split(","):
            ks, st, th, tw, bn, tg, ca = tiles[tile.strip()][:7]
            forms.add(sp(ks, st, th, tw, bn, tg, ca, f["POST"], f["BSTAT"], f["UPM"], f["AHI"], f["KSL"], f["NB"]))
    with open(os.path.join(csrc, "conv_spq.hip")) as f:
        text = f.read()
    for m in re.finditer(r"\blaunch_spq<([0-9, ]+)>\(a, stream", text):
        v = [int(t) for t in m.group(1).split(",")] + [0, 0, 0]
        if v[2] == 0:
            forms.add(spq(v[0], v[1], v[3]))
    forms.add(STEM)
    return forms


def test_table_lists_every_form_of_the_dispatch():
    """every kernel instantiation the launchers of conv_sp.hip / conv_spq.hip / conv_pre_pair.inl are called with has a
    row (a form added to the dispatch shows up here as missing), the forms the issue names are present by name, and
    every row holds both operand families"""
    table = {r.form for r in ROWS}
    found = _dispatch_forms()
    assert len(found) == 43, len(found)
    missing = found - table - UNREACHABLE
    assert not missing, sorted(missing)
    assert not (table - found), sorted(table - found)
    for name in ("S3_256x64", "S3_256x32", "S3_256x32 stationary", "S3_128x64", "S3_64x64 NB3", "S3_64x64 NB2", "S3S2_128x64",
                 "S3S2_64x64 NB3", "S3_256x64_T9", "S3_128x64_T9", "S3_64x64_T9", "S3S2_64x64_T9", "S3S2_128x64_T9", "S3_512x64",
                 "S3_256x128", "S1_256x64", "S1_64x64", "S1_256x64_C1", "hi-only stationary", "hi-only streaming", "bit-grid",
                 "POST1 streaming", "POST1 stationary", "POST2 heads", "KSL S3_64x64", "SPQ BN32", "SPQ BN64", "SPQ deep", "SPQ KSL",
                 "SPQ KSL deep", "UPM S3_256x32", "UPM S3_128x64", "stem pair"):
        assert name in ROW, name
    for r in ROWS:
        signs = {run.case.sign for run in r.runs}
        assert signs == {"randn", "pos"} or len(r.runs) == 1, (r.name, signs)
        for run in r.runs:
            assert C.family_of(run.case) in C.C32
    assert sum(len(r.runs) for r in ROWS) <= 330


# --- running a row ------------------------------------------------------------------------------------
def _nan_sp(ops, n, h, w, c):
    t = ops.SpTensor(n, h, w, c, device="cuda")
    t.data.view(torch.int16).fill_(-1)              # 0xFF bytes: every half a NaN
    return t


class _Rows:
    """fp32 NHWC rows of c channels inside a wider tensor (4 floats either side), all 0xFF bytes before the launch"""
    def __init__(self, n, h, w, c):
        self.wide = torch.empty(n, h, w, c + 8, dtype=torch.float32, device="cuda")
        self.wide.view(torch.int32).fill_(-1)
        self.view = self.wide[..., 4:4 + c]
        self.c = c

    def untouched(self):
        b = self.wide.view(torch.int32)
        return bool((b[..., :4] == -1).all()) and bool((b[..., 4 + self.c:] == -1).all())


def _nchw(t):
    return t.detach().cpu().permute(0, 3, 1, 2).double()


def _source(ops, m):
    c = m.case
    x = m.x0.permute(0, 2, 3, 1).contiguous()
    if c.src == "bits":
        words = (x.to(torch.int64) << torch.arange(c.c0, dtype=torch.int64)).sum(-1)
        words = torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32)
        return ops.SpTensor(c.n, x.shape[1], x.shape[2], c.c0, device="cuda", bits=True, data=words.cuda())
    full = ops.SpTensor.from_nhwc(x.cuda())
    if c.src == "hi":
        return ops.SpTensor(c.n, x.shape[1], x.shape[2], c.c0, device="cuda", hi_only=True, data=full.data[:, :, :2].contiguous())
    return full


def run_one(run):
    """launch `run` -> (problems, worst err / (c A), form dict)"""
    import ctypes
    from disconet_amd import ops, _lib
    lib = _lib.load()
    c, m = run.case, C.make(run.case)
    ref = C.reference(c)
    ptr, st = ops._ptr, ops._stream
    problems, ratios = [], []
    ops.sp_range_flags(reset=True)

    def judge(what, got, out_f32):
        cc = C.c_of(c, out_f32, run.kslices)
        r = C.worst(got, ref, cc)
        ratios.append(r)
        if not r <= 1.0:
            err = (got - ref.y).abs()
            k = int(torch.nan_to_num(err / ref.A.clamp(min=1e-300), nan=float("inf")).argmax())
            problems.append("%s: err / (c A) = %.3g (c = %.3e; worst element %s: got %r want %r A %r)"
                            % (what, r, cc, tuple(int(v) for v in torch.unravel_index(torch.tensor(k), err.shape)),
                               float(got.reshape(-1)[k]), float(ref.y.reshape(-1)[k]), float(ref.A.reshape(-1)[k])))

    src0 = _source(ops, m)
    src1 = ops.SpTensor.from_nhwc(m.x1.permute(0, 2, 3, 1).contiguous().cuda()) if c.c1 else None
    p1 = ptr(src1.data) if src1 is not None else None
    d = ops.conv_desc(c.n, c.h, c.w, c.c0, c.c_out, c.k, c.stride, c.relu, c1=c.c1, up0=c.up0, math="sp")
    packed, wmul = ops.sp_pack_conv_weights(d, m.w1.cuda())
    assert wmul == m.wmul1
    sc, sh = (m.scale1 / wmul).cuda(), m.shift1.cuda()
    ho, wo = ops.conv_out_hw(d)
    if c.stem:
        d2 = ops.conv_desc(c.n, c.h, c.w, 32, c.stem, 3, 1, True, math="sp")
        packed2, wmul2 = ops.sp_pack_conv_weights(d2, m.w2.cuda())
        assert wmul2 == m.wmul2 and ops.sp_conv2d_pre_pair_supported(d, d2)
        out = _nan_sp(ops, c.n, c.h, c.w, c.stem)
        sc2, sh2 = (m.scale2 / wmul2).cuda(), m.shift2.cuda()
        ops.sp_conv2d_pre_pair(d, d2, src0, packed, sc, sh, packed2, sc2, sh2, out=out)
        judge("SP", _nchw(out.nhwc()), False)
    elif c.post:
        c2, split, relu2, block_diag = c.post
        w2 = m.w2.reshape(c2, 64).cuda()
        packed2, wmul2 = ops.sp_pack_heads_weights(w2, split) if block_diag else ops.sp_pack_post1x1_weights(w2)
        assert wmul2 == m.wmul2
        sc2, sh2 = (m.scale2 / wmul2).cuda(), m.shift2.cuda()
        if run.epi == "sp":
            out = _nan_sp(ops, c.n, ho, wo, c2)
            ops.sp_conv2d_post1x1(d, src0, packed, sc, sh, packed2, sc2, sh2, c2, split, relu2, out)
            judge("SP", _nchw(out.nhwc()), False)
        else:
            out_a = torch.empty(c.n, ho, wo, split, device="cuda")
            out_a.view(torch.int32).fill_(-1)
            out_b = None
            if split < c2:
                out_b = torch.empty(c.n, ho, wo, c2 - split, device="cuda")
                out_b.view(torch.int32).fill_(-1)
            ops.sp_conv2d_post1x1(d, src0, packed, sc, sh, packed2, sc2, sh2, c2, split, relu2, out_a, out_b, block_diag=block_diag)
            judge("fp32", _nchw(out_a if out_b is None else torch.cat((out_a, out_b), -1)), True)
    else:
        if c.src == "hi":
            d.math = 3
        elif c.src == "bits":
            d.math = 4
        out = _nan_sp(ops, c.n, ho, wo, c.c_out) if run.epi != "nhwc" else None
        rows = _Rows(c.n, ho, wo, c.c_out) if run.epi != "sp" else None
        po = ptr(out.data) if out is not None else None
        pr, ld = (ptr(rows.view), rows.wide.stride(2)) if rows is not None else (None, 0)
        if run.kslices > 1:
            assert lib.dn_spconv_ks_supported(ctypes.byref(d), run.kslices)
            nb = int(lib.dn_spconv_workspace_bytes(ctypes.byref(d), run.kslices)) if run.ws else 0
            ws = torch.empty(max(nb, 16), dtype=torch.uint8, device="cuda")
            ops.check(lib.dn_spconv2d_ks(ctypes.byref(d), run.kslices, ptr(src0.data), p1, ptr(packed), ptr(sc), ptr(sh), po, pr, ld,
                                         ptr(ws) if run.ws else None, nb, st()), "dn_spconv2d_ks")
        elif run.epi == "sp":
            ops.check(lib.dn_spconv2d(ctypes.byref(d), ptr(src0.data), p1, ptr(packed), ptr(sc), ptr(sh), po, st()), "dn_spconv2d")
        elif run.epi == "dual":
            ops.check(lib.dn_spconv2d_dual(ctypes.byref(d), ptr(src0.data), p1, ptr(packed), ptr(sc), ptr(sh), po, pr, ld, st()),
                      "dn_spconv2d_dual")
        else:
            ops.check(lib.dn_spconv2d_nhwc(ctypes.byref(d), ptr(src0.data), p1, ptr(packed), ptr(sc), ptr(sh), pr, ld, st()),
                      "dn_spconv2d_nhwc")
        if out is not None:
            judge("SP", _nchw(out.nhwc()), False)
        if rows is not None:
            judge("fp32 rows", _nchw(rows.view), True)
            if not rows.untouched():
                problems.append("the fp32 rows' neighbours in the wider tensor were written")
    torch.cuda.synchronize()
    form = ops.sp_last_form()
    flags = ops.sp_range_flags(reset=True)
    if flags & 5:
        problems.append("range flags %d" % flags)
    if run.kslices > 1:
        if run.ws and not form["n_split"] > 0:
            problems.append("a workspace was given and no tile was split (n_whole %d)" % form["n_whole"])
        if not run.ws and form["n_split"] != 0:
            problems.append("no workspace, yet %d tiles split" % form["n_split"])
        if form["n_whole"] + form["n_split"] * run.kslices != form["total_items"]:
            problems.append("K-slice plan does not add up: %r" % form)
    if run.persistent and not form["total_items"] > 2 * form["grid"]:
        problems.append("not a persistent-loop case: %d items on %d workgroups" % (form["total_items"], form["grid"]))
    return problems, max(ratios), form


def run_row(row):
    """-> (problems, worst ratio): every run of the row under its force id, the recorded form checked after each"""
    from disconet_amd import _lib
    lib = _lib.load()
    problems, worst = [], 0.0
    want = dict(zip(FORM_KEYS, row.form))
    lib.dn_spconv_force_config(-1 if row.force is None else CFG[row.force])
    try:
        for run in row.runs:
            bad, r, form = run_one(run)
            got = {k: form[k] for k in FORM_KEYS}
            if got != want:
                bad.append("ran %r, the row is %r" % ({k: v for k, v in got.items() if v != want[k]},
                                                      {k: v for k, v in want.items() if v != got[k]}))
            worst = max(worst, r)
            problems += ["%s: %s" % (run, b) for b in bad]
    finally:
        lib.dn_spconv_force_config(-1)
    return problems, worst


def child_main(kind):
    """the rows that need process-wide state, in a process of their own: prints one JSON line"""
    from disconet_amd import _lib
    if kind == "upm":
        _lib.load().dn_spconv_set_upmode(1)
    out = {}
    for row in ROWS:
        if row.child == kind:
            problems, worst = run_row(row)
            out[row.name] = {"problems": problems, "worst": worst}
    print("ROWS_JSON " + json.dumps(out))


@pytest.mark.gpu
@pytest.mark.parametrize("name", [r.name for r in ROWS if not r.child])
def test_form(name):
    problems, worst = run_row(ROW[name])
    print("FORM %-24s %3d runs, largest err / (c A) = %.3f" % (name, len(ROW[name].runs), worst))
    assert not problems, "\n".join(problems)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["b3", "upm"])
def test_forms_of_a_child_process(kind):
    """DN_SP_B3 is read once and dn_spconv_set_upmode changes the packed image of the process: their forms run in a
    child (one per kind), which reports every row"""
    env = dict(os.environ, DN_SP_B3="0") if kind == "b3" else dict(os.environ)
    code = "from tests.test_gpu_conv_fp64 import child_main; child_main(%r)" % kind
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("ROWS_JSON ")][0]
    res = json.loads(line[len("ROWS_JSON "):])
    assert sorted(res) == sorted(r.name for r in ROWS if r.child == kind)
    for name, v in res.items():
        print("FORM %-24s %3d runs, largest err / (c A) = %.3f" % (name, len(ROW[name].runs), v["worst"]))
    bad = ["%s: %s" % (name, p) for name, v in res.items() for p in v["problems"]]
    assert not bad, "\n".join(bad)
