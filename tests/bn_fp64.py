"""A float64 reference of the BatchNorm training kernels (disconet_amd/csrc/train_ops.hip: statistics, running update, apply,
backward reduce, backward apply, the folds and the channel sums), a CPU emulation of the kernels' own arithmetic with switches
that break one rule each on purpose, the bound that separates the two, and the seeded cases the BatchNorm tests share.  Plain
torch on the CPU, no GPU import.  TEST infrastructure: tests/test_bn_fp64_cpu.py shows on the CPU that the faithful emulation
passes the bound, that every mutant fails it on the cases that name it and that every kernel of the unit's BatchNorm half is
named by a case; tests/test_gpu_bn_fp64.py holds every kernel to the same bound and the launch record
(dn_bn_train_last_form) to the case's claim.

Operands as stored.  Every reference is float64 ON THE FP32 VALUES THE LAUNCH WAS GIVEN: the apply and the backward are judged
on the fp32 mean / var / gamma / beta (and y or the byte mask as the gate), the running update on the fp32 statistics, a
two-rank launch on the float64 sums of the other rank that `sync` handed it -- so a bound judges one kernel, not its inputs.

The bound.  |got - ref| <= c A per element, an element with A = 0 must be exactly 0 (conv_fp64.worst).
  statistics   A_mean = 2^-24 |mean| + rows 2^-53 E|z|,  A_var = 2^-24 var + rows 2^-53 (E[z^2] + mean^2),  c = MARGIN: one fp32
               rounding of the result plus the worst case of a double sum of `rows` terms in any order.
  apply        y = zhat gamma + beta (then the ReLU), A = |zhat gamma| + |beta|
  backward     g = (dy_a [2 x 2 block sum | space-to-depth read] + dy_b) gate, S1 = sum g, S2 = sum g zhat over the group's rows,
               dbeta = sum over groups of S1, dgamma = of S2, dz = gamma rstd (g - S1 / norm_rows - zhat S2 / norm_rows);
               A_dz = |gamma| rstd (|g| + |S1 / norm_rows| + |zhat S2 / norm_rows|), A_dbeta = sum |g|, A_dgamma = sum |g zhat|;
               accumulate adds |old| to A and one fp32 rounding (2^-24) to c
  bias         the sum of the fp32 dz the same launch wrote, A = sum |dz|
  running      the momentum recurrence in float64 in the order given, A the same recurrence on absolute values
  c = MARGIN * yard (MARGIN is conv_fp64's), yard = what a plain float32 CPU evaluation of the same formulas (torch float32
  ops, double sums where the kernel has double sums) loses against the float64 reference, normalised by A, per (output, value
  family): YARD below, `python -m tests.bn_fp64` prints the table.
The SP copies (y_sp, dz_sp) and the byte mask are judged in tests/test_gpu_bn_fp64.py from the fp32 tensor the same launch
wrote (sp_bytes, mask_of below); the mask's bits against the reference wherever |y_ref| > c A (mask_free_share).

The emulation.  fp32 element operations; the fused multiply-adds that bn_fwd_element, bn_bwd_element and bn_stats_finish spell out
taken as float64 and rounded; every product of bn_running_step rounded; sums in float64 (their order is free: double); m1, m2
rounded to fp32; the bias form's in-thread fp32 sum in loop order, then double."""
import os
import re
import zlib
from dataclasses import dataclass
from functools import lru_cache
from types import SimpleNamespace

import numpy as np
import torch

from tests import sp_format
from tests.conv_fp64 import MARGIN, Ref, worst  # noqa: F401

EPS = 1e-5
P21, P24, P53 = 2.0 ** -21, 2.0 ** -24, 2.0 ** -53
POISON = 7.0                       # what the slack of a strided operand holds (and every output before the launch)
MASK_FREE_CAP = 1e-3               # share of a case's mask bits that may lie inside the band |y_ref| <= c A
SP_LIFT = 2.0 ** 9                 # dz ~ 1e-3 gamma rstd: the lifted copy stays far below 65504


# --- the host dispatch, restated (tests/test_gpu_bn_fp64.py holds the launch record to it) -------------------------------
def lanes_for(c):
    t = 1
    while t < c and t < 64:
        t *= 2
    return t


def blocks_per_group(rows, groups):
    """workgroups per group of a reduction: ~1024 over all groups, at least 64 rows each"""
    return max(1, min(1024 // groups, rows // 64))


def grid_for(total, cap):
    return max(1, min((total + 255) // 256, cap))


def class_of(groups, rows, c, aligned=True):
    """general | vec4 | fast: bn_form's rule (aligned: every pointer on 16 bytes and every row stride % 4 == 0)"""
    if c % 4 or not aligned:
        return "general"
    c4 = c // 4
    return "fast" if groups == 1 and c <= 512 and c4 & (c4 - 1) == 0 and rows * c // 4 < 2 ** 31 else "vec4"


CLS = {"general": 0, "vec4": 1, "fast": 2}
REC_SP, REC_BIAS, REC_MASK, REC_DZ_NULL, REC_RUNNING, REC_ORDER = 1, 2, 4, 8, 16, 32
FOLD_NONE, FOLD_FINALIZE, FOLD_STATS_FINISH, FOLD_PARAM_GRAD, FOLD_PARTIALS_PARAM_GRAD, FOLD_CHANNEL_SUM, FOLD_DEFERRED = range(7)

# every kernel of the unit's BatchNorm half as the host code instantiates it; the U = 1 reductions are DN_BN_LEGACY's (covered by
# the child-process A/B test of tests/test_gpu_train_ops.py, not here)
LEGACY_KERNELS = ("bn_stats_v4_kernel<1>", "bn_bwd_reduce_v4_kernel<1>", "channel_sum_v4_kernel<1>")
BN_KERNELS = ("fold_partials_kernel", "bn_stats_finalize_kernel", "bn_update_running_kernel", "bn_param_grad_kernel",
              "fold_stats_finish_kernel", "fold_param_grad_kernel", "fold_channel_sum_kernel", "fold_channel_sum_multi_kernel",
              "bn_apply_kernel", "bn_apply_v4_kernel", "bn_apply_v4_fast_kernel<false>", "bn_apply_v4_fast_kernel<true>",
              "bn_stats_kernel", "bn_stats_v4_kernel<4>", "bn_bwd_reduce_kernel", "bn_bwd_reduce_v4_kernel<2>",
              "channel_sum_kernel", "channel_sum_v4_kernel<4>", "bn_bwd_apply_kernel", "bn_bwd_apply_v4_kernel<false>",
              "bn_bwd_apply_v4_kernel<true>", "bn_bwd_apply_v4_fast_kernel<false, false>", "bn_bwd_apply_v4_fast_kernel<true, false>",
              "bn_bwd_apply_v4_fast_kernel<false, true>", "bn_bwd_apply_v4_fast_kernel<true, true>") + LEGACY_KERNELS


def kernels_in_source():
    """the __global__ functions of train_ops.hip in front of add_rows_kernel: the BatchNorm half, read from the source"""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "disconet_amd", "csrc", "train_ops.hip")
    with open(path) as f:
        text = f.read()
    text = text[:text.index("add_rows_kernel")]
    return set(re.findall(r"__global__\s+void(?:\s+__launch_bounds__\(\d+\))?\s+(\w+)\(", text))


# --- cases ---------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    """One call.  kind: "stats" | "running" | "apply" | "bwd".  shape (n, h, w, c) in `groups` groups of consecutive images
    (running: (n_groups, c), `rows` rows per group, `order` the listed groups).
    vals: "randn" z = 2 randn + 0.5 | "bigmean" channels alternate mean 1e3 / std 1 and mean 10 / std 0.1 | "const" channel 0 is
    0.37 everywhere | "gate" channels 0, 1, 2 have gamma = 0 and beta = 0, -1, +1 (y exactly 0, -1, +1: gate closed, closed,
    open; dz exactly 0).  The backward's dy is 1e-3 randn everywhere ("small").
    off: floats between a 16-byte boundary and the first element of z (stats, apply) or dy_a (bwd); ldz_pad: floats behind a row
    of z.  sync: a second rank's float64 sums are added and norm_rows = 2 rows.  running: the momentum of the fused update.
    relu: apply 0 | 1; bwd 0 | 1 (y) | 2 (the byte mask).  mask / sp: the apply also writes them; bwd sp: the SP copy of dz.
    src: dy_a "dense" | "wide" (channels 8 .. of rows of c + 8) | "up1" (2 x 2 block sums of channels 8 .. of a
    (n, 2h, 2w, c + 16) map) | "s2d" (space-to-depth).  dyb: a second gradient, rows of c + 4.  bias: None | "fold" | "deferred"
    (33 jobs).  catches: the mutants this case is meant to catch.  refuse: the entry point must return an error."""
    name: str
    kind: str
    shape: tuple
    groups: int = 1
    vals: str = "randn"
    off: int = 0
    ldz_pad: int = 0
    sync: bool = False
    running: float = None
    relu: int = 1
    mask: bool = False
    sp: bool = False
    src: str = "dense"
    dyb: bool = False
    accumulate: bool = False
    bias: str = None
    want_dz: bool = True
    rows: int = 0
    order: tuple = None
    momentum: float = 0.1
    catches: tuple = ()
    refuse: bool = False
    heavy: bool = False          # too long for the mutant sweep of the CPU file (the faithful emulation still runs)

    # ---- geometry
    @property
    def c(self):
        return self.shape[-1]

    @property
    def rpg(self):
        """rows per group"""
        if self.kind == "running":
            return self.rows
        n, h, w, _ = self.shape
        return n // self.groups * h * w

    @property
    def norm_rows(self):
        return 2 * self.rpg if self.sync else self.rpg

    @property
    def ldz(self):
        return self.c + self.ldz_pad

    @property
    def a_layout(self):
        """(floats in front of dy_a's channels inside its row, row stride) of the backward's first gradient"""
        c = self.c
        return {"dense": (self.off, c + (4 if self.off else 0)), "wide": (8, c + 8), "up1": (8, c + 16), "s2d": (0, 4 * c)}[self.src]

    @property
    def aligned(self):
        if self.kind == "bwd":
            return self.off % 4 == 0 and self.a_layout[1] % 4 == 0
        return self.off % 4 == 0 and self.ldz % 4 == 0

    @property
    def cls(self):
        """the kernel class bn_form gives this call"""
        return class_of(self.groups, self.rpg, self.c, self.aligned)

    @property
    def V(self):
        return 1 if self.cls == "general" else 4

    @property
    def U(self):
        """rows a thread of the reduction fetches before it adds them"""
        return 1 if self.cls == "general" else (4 if self.kind == "stats" else 2)

    @property
    def nblk(self):
        return blocks_per_group(self.rpg, self.groups)

    @property
    def total(self):
        return self.groups * self.rpg * self.c

    def kernels(self):
        """the kernels this case runs"""
        v4 = self.cls != "general"
        if self.kind == "running":
            return ("bn_update_running_kernel",)
        if self.kind == "stats":
            fin = ("fold_partials_kernel", "bn_stats_finalize_kernel") if self.sync else ("fold_stats_finish_kernel",)
            return ("bn_stats_v4_kernel<4>" if v4 else "bn_stats_kernel",) + fin
        if self.kind == "apply":
            return ({"general": "bn_apply_kernel", "vec4": "bn_apply_v4_kernel"}.get(self.cls) or
                    "bn_apply_v4_fast_kernel<%s>" % str(self.sp).lower(),)
        red = ("bn_bwd_reduce_v4_kernel<2>" if v4 else "bn_bwd_reduce_kernel",)
        red += ("fold_param_grad_kernel",) if self.groups == 1 else ("fold_partials_kernel", "bn_param_grad_kernel")
        sp, bias = str(self.sp).lower(), str(self.bias is not None).lower()
        app = {"general": "bn_bwd_apply_kernel", "vec4": "bn_bwd_apply_v4_kernel<%s>" % sp,
               "fast": "bn_bwd_apply_v4_fast_kernel<%s, %s>" % (sp, bias)}[self.cls]
        extra = {None: (), "fold": ("fold_channel_sum_kernel",),
                 "deferred": ("fold_channel_sum_multi_kernel", "channel_sum_kernel", "channel_sum_v4_kernel<4>")}[self.bias]
        return red + (app,) + extra

    def claim(self):
        """pass -> the fields of dn_bn_train_last_form the launch must leave"""
        k, g, c = CLS[self.cls], self.groups, self.c
        if self.kind == "running":
            n = len(self.order) if self.order else self.shape[0]
            return {"running": dict(cls=0, u=8, flags=REC_ORDER if self.order else 0, fold=FOLD_NONE, grid=(c + 63) // 64, groups=n,
                                    c=c, rows=self.rows)}
        if self.kind == "stats":
            red = dict(cls=k, u=self.U, flags=0, fold=FOLD_NONE, grid=self.nblk, groups=g, c=c, rows=self.rpg)
            if self.sync:
                fin = dict(cls=0, flags=0, fold=FOLD_FINALIZE, grid=(g * c + 255) // 256, groups=g, c=c, rows=self.norm_rows)
            else:
                fin = dict(cls=0, flags=REC_RUNNING if self.running is not None else 0, fold=FOLD_STATS_FINISH, grid=(g * c + 3) // 4,
                           groups=g, c=c, rows=self.rpg)
            return {"stats_reduce": red, "stats_finish": fin}
        if self.kind == "apply":
            flags = (REC_MASK if self.mask else 0) | (REC_SP if self.sp else 0)
            return {"apply": dict(cls=k, u=1, flags=flags, fold=FOLD_NONE, grid=grid_for(self.total // self.V, 8192), groups=g, c=c,
                                  rows=self.rpg)}
        m = REC_MASK if self.relu == 2 else 0
        red = dict(cls=k, u=self.U, flags=m, fold=FOLD_PARAM_GRAD if g == 1 else FOLD_PARTIALS_PARAM_GRAD, grid=self.nblk, groups=g, c=c,
                   rows=self.rpg)
        flags = m | (REC_SP if self.sp else 0) | (REC_BIAS if self.bias else 0) | (0 if self.want_dz else REC_DZ_NULL)
        fold = {None: FOLD_NONE, "fold": FOLD_CHANNEL_SUM, "deferred": FOLD_DEFERRED}[self.bias]
        app = dict(cls=k, u=1, flags=flags, fold=fold, grid=grid_for(self.total // self.V, 1024 if self.bias else 8192), groups=g, c=c,
                   rows=self.norm_rows)
        return {"bwd_reduce": red, "bwd_apply": app}


def _seed(name):
    return zlib.crc32(name.encode())


def _values(vals, rows, c, g):
    z = torch.randn(rows, c, generator=g) * 2.0 + 0.5
    if vals == "bigmean":
        big = torch.arange(c) % 2 == 0
        z = torch.randn(rows, c, generator=g)
        z = torch.where(big, z + 1e3, z * 0.1 + 10.0)
    if vals == "const":
        z[:, 0] = 0.37
    return z.float()


def embed(rows2d, off, ld):
    """[R, c] -> the flat fp32 buffer a strided operand lives in: R rows of ld floats, the c values `off` floats into each row,
    everything else POISON; `off` more floats behind the last row so that the channels' window of every row is inside"""
    R, c = rows2d.shape
    flat = torch.full((R * ld + off,), POISON, dtype=torch.float32)
    flat[off:off + R * ld].view(R, ld)[:, :c] = rows2d          # (the pointer is at `off`: row r's channels at off + r ld)
    return flat


def _stats64(z3):
    """[G, R, c] float64 -> mean, biased var (two-pass)"""
    m = z3.mean(1)
    return m, ((z3 - m[:, None]) ** 2).mean(1)


@lru_cache(maxsize=None)
def make(case):
    """-> the operands of the call, every tensor fp32 (or float64 where the kernel takes doubles) as the launch is given it"""
    k = case
    g = torch.Generator().manual_seed(_seed(k.name))
    m = SimpleNamespace(case=k)
    if k.kind == "running":
        n_stat, c = k.shape
        m.mean = (torch.randn(n_stat, c, generator=g) * 2.0).float()
        m.var = (torch.rand(n_stat, c, generator=g) * 3.0 + 0.01).float()
        m.rm0, m.rv0 = torch.randn(c, generator=g).float(), (torch.rand(c, generator=g) + 0.5).float()
        return m
    n, h, w, c = k.shape
    G, R = k.groups, k.rpg
    m.z = _values(k.vals, G * R, c, g).view(G, R, c)
    if k.sync:
        m.zB = _values(k.vals, G * R, c, g).view(G, R, c)
    if k.kind == "stats":
        if k.sync:      # the other rank's folded sums, float64 [G, 2, c] (exact: a float x float product and these sums fit a double)
            zb = m.zB.double()
            m.sumsB = torch.stack((zb.sum(1), (zb * zb).sum(1)), 1)
        if k.running is not None:
            m.rm0, m.rv0 = torch.randn(c, generator=g).float(), (torch.rand(c, generator=g) + 0.5).float()
        return m
    # apply and backward: the stored statistics are those of the (two-rank) batch, rounded to fp32
    zall = torch.cat((m.z, m.zB), 1).double() if k.sync else m.z.double()
    mean, var = _stats64(zall)
    m.mean, m.var = mean.float(), var.float()
    m.gamma = (torch.randn(c, generator=g) * 0.5 + 1.0).float()
    m.beta = (torch.randn(c, generator=g) * 0.5).float()
    if k.vals == "gate":
        m.gamma[:3] = 0.0
        m.beta[:3] = torch.tensor([0.0, -1.0, 1.0])
    if k.kind == "apply":
        return m
    # backward: y and the byte mask are what the forward kernel stores (its emulation), dy ~ 1e-3
    relu = k.relu != 0
    m.y = _apply32(m.z, m.mean, m.var, m.gamma, m.beta, relu)
    m.maskbytes = mask_of(_apply32(m.z, m.mean, m.var, m.gamma, m.beta, False))
    small = lambda *s: (torch.randn(*s, generator=g) * 1e-3).float()      # noqa: E731
    if k.src == "up1":
        m.dy_a = small(n, 2 * h, 2 * w, c)
    elif k.src == "s2d":
        m.dy_a = small(n, h // 2, w // 2, 4 * c)
    else:
        m.dy_a = small(n, h, w, c)
    m.dy_b = small(G, R, c) if k.dyb else None
    if k.accumulate:
        m.old_dgamma, m.old_dbeta = torch.randn(c, generator=g).float(), torch.randn(c, generator=g).float()
    if k.sync:          # the other rank's rows under the same statistics -> its float64 sums of g and g zhat [G, 2, c]
        yB = _apply32(m.zB, m.mean, m.var, m.gamma, m.beta, relu)
        gB = small(G, R, c).double() * ((yB > 0).double() if relu else 1.0)
        zhB = (m.zB.double() - m.mean.double()[:, None]) / torch.sqrt(m.var.double() + EPS)[:, None]
        m.sumsB = torch.stack((gB.sum(1), (gB * zhB).sum(1)), 1)
    return m


# --- fp32 pieces of the kernels' arithmetic ---------------------------------------------------------------
def _fma32(a, b, c):
    """fmaf(a, b, c): the product of two floats is exact in double, one rounding to double, one to float"""
    return (a.double() * b.double() + c.double()).float()


def _rstd32(var):
    return 1.0 / torch.sqrt(var + torch.tensor(EPS, dtype=torch.float32))


def _apply32(z3, mean, var, gamma, beta, relu, plain=False):
    """bn_fwd_element on [G, R, c]: zhat = (z - mean) * rstd, y = fma(zhat, gamma, beta); plain: no fused multiply-add"""
    zhat = (z3 - mean[:, None]) * _rstd32(var)[:, None]
    y = zhat * gamma + beta if plain else _fma32(zhat, gamma.expand_as(zhat), beta.expand_as(zhat))
    return y.clamp(min=0.0) if relu else y


def mask_of(y_pre, reverse=False):
    """[.., c] pre-ReLU values -> uint8 [numel / 4]: bit e of byte i is y[4 i + e] > 0"""
    bits = (y_pre.reshape(-1, 4) > 0).to(torch.uint8)
    w = torch.tensor([8, 4, 2, 1] if reverse else [1, 2, 4, 8], dtype=torch.uint8)
    return (bits * w).sum(1).to(torch.uint8)


def gate_of(maskbytes, shape, reverse=False):
    sh = torch.tensor([3, 2, 1, 0] if reverse else [0, 1, 2, 3], dtype=torch.uint8)
    return ((maskbytes[:, None] >> sh) & 1).reshape(shape).bool()


def sp_bytes(x_nhwc):
    """the bytes of the SP copy of the fp32 tensor x [n, h, w, c] (tests/sp_format.py's CPU split), uint8"""
    return torch.from_numpy(np.ascontiguousarray(sp_format.act_image(x_nhwc.numpy())).view(np.uint8).reshape(-1).copy())


def sp_values(data_u8, shape):
    """the values (hi + lo) an SP tensor's bytes hold, as [n, h, w, c] float64 (c % 16 == 0)"""
    n, h, w, c = shape
    bits = data_u8.numpy().view(np.uint16).reshape(n, c // 16, 2, 2, h * w, 8)      # [img][chunk][part][oct][px][8]
    val = sp_format.value_of(bits[:, :, 0], bits[:, :, 1])                                # [img][chunk][oct][px][8]
    return torch.from_numpy(val.transpose(0, 3, 1, 2, 4).reshape(n, h, w, c).astype(np.float64))


# --- which rows and channels a reduction adds --------------------------------------------------------------
def _row_mask(rows, c, nblk, V, U, mutant):
    """bool [rows, c]: the (row, channel) pairs group_channel_sums and the fold add; a mutant drops some"""
    keep = torch.ones(rows, c, dtype=torch.bool)
    chunk = -(-rows // nblk)
    cvn = c // 4 if V == 4 else c
    tx_n = lanes_for(cvn)
    ty_n = 256 // tx_n
    r = torch.arange(rows)
    blk = r // chunk
    if mutant == "last_chunk":                  # the last workgroup that owns rows
        keep[blk == (rows - 1) // chunk] = False
    if mutant == "fold_tail":                   # the fold's loop after its full batches of 8 x 64 partials
        keep[blk >= 512] = False
    if mutant == "u_tail" and U > 1:            # a thread's rows after its U-unrolled loop
        i = r - blk * chunk
        ty, kk = i % ty_n, i // ty_n
        in_chunk = torch.clamp((blk + 1) * chunk, max=rows) - blk * chunk
        n_k = (in_chunk - ty + ty_n - 1) // ty_n
        keep[kk >= n_k // U * U] = False
    if mutant == "lane2":                       # the second pass of `for (cv = tx; cv < cvn; cv += tx_n)`
        keep[:, V * tx_n:] = False
    return keep


def _read_rows(rows2d, off, ld, wrong_ld=None):
    """what a kernel reads through (pointer, ld) -- or through another stride than the buffer's"""
    R, c = rows2d.shape
    if wrong_ld is None:
        return rows2d
    flat = embed(rows2d, off, ld)[off:]
    need = (R - 1) * wrong_ld + c
    flat = torch.cat((flat, torch.full((max(0, need - flat.numel()),), POISON)))
    return flat.as_strided((R, c), (wrong_ld, 1)).clone()


# --- references ------------------------------------------------------------------------------------------
def running_reference(mean, var, rows, rm0, rv0, momentum, order):
    """-> {"rm": Ref, "rv": Ref}: the recurrence in float64 on the fp32 statistics, in `order` (a list of groups)"""
    mom = float(torch.tensor(momentum, dtype=torch.float32))
    unbias = rows / (rows - 1.0) if rows > 1 else 1.0
    rm, rv = rm0.double(), rv0.double()
    am, av = rm.abs(), rv.abs()
    for gi in order:
        rm = (1.0 - mom) * rm + mom * mean[gi].double()
        am = (1.0 - mom) * am + mom * mean[gi].double().abs()
        rv = (1.0 - mom) * rv + mom * (var[gi].double() * unbias)
        av = (1.0 - mom) * av + mom * (var[gi].double() * unbias)
    return {"rm": Ref(rm, am), "rv": Ref(rv, av)}


def _groups_of(case):
    return list(case.order) if case.order else list(range(case.shape[0]))


def _g64(case, m):
    """the incoming gradient in float64 [G, R, c], gated by the stored y / byte mask"""
    k = case
    n, h, w, c = k.shape
    a = m.dy_a.double()
    if k.src == "up1":
        a = a[:, 0::2, 0::2] + a[:, 0::2, 1::2] + a[:, 1::2, 0::2] + a[:, 1::2, 1::2]
    elif k.src == "s2d":
        a = a.view(n, h // 2, w // 2, 2, 2, c).permute(0, 1, 3, 2, 4, 5).reshape(n, h, w, c)
    a = a.reshape(k.groups, k.rpg, c)
    if m.dy_b is not None:
        a = a + m.dy_b.double()
    if k.relu == 1:
        a = a * (m.y > 0).double()
    elif k.relu == 2:
        a = a * gate_of(m.maskbytes, a.shape).double()
    return a


@lru_cache(maxsize=None)
def reference(case):
    """-> {output: Ref(y, A)} in float64 on the operands as stored"""
    k, m = case, make(case)
    if k.kind == "running":
        return running_reference(m.mean, m.var, k.rows, m.rm0, m.rv0, k.momentum, _groups_of(k))
    out = {}
    if k.kind == "stats":
        z = torch.cat((m.z, m.zB), 1).double() if k.sync else m.z.double()
        N = z.shape[1]
        mean, var = _stats64(z)
        out["mean"] = Ref(mean, P24 * mean.abs() + N * P53 * z.abs().mean(1))
        out["var"] = Ref(var, P24 * var + N * P53 * ((z * z).mean(1) + mean * mean))
        return out
    mean, var, gamma, beta = m.mean.double()[:, None], m.var.double()[:, None], m.gamma.double(), m.beta.double()
    rstd = 1.0 / torch.sqrt(var + EPS)
    zhat = (m.z.double() - mean) * rstd
    if k.kind == "apply":
        y = zhat * gamma + beta
        out["y_pre"] = Ref(y, (zhat * gamma).abs() + beta.abs())
        out["y"] = Ref(y.clamp(min=0.0) if k.relu else y, out["y_pre"].A)
        return out
    g = _g64(k, m)
    S1, S2 = g.sum(1), (g * zhat).sum(1)                      # this rank's [G, c]
    A1, A2 = g.abs().sum(1), (g * zhat).abs().sum(1)
    db, dg, Ab, Ag = S1.sum(0), S2.sum(0), A1.sum(0), A2.sum(0)
    if k.accumulate:
        db, dg = db + m.old_dbeta.double(), dg + m.old_dgamma.double()
        Ab, Ag = Ab + m.old_dbeta.double().abs(), Ag + m.old_dgamma.double().abs()
    out["dbeta"], out["dgamma"] = Ref(db, Ab), Ref(dg, Ag)
    if k.sync:
        S1, S2 = S1 + m.sumsB[:, 0], S2 + m.sumsB[:, 1]
    m1, m2 = (S1 / k.norm_rows)[:, None], (S2 / k.norm_rows)[:, None]
    out["dz"] = Ref(gamma * rstd * (g - m1 - zhat * m2), gamma.abs() * rstd * (g.abs() + m1.abs() + (zhat * m2).abs()))
    return out


def bias_reference(dz32):
    """the fused bias gradient against the fp32 dz [.., c] the same launch wrote"""
    d = dz32.double().reshape(-1, dz32.shape[-1])
    return Ref(d.sum(0), d.abs().sum(0))


def channel_sum_reference(x):
    d = x.double().reshape(-1, x.shape[-1])
    return Ref(d.sum(0), d.abs().sum(0))


# --- the kernels' arithmetic, and ways to get it wrong -------------------------------------------------------
MUTANTS = ("sq32", "var_unbiased", "norm_rows", "group0", "last_chunk", "u_tail", "fold_tail", "lane2", "up_tap", "s2d_parity", "ld_b",
           "ldz", "gate_ge", "mask_bits", "no_m2", "acc_ignored", "order_ignored", "pad8", "no_unbias", "bias_quad")


def _running32(mean, var, rows, rm0, rv0, momentum, order, no_unbias=False):
    """bn_running_step, every product rounded: torch's float32 ops round each"""
    mom = torch.tensor(momentum, dtype=torch.float32)
    one = torch.tensor(1.0, dtype=torch.float32)
    unbias = (torch.tensor(float(rows), dtype=torch.float32) / torch.tensor(float(rows - 1), dtype=torch.float32)) if rows > 1 and not no_unbias else one
    rm, rv = rm0.clone(), rv0.clone()
    for gi in order:
        rm = (one - mom) * rm + mom * mean[gi]
        rv = (one - mom) * rv + mom * (var[gi] * unbias)
    return rm, rv


def _g32(case, m, mutant):
    """GradSrc::load: the incoming gradient in fp32 [G, R, c]"""
    k = case
    n, h, w, c = k.shape
    a = m.dy_a
    if k.src == "up1":
        t00, t01, t10, t11 = a[:, 0::2, 0::2], a[:, 0::2, 1::2], a[:, 1::2, 0::2], a[:, 1::2, 1::2]
        a = (t00 + t01) + (t10 + (0.0 if mutant == "up_tap" else t11))
    elif k.src == "s2d":
        perm = (0, 1, 4, 2, 3, 5) if mutant == "s2d_parity" else (0, 1, 3, 2, 4, 5)
        a = a.view(n, h // 2, w // 2, 2, 2, c).permute(*perm).reshape(n, h, w, c)
    a = a.reshape(k.groups, k.rpg, c)
    if m.dy_b is not None:
        b = m.dy_b.reshape(-1, c)
        a = a + _read_rows(b, 0, c + 4, c if mutant == "ld_b" else None).view_as(a)
    if k.relu == 1:
        a = torch.where((m.y >= 0) if mutant == "gate_ge" else (m.y > 0), a, torch.zeros(()))
    elif k.relu == 2:
        a = torch.where(gate_of(m.maskbytes, a.shape, reverse=mutant == "mask_bits"), a, torch.zeros(()))
    return a


def _bias32(dz, blocks, c, mutant):
    """the bias partials of bn_bwd_apply_body: thread t of the grid adds its quads t, t + T, ... in fp32 in that order, then double
    over the threads of a channel quad"""
    c4n = c // 4
    T = blocks * 256
    q = dz.reshape(-1, 4)
    K = -(-q.shape[0] // T)
    q = torch.cat((q, torch.zeros(K * T - q.shape[0], 4)))
    acc = torch.zeros(T, 4)
    for kk in range(K):
        acc = acc + q[kk * T:(kk + 1) * T]                    # (+ 0.f for a thread past the end: exact)
    per_quad = acc.double().view(-1, c4n, 4).sum(0)           # thread t holds quad t % c4n (T % c4n == 0)
    if mutant == "bias_quad":
        per_quad = per_quad.roll(1, 0)
    return per_quad.reshape(c).float()


def emulate(case, mutant=None, plain=False):
    """A CPU emulation of the call -> {output: float64 tensor}; mutant: one of MUTANTS; plain: the float32 yardstick (torch float32
    ops without the spelled-out fused multiply-adds, double sums)"""
    assert mutant is None or mutant in MUTANTS
    k, m = case, make(case)
    if k.kind == "running":
        n_stat = k.shape[0]
        order = _groups_of(k)
        if mutant == "order_ignored":
            order = [min(i, n_stat - 1) for i in range(len(order))]
        if mutant == "pad8" and len(order) % 8:
            order = order + [order[-1]] * (8 - len(order) % 8)
        rm, rv = _running32(m.mean, m.var, k.rows, m.rm0, m.rv0, k.momentum, order, mutant == "no_unbias")
        return {"rm": rm.double(), "rv": rv.double()}
    G, R, c = k.groups, k.rpg, k.c
    z = m.z
    if mutant == "ldz":
        z = _read_rows(m.z.reshape(-1, c), k.off, k.ldz, c).view(G, R, c)
    keep = _row_mask(R, c, k.nblk, k.V, k.U, mutant).double()
    if k.kind == "stats":
        if mutant == "group0":
            z = z[:1].expand(G, R, c)
        zd = z.double()
        sq = (z * z).double() if mutant == "sq32" else zd * zd
        s0, s1 = (zd * keep).sum(1), (sq * keep).sum(1)
        if k.sync:
            s0, s1 = s0 + m.sumsB[:, 0], s1 + m.sumsB[:, 1]
        N = R if mutant == "norm_rows" else k.norm_rows
        mean = s0 / N
        var = s1 / N - mean * mean                            # fma(-m, m, s1 / rows): the product's own rounding is 2^-53 m^2
        if mutant == "var_unbiased":
            var = var * N / (N - 1.0)
        out = {"mean": mean.float().double(), "var": var.clamp(min=0.0).float().double()}
        if k.running is not None:
            rm, rv = _running32(out["mean"].float(), out["var"].float(), R, m.rm0, m.rv0, k.running, [0], mutant == "no_unbias")
            out["rm"], out["rv"] = rm.double(), rv.double()
        return out
    mean, var = (m.mean[:1].expand(G, c), m.var[:1].expand(G, c)) if mutant == "group0" else (m.mean, m.var)
    if k.kind == "apply":
        pre = _apply32(z, mean, var, m.gamma, m.beta, False, plain)
        out = {"y_pre": pre.double(), "y": (pre.clamp(min=0.0) if k.relu else pre).double()}
        if k.mask:
            out["mask"] = mask_of(pre, reverse=mutant == "mask_bits")
        return out
    # backward
    rstd = _rstd32(var)[:, None]
    zhat = (z - mean[:, None]) * rstd
    g = _g32(k, m, mutant)
    S = torch.stack((g.double() * keep, (g * zhat).double() * keep)).sum(2)      # [2, G, c]
    db, dg = S[0].sum(0).float(), S[1].sum(0).float()
    if k.accumulate and mutant != "acc_ignored":
        db, dg = m.old_dbeta + db, m.old_dgamma + dg
    if k.sync:
        S = S + m.sumsB.permute(1, 0, 2)
    N = R if mutant == "norm_rows" else k.norm_rows
    m1 = (S[0] / N).float()[:, None]
    m2 = torch.zeros_like(m1) if mutant == "no_m2" else (S[1] / N).float()[:, None]
    if plain:
        dz = m.gamma * rstd * ((g - m1) - zhat * m2)
    else:
        dz = m.gamma * rstd * _fma32(-zhat, m2.expand_as(zhat), g - m1)
    out = {"dbeta": db.double(), "dgamma": dg.double(), "dz": dz.double()}
    if k.bias:
        out["dbias"] = _bias32(dz, grid_for(k.total // 4, 1024), c, mutant).double()
    if k.sp:
        out["dz_sp"] = sp_values(sp_bytes((dz * SP_LIFT).view(k.shape)), k.shape).view(G, R, c) / SP_LIFT
    return out


# --- the bound ----------------------------------------------------------------------------------------
def family_of(case, name):
    """(output, value family); the backward's dz apart where g is itself a rounded fp32 sum (the 2 x 2 block sum, dy_a + dy_b):
    A_dz holds |g|, not the sum of the addends' magnitudes, so a cancelling sum shows in the yardstick"""
    name = {"y_pre": "y", "rm": "running", "rv": "running", "dz_sp": "dz"}.get(name, name)
    if name == "dz" and (case.src == "up1" or case.dyb):
        name = "dz+sum"
    return name if name == "running" else name + "/" + case.vals


# Measured with `python -m tests.bn_fp64`: max over the family's cases and elements of |float32 - ref| / A (emulate(plain=True)
# against reference()).  Beside each entry the faithful emulation's figure.
YARD = {
    "dbeta/const": 2.257e-08,      # emulation 2.257e-08
    "dbeta/gate": 1.608e-08,      # emulation 1.608e-08
    "dbeta/randn": 4.788e-08,      # emulation 4.788e-08
    "dbias/randn": 2.761e-08,      # emulation 2.733e-08
    "dgamma/const": 3.286e-08,      # emulation 3.286e-08
    "dgamma/gate": 4.188e-08,      # emulation 4.188e-08
    "dgamma/randn": 9.231e-08,      # emulation 9.231e-08
    "dz+sum/randn": 6.059e-06,      # emulation 6.050e-06
    "dz/const": 3.920e-07,      # emulation 3.780e-07
    "dz/gate": 3.181e-07,      # emulation 3.181e-07
    "dz/randn": 5.675e-06,      # emulation 5.675e-06
    "running": 4.619e-07,      # emulation 4.619e-07
    "y/bigmean": 1.866e-07,      # emulation 1.611e-07
    "y/gate": 2.020e-07,      # emulation 1.875e-07
    "y/randn": 2.503e-07,      # emulation 2.351e-07
}


def _ratios(case, outs):
    """{output: worst |outs - ref| / A} of every output of the case that has a float64 reference (c = 1)"""
    ref = reference(case)
    r = {name: worst(outs[name], ref[name], 1.0) for name in ref if name in outs and name != "y_pre"}
    if "dbias" in outs:
        r["dbias"] = worst(outs["dbias"], bias_reference(outs["dz"].float()), 1.0)
    return r


def _yard_cases():
    return [k for k in CASES if k.kind != "stats" and not k.refuse]


def _measure(plain):
    table = {}
    for k in _yard_cases():
        for name, r in _ratios(k, emulate(k, plain=plain)).items():
            fam = family_of(k, name)
            table[fam] = max(table.get(fam, 0.0), r)
    return table


def measure_yard():
    return _measure(True)


def measure_emulation():
    return _measure(False)


def c_of(case, name):
    """the factor c of |got - ref| <= c A for output `name` of the case"""
    if case.kind == "stats" and name in ("mean", "var"):
        return MARGIN
    c = MARGIN * YARD[family_of(case, name)]
    return c + P24 if case.accumulate and name in ("dbeta", "dgamma") else c


def judge(case, outs):
    """{output: worst |got - ref| / (c A)} over what `outs` holds: <= 1 passes.  outs as emulate() returns them (float64, the
    kernel's layout [G, R, c]); "mask" (bytes) gives the share of determined bits that differ, as inf where any does; a fused
    running update (rm, rv) is judged on the fp32 mean / var of the same outs; dbias on the fp32 dz of the same outs (want_dz
    False: on the float64 dz with the elements' own bounds added); dz_sp of such a launch on the float64 dz plus the split's own
    2^-21 max |dz|."""
    k, ref = case, dict(reference(case))
    r = {}
    if k.kind == "stats" and k.running is not None:
        m = make(k)
        ref.update(running_reference(outs["mean"].float(), outs["var"].float(), k.rpg, m.rm0, m.rv0, k.running, [0]))
    for name in ref:
        if name in outs and name != "y_pre":
            r[name] = worst(outs[name], ref[name], c_of(k, name))
    if "mask" in outs:
        pre = ref["y_pre"]
        fixed = (pre.y.abs() > c_of(k, "y") * pre.A) | (pre.A == 0)
        got = gate_of(outs["mask"], pre.y.shape)
        r["mask"] = float("inf") if bool(((got != (pre.y > 0)) & fixed).any()) else 0.0
    if "dbias" in outs:
        cb = c_of(k, "dbias")
        if k.want_dz:
            r["dbias"] = worst(outs["dbias"], bias_reference(outs["dz"].float()), cb)
        else:
            d = ref["dz"]
            A = d.y.abs().reshape(-1, k.c).sum(0) + (c_of(k, "dz") / cb) * d.A.reshape(-1, k.c).sum(0)
            r["dbias"] = worst(outs["dbias"], Ref(d.y.reshape(-1, k.c).sum(0), A), cb)
    if "dz_sp" in outs and not k.want_dz:
        d, cz = ref["dz"], c_of(k, "dz")
        r["dz_sp"] = worst(outs["dz_sp"], Ref(d.y, d.A + P21 * float(d.y.abs().max()) / cz), cz)
    return r


def mask_free_share(case):
    """share of the reference's own mask bits inside the band |y_ref| <= c A (free: either bit passes)"""
    pre = reference(case)["y_pre"]
    free = ~((pre.y.abs() > c_of(case, "y") * pre.A) | (pre.A == 0))
    return float(free.double().mean())


# --- cases ---------------------------------------------------------------------------------------
def _stats_cases():
    S1, S4, S5 = (2, 9, 7, 13), (1, 20, 32, 4), (1, 9, 36, 512)
    K = lambda name, shape, groups=1, catches=(), **kw: Case("stats:" + name, "stats", shape, groups,      # noqa: E731
                                                             catches=("var_unbiased",) + tuple(catches), **kw)
    out = [
        K("S1-scalar-odd-c", S1, catches=("last_chunk",)),
        K("S2-c1-3groups", (3, 8, 8, 1), 3, catches=("group0",)),
        K("S3-c16-misaligned", (1, 8, 8, 16), off=1, ldz_pad=4),
        K("S4-float4-10wg", S4, catches=("last_chunk", "u_tail")),
        K("S5-ty4-chunk65", S5, catches=("u_tail", "last_chunk", "lane2")),
        K("S6-cvn65", (1, 8, 16, 260), catches=("lane2",)),
        K("S7-trailing-wg-owns-no-rows", (24, 2731, 1, 4), 8, catches=("last_chunk", "group0")),
        K("S8a-576-partials", (1, 192, 192, 4), catches=("fold_tail",)),
        K("S8b-1024-partials", (1, 256, 256, 4), catches=("fold_tail",)),
        K("S9a-9groups-float4", (9, 8, 8, 12), 9, catches=("group0",)),
        K("S9b-16groups-scalar", (16, 4, 4, 5), 16, catches=("group0",)),
    ]
    for nm, shape in (("S1", S1), ("S4", S4), ("S5", S5)):
        out.append(K("S10-%s-bigmean" % nm, shape, vals="bigmean", catches=("sq32",)))
        out.append(K("S10-%s-const" % nm, shape, vals="const"))
    out.append(K("S10-S7-bigmean", (24, 2731, 1, 4), 8, vals="bigmean", catches=("sq32",)))
    out += [K("S11-S4-two-ranks", S4, sync=True, catches=("norm_rows",)),
            K("S11-S9a-two-ranks", (9, 8, 8, 12), 9, sync=True, catches=("norm_rows", "group0"))]
    for mom in (0.1, 1.0):
        for nm, shape in (("S1", S1), ("S4", S4)):
            out.append(K("S12-%s-running-%g" % (nm, mom), shape, running=mom, catches=("no_unbias",)))
        out.append(K("S12-1row-running-%g" % mom, (1, 1, 1, 8), running=mom, catches=()))
    out += [K("S13-S4-ldz", S4, ldz_pad=8, catches=("ldz",)), K("S13-S5-ldz", S5, ldz_pad=8, catches=("ldz",))]
    return out


def _running_cases():
    out = []
    for c in (5, 70):
        for n in (1, 7, 8, 9, 17):
            out.append(Case("running:%d-groups-c%d" % (n, c), "running", (n, c), rows=96,
                            catches=("no_unbias",) + (("pad8",) if n % 8 else ())))
        out.append(Case("running:order-11-of-9-c%d" % c, "running", (9, c), rows=96, order=(4, 0, 8, 8, 2, 7, 0, 5, 1, 8, 3),
                        catches=("order_ignored", "pad8", "no_unbias")))
    out.append(Case("running:1-row-per-group", "running", (3, 5), rows=1, catches=("pad8",)))
    return out


def _apply_cases():
    K = lambda name, shape, groups=1, **kw: Case("apply:" + name, "apply", shape, groups, **kw)      # noqa: E731
    out = [
        K("general-odd-c", (2, 9, 7, 13)),
        K("general-3groups", (3, 8, 8, 5), 3, catches=("group0",)),
        K("general-c16-misaligned", (1, 8, 8, 16), off=1, ldz_pad=4, catches=("ldz",)),
        K("general-c16-misaligned-mask-refused", (1, 8, 8, 16), off=1, ldz_pad=4, mask=True, refuse=True),
        K("general-odd-c-mask-refused", (2, 9, 7, 13), mask=True, refuse=True),
        K("vec4-c12-mask", (2, 5, 5, 12), mask=True, catches=("mask_bits",)),
        K("vec4-c16-2groups-mask", (2, 5, 5, 16), 2, mask=True, catches=("group0", "mask_bits")),
        K("vec4-c12-ldz", (2, 5, 5, 12), ldz_pad=8, relu=0, catches=("ldz",)),
    ]
    for c in (4, 16, 512):
        shape = (2, 6, 10, c)
        out += [K("fast-c%d-relu-mask" % c, shape, mask=True, catches=("mask_bits",)), K("fast-c%d-no-relu" % c, shape, relu=0),
                K("fast-c%d-relu" % c, shape), K("fast-c%d-gate-mask" % c, shape, vals="gate", mask=True, catches=("mask_bits",)),
                K("fast-c%d-bigmean" % c, shape, vals="bigmean"), K("fast-c%d-ldz" % c, shape, ldz_pad=8, catches=("ldz",))]
    out += [K("sp-3-images-c16", (3, 5, 7, 16), mask=True, sp=True, catches=("mask_bits",)),
            K("sp-2-images-c32", (2, 6, 6, 32), mask=True, sp=True, catches=("mask_bits",)),
            K("fast-grid-wrap", (9, 64, 64, 256), mask=True, heavy=True)]
    return out


def _bwd_cases():
    K = lambda name, shape, groups=1, **kw: Case("bwd:" + name, "bwd", shape, groups, **kw)      # noqa: E731
    out = []
    for cls, c in (("fast", 16), ("vec4", 12), ("general", 13)):
        shape = (2, 6, 10, c)
        base = ("no_m2", "last_chunk") + (("u_tail",) if c != 13 else ())
        out += [
            K("%s-dense" % cls, shape, catches=base + ("gate_ge",)),
            K("%s-wide-dy_a" % cls, shape, src="wide", catches=base),
            K("%s-up1" % cls, shape, src="up1", relu=0, catches=base + ("up_tap",)),
            K("%s-s2d" % cls, shape, src="s2d", catches=base + ("s2d_parity", "gate_ge")),
            K("%s-dy_b" % cls, shape, dyb=True, catches=base + ("ld_b",)),
            K("%s-no-relu" % cls, shape, relu=0, catches=base),
            K("%s-accumulate" % cls, shape, accumulate=True, catches=base + ("acc_ignored",)),
            K("%s-two-ranks" % cls, shape, sync=True, catches=("norm_rows",)),
            K("%s-gate" % cls, shape, vals="gate", catches=base + ("gate_ge",)),
            K("%s-const" % cls, shape, vals="const", catches=base),
        ]
        if c % 4 == 0:
            out += [K("%s-mask" % cls, shape, relu=2, catches=base + ("mask_bits",)),
                    K("%s-mask-up1-dy_b" % cls, shape, relu=2, src="up1", dyb=True, catches=base + ("mask_bits", "up_tap", "ld_b"))]
    out += [
        # c = 16 with dy_a one float off 16 bytes: a float4-shaped call on the scalar kernels, the byte mask read by them too
        K("c16-misaligned-dy_a", (2, 6, 10, 16), off=1, catches=("no_m2", "last_chunk")),
        K("c16-misaligned-dy_a-mask", (2, 6, 10, 16), off=1, relu=2, catches=("no_m2", "mask_bits")),
        K("9-groups-float4", (9, 4, 4, 12), 9, catches=("group0", "no_m2")),
        K("16-groups-scalar", (16, 4, 4, 5), 16, catches=("group0", "no_m2")),
        K("9-groups-two-ranks-accumulate", (9, 4, 4, 12), 9, sync=True, accumulate=True, catches=("norm_rows", "acc_ignored", "group0")),
        K("sp-fast-c16", (2, 6, 10, 16), sp=True, catches=("no_m2",)),
        K("sp-fast-c64", (2, 6, 10, 64), sp=True, relu=2, catches=("no_m2", "mask_bits")),
        K("sp-vec4-c48", (2, 6, 10, 48), sp=True, catches=("no_m2",)),
        # the sum of dz over a whole batch is zero in exact arithmetic (sum zhat = 0, sum (g - m1) = 0): only a rank's SHARE of a
        # two-rank batch gives the fused bias gradient values a wrong quad, a dropped thread or a wrong fold would change
        K("bias-c4", (2, 6, 10, 4), bias="fold", catches=("no_m2",)),
        K("bias-sp-c16", (2, 6, 10, 16), bias="fold", sp=True, sync=True, catches=("bias_quad", "norm_rows")),
        K("bias-c512", (2, 6, 10, 512), bias="fold", sync=True, catches=("bias_quad",)),
        K("bias-sp-c16-dz-null", (2, 6, 10, 16), bias="fold", sp=True, want_dz=False, sync=True, catches=("bias_quad", "no_m2")),
        K("bias-c16-deferred-33-jobs", (2, 6, 10, 16), bias="deferred", sync=True, catches=("bias_quad",)),
        K("bias-grid-wrap", (1, 64, 72, 256), bias="fold", relu=2, sync=True, catches=("bias_quad", "last_chunk")),
    ]
    return out


CASES = _stats_cases() + _running_cases() + _apply_cases() + _bwd_cases()
assert len({k.name for k in CASES}) == len(CASES)


def fold_jobs_inputs():
    """the 32 tiny tensors whose channel_sum(..., folds=) jobs stand in front of the deferred bias fold (33 jobs: two launches
    of dn_channel_sum_fold_multi): odd and even, c = 5 on the scalar kernel, c = 8 on the float4 one"""
    g = torch.Generator().manual_seed(33)
    return [torch.randn(3 + j % 3, 5 if j % 2 else 8, generator=g).float() for j in range(32)]


if __name__ == "__main__":
    yard, emu = measure_yard(), measure_emulation()
    for fam in sorted(yard):
        print('    "%s": %.3e,      # emulation %.3e' % (fam, yard[fam], emu[fam]))
