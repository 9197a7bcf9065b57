"""Case generators, launch caps and the float64 reference call for the corner localisation loss (dn_det_loss_corner,
train_ops.det_loss_corner; reference: train_ops.host_corner_loss).  Plain torch on the CPU.  TEST infrastructure:
tests/test_corner_loss_host_cpu.py checks the reference and the generators without a GPU, tests/test_gpu_corner_loss.py
compares the HIP kernels with them.

Why the generator keeps every non-zero corner distance of a masked anchor above MIN_DIST: the gradient of a distance is
the unit vector d / |d|, and d is the difference of two corners computed in fp32 at coordinates of up to 32 m (half an
ulp: 1.9e-6), so its relative accuracy goes like 1 / |d|.  tests/test_corner_loss_host_cpu.py ::
test_fp32_host_statement_stays_within_half_the_tolerance measures the fp32 torch statement against float64 on every case
here and holds it to HALF the GPU test's gradient tolerance; the bound is raised, never the tolerance, if that fails."""
import functools

import torch

MIN_DIST = 5e-3                   # metres; see above
LOSS_RTOL = 1e-5                  # each loss value, relative (tests/test_gpu_det_loss_fp64.py)
GRAD_TOL = 2e-5                   # dloc, of the largest |gradient| of the call (the same file)

# grid caps (train_ops.hip :: dn_det_loss_corner): items per pass of the grid-stride loops = workgroups * 256 threads
CORNER_V4_CAP = 4096 * 256        # grid_for(n * 6 / 4, 4096): float4s of dloc -> 699 051 anchors
CORNER_SCALAR_CAP = 2048 * 256    # grid_for(n, 2048): anchors

ALPHA, GAMMA = 0.25, 2.0


def takes_float4_path(n, *ptrs):
    """the dispatch rule of dn_det_loss_corner (dn_det_loss' for code 6): even n and 16-byte aligned tensors"""
    return n % 2 == 0 and all(p % 16 == 0 for p in ptrs)


def anchor_table():
    """the [256 * 256 * 6, 6] rows of postprocess.make_anchors for the default 256 x 256 map: centres up to +-32 m, both
    anchor sizes, the three yaws"""
    from disconet_amd import Config, postprocess
    return postprocess.make_anchors(Config(), device="cpu").reshape(-1, 6)


def corner_distances64(loc, targets, rows):
    """[m, 4] float64 corner distances of anchors whose codes are loc / targets [m, 6] against the anchor rows [m, 6] --
    written apart from host_corner_loss (complex arithmetic: corner = centre + (dx + i dy) (cos + i sin))"""
    a = rows.double()

    def corners(t):
        t = t.double()
        centre = torch.complex(a[:, 0] + t[:, 0] * a[:, 2], a[:, 1] + t[:, 1] * a[:, 3])
        w, h = a[:, 2] * torch.exp(t[:, 2]), a[:, 3] * torch.exp(t[:, 3])
        rot = torch.complex(a[:, 5] * t[:, 5] - a[:, 4] * t[:, 4], a[:, 4] * t[:, 5] + a[:, 5] * t[:, 4])
        off = torch.stack([torch.complex(-w, -h), torch.complex(w, -h), torch.complex(w, h), torch.complex(-w, h)], 1) / 2
        return centre[:, None] + off * rot[:, None]

    return (corners(loc) - corners(targets)).abs()


def make_case(n, per_image, seed, p_pos=0.3, noise=0.2, exact_rows=0, mask="random"):
    """-> dict of float32 tensors: cls [n, 2], labels [n, 2], loc [n, 6], targets [n, 6], mask [n], anchors [per_image, 6],
    and norm.  Anchor rows are drawn from anchor_table() (mixed sizes and yaws); targets are offsets of up to ~1 anchor
    size, log sizes of +-0.2 and a UNIT (sin, cos) pair; predictions are the targets plus `noise` * randn.  mask: "random"
    (p_pos, anchor 0 always masked), "ones" or "zeros".  exact_rows: that many masked anchors get loc == targets bitwise.
    Rows whose prediction puts a corner closer than MIN_DIST to its target corner are redrawn; the bound is asserted."""
    assert n % per_image == 0
    g = torch.Generator().manual_seed(seed)
    table = anchor_table()
    anchors = table[torch.randint(0, table.shape[0], (per_image,), generator=g)].clone()
    cls = torch.randn(n, 2, generator=g) * 3
    fg = torch.rand(n, generator=g) < 0.05
    labels = torch.stack([(~fg).float(), fg.float()], -1)
    labels[torch.rand(n, generator=g) < 0.02] = 0                          # "don't care" rows
    yaw = (torch.rand(n, generator=g) * 2 - 1) * 3.141592653589793
    targets = torch.stack([torch.randn(n, generator=g) * 0.3, torch.randn(n, generator=g) * 0.3,
                           torch.randn(n, generator=g) * 0.2, torch.randn(n, generator=g) * 0.2,
                           torch.sin(yaw.double()).float(), torch.cos(yaw.double()).float()], 1)
    loc = targets + noise * torch.randn(n, 6, generator=g)
    if mask == "ones":
        m = torch.ones(n)
    elif mask == "zeros":
        m = torch.zeros(n)
    else:
        m = (torch.rand(n, generator=g) < p_pos).float()
        m[0] = 1.0
    rows = anchors[torch.arange(n) % per_image]
    for _ in range(20):                                                    # redraw the predictions that come too close
        close = (corner_distances64(loc, targets, rows).min(1).values < MIN_DIST) & (m != 0)
        if not bool(close.any()):
            break
        k = int(close.sum())
        loc[close] = targets[close] + noise * torch.randn(k, 6, generator=g)
    exact = (m != 0).nonzero().flatten()[:exact_rows]
    loc[exact] = targets[exact]
    d = corner_distances64(loc, targets, rows)[m != 0]
    assert bool(((d == 0) | (d >= MIN_DIST)).all()), float(d[d > 0].min())
    assert exact_rows == 0 or bool((d[:exact_rows] == 0).all())
    return {"cls": cls, "labels": labels, "loc": loc, "targets": targets, "mask": m, "anchors": anchors,
            "norm": float(n // per_image), "exact": exact}


# name -> make_case arguments.  n = 1, 7, 255, 257, 4099: tails and odd n (the per-anchor kernel); 256 / 258 / 4098: even n
# (the float4 kernel); two and three images for the i % per_image anchor row; the two extreme masks; exact rows.
SMALL_CASES = {
    "n1": dict(n=1, per_image=1, seed=1),
    "n7": dict(n=7, per_image=7, seed=2),
    "n255_3img": dict(n=255, per_image=85, seed=3),
    "n257": dict(n=257, per_image=257, seed=4, exact_rows=3),
    "n258_2img": dict(n=258, per_image=129, seed=5, exact_rows=4),
    "n4099": dict(n=4099, per_image=4099, seed=6, p_pos=0.05),
    "n4098_3img": dict(n=4098, per_image=1366, seed=7, p_pos=0.05, exact_rows=2),
    "n256_ones": dict(n=256, per_image=128, seed=8, mask="ones"),
    "n256_zeros": dict(n=256, per_image=128, seed=9, mask="zeros"),
    "n255_zeros": dict(n=255, per_image=255, seed=10, mask="zeros"),
}
# above both grid caps (even: the float4 kernel's 1 048 576 float4s = 699 051 anchors; the same tensors from one-float-offset
# views run the per-anchor kernel past its 524 288 anchors): both grid-stride loops iterate.  Three images, 1 % positives.
LONG_N = 700002
LONG_CASE = dict(n=LONG_N, per_image=LONG_N // 3, seed=11, p_pos=0.01, exact_rows=5)
assert LONG_N * 6 // 4 > CORNER_V4_CAP and LONG_N > CORNER_SCALAR_CAP and LONG_N % 6 == 0


@functools.lru_cache(maxsize=None)
def case(name):
    """the named case (built once per process; treat the tensors as read-only)"""
    return make_case(**(LONG_CASE if name == "long" else SMALL_CASES[name]))


def corner_ref(c, dtype=torch.float64):
    """train_ops.host_corner_loss in `dtype` under autograd on the case's fp32 values -> (loss, dloc [n, 6]) as float64"""
    from disconet_amd.train_ops import host_corner_loss
    loc = c["loc"].to(dtype).clone().requires_grad_(True)
    loss = host_corner_loss(loc, c["targets"].to(dtype), c["mask"].to(dtype), c["anchors"].to(dtype), c["norm"])
    loss.backward()
    return float(loss.detach()), loc.grad.double()


@functools.lru_cache(maxsize=None)
def ref64(name):
    return corner_ref(case(name))


def offset_copy(t, floats=1):
    """the same values in a view whose data pointer is `floats` floats past a 16-byte boundary"""
    pad = torch.zeros(t.numel() + floats, dtype=t.dtype, device=t.device)
    pad[floats:] = t.reshape(-1)
    v = pad[floats:].view(t.shape)
    assert v.data_ptr() % 16 == 4 * floats
    return v


def bits(t):
    return t.contiguous().view(torch.int32)
