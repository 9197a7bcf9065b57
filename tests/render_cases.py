"""The rendering cases that tests/test_render_host_cpu.py and tests/test_gpu_render.py share: seeded, small, numpy.

A case is {"name", "config", "kwargs"}: kwargs go to render.host_render_bev as they are and, through to_device(), to
render.render_bev.  N = 3 images; maps of 32 x 32 and a non-square 24 x 40 (its canvas is no multiple of the 32-pixel
tile at scale 1 and 2, so tiles straddle the canvas edge); scale 1, 2 and 4; K = 8 rows a set, and one case of K = 300
rows that all cover one tile (more than the 256 entries one pass of the kernel's list holds).

What the rows carry (make_layers): a box across tile borders, one partly off the canvas, one wholly off, one larger than
the canvas, w = 0, a negative h, (sin, cos) = (0, 0), an un-normalised (sin, cos), a NaN and an infinity in each member,
count = 0 and count = K, a NaN score and a score above 1, id 33 and id -1, thickness 1 (set 2, and every set at scale 1)
and a translucent fill (set 0) under the outlines of the later sets.  The heat map holds a NaN, both infinities and values
below lo and above hi; the class map a label of -100 and a label of C.
"""
import functools
import types

import numpy as np

N = 3
K = 8
K_MANY = 300
VOXEL = 0.25
MAGENTA = (200, 0, 200)


def make_config(h, w):
    """what render_bev reads of a Config, for an h x w map (Config itself is square)"""
    return types.SimpleNamespace(voxel_size=(VOXEL, VOXEL, 0.4), map_dims=[h, w, 13],
                                 area_extents=np.array([[-h * VOXEL / 2, h * VOXEL / 2], [-w * VOXEL / 2, w * VOXEL / 2],
                                                        [-3.0, 2.0]]))


def _unit(yaw):
    return np.sin(yaw), np.cos(yaw)


def _random_boxes(rng, n, k, hx, hy):
    b = np.zeros((n, k, 6), dtype=np.float32)
    b[..., 0] = rng.uniform(-hx, hx, (n, k))
    b[..., 1] = rng.uniform(-hy, hy, (n, k))
    b[..., 2] = rng.uniform(0.8, 2.5, (n, k))
    b[..., 3] = rng.uniform(0.5, 1.5, (n, k))
    yaw = rng.uniform(-np.pi, np.pi, (n, k))
    b[..., 4], b[..., 5] = np.sin(yaw), np.cos(yaw)
    return b


def make_layers(h, w, seed):
    """the four sets of the main case as BoxLayer keyword dicts"""
    rng = np.random.RandomState(seed)
    hx, hy = h * VOXEL / 2, w * VOXEL / 2
    # set 0: "ground truth", fixed colour, translucent fill
    gt = _random_boxes(rng, N, K, hx, hy)
    gt[:, 0] = [0.05, -0.1, 3.0, 2.0, *_unit(np.pi / 6)]              # across the tile borders at the canvas centre
    gt[:, 1] = [hx - 0.2, hy - 0.4, 2.0, 1.5, *_unit(-0.4)]           # partly off the canvas
    gt[:, 2] = [5 * hx, -5 * hy, 2.0, 1.0, 0.0, 1.0]                  # wholly off
    gt[:, 3, 2] = 0.0                                                # w = 0
    gt[:, 4, 3] = -1.0                                               # a negative h
    gt[:, 5, 4:] = 0.0                                               # (sin, cos) = (0, 0)
    gt[:, 6] = [-0.5 * hx, 0.4 * hy, 2.0, 1.0, 1.5, 2.0]              # un-normalised (sin, cos)
    set0 = {"boxes": gt, "count": np.asarray([K, 0, 5], np.int32), "colour": (0, 170, 0), "fill_alpha": 96}
    # set 1: "detections", coloured by score, their outlines over set 0's fill
    det = _random_boxes(rng, N, K, hx, hy)
    det[:, 0] = [0.2, 0.1, 2.8, 1.8, *_unit(np.pi / 6 + 0.1)]
    scores = rng.uniform(0, 1, (N, K)).astype(np.float32)
    scores[:, 1], scores[:, 2], scores[:, 3] = np.nan, 1.7, -0.2
    set1 = {"boxes": det, "scores": scores, "by": "score", "colour": (40, 90, 255), "colour_hi": (255, 40, 0)}
    # set 2: "tracks", coloured by id, no heading tick, thickness 1 at every scale
    trk = _random_boxes(rng, N, K, hx, hy)
    ids = rng.randint(0, 200, (N, K)).astype(np.int32)
    ids[:, 0], ids[:, 1], ids[:, 2] = 33, -1, 1
    set2 = {"boxes": trk, "ids": ids, "count": np.asarray([K, K, 0], np.int32), "by": "id", "heading": False, "thickness": 1}
    # set 3: rows that must not be painted, a NaN (image 0) and an infinity (image 1) in each member, and a box larger
    # than the canvas whose long edges cross it
    bad = _random_boxes(rng, N, K, hx, hy)
    for m in range(6):
        bad[0, m, m] = np.nan
        bad[1, m, m] = np.inf if m % 2 else -np.inf
    bad[:, 6] = [0.0, 0.0, 2 * hx - 0.45, 30.0 * hy, 0.0, 1.0]
    set3 = {"boxes": bad, "colour": MAGENTA, "thickness": 2}
    return [set0, set1, set2, set3]


def make_words(rng, h, w, p=0.12):
    """occupancy words [N, h, w] int32: a share p of the pixels holds 1..13 points"""
    depth = rng.randint(1, 14, (N, h, w))
    bits = np.zeros((N, h, w), dtype=np.uint32)
    for i, j, k in zip(*np.nonzero(rng.uniform(0, 1, (N, h, w)) < p)):
        bits[i, j, k] = np.uint32(sum(1 << int(z) for z in rng.choice(32, depth[i, j, k], replace=False)))
    return bits.view(np.int32)


def make_heat(rng, hh, hw):
    heat = rng.uniform(-0.2, 1.2, (N, hh, hw)).astype(np.float32)     # heat_range is (0.1, 0.9): below lo, above hi
    heat[:, 0, 0], heat[:, 1, 2], heat[:, 2, 1] = np.nan, np.inf, -np.inf
    return heat


def main_case(h, w, scale, heat_hw, seed=7):
    rng = np.random.RandomState(seed + 1000)
    return {"name": "main_%dx%d_s%d" % (h, w, scale), "config": make_config(h, w),
            "kwargs": {"background": make_words(rng, h, w), "heat": make_heat(rng, *heat_hw), "heat_range": (0.1, 0.9),
                       "heat_alpha": 160, "layers": make_layers(h, w, seed), "scale": scale}}


def classes_case(scale=2, seed=11):
    rng = np.random.RandomState(seed)
    h = w = 32
    labels = rng.randint(0, 4, (N, h, w)).astype(np.int32)
    labels[:, 3, 5], labels[:, 9, 2] = -100, 4                        # outside [0, C): ground
    palette = np.asarray([[250, 250, 250], [120, 120, 120], [70, 130, 180], [250, 170, 30]], dtype=np.uint8)
    return {"name": "classes_s%d" % scale, "config": make_config(h, w),
            "kwargs": {"classes": labels, "palette": palette, "layers": make_layers(h, w, seed)[:2], "scale": scale}}


def plain_case(scale=1, seed=13):
    """no background, no heat: the number of images comes from the layers"""
    h = w = 32
    return {"name": "plain_s%d" % scale, "config": make_config(h, w),
            "kwargs": {"layers": make_layers(h, w, seed)[1:3], "scale": scale, "ground": (10, 20, 30)}}


def many_case(scale=2, seed=17):
    """K = 300 rows that all cover the first tile, translucent, so that the order of the whole list shows"""
    rng = np.random.RandomState(seed)
    h = w = 32
    boxes = np.zeros((N, K_MANY, 6), dtype=np.float32)
    boxes[..., 0] = rng.uniform(-2.2, -1.8, (N, K_MANY))              # the first tile is [-4, 0) m at scale 2
    boxes[..., 1] = rng.uniform(-2.2, -1.8, (N, K_MANY))
    boxes[..., 2] = rng.uniform(4.5, 6.0, (N, K_MANY))               # larger than the tile wherever it is turned
    boxes[..., 3] = rng.uniform(4.5, 6.0, (N, K_MANY))
    yaw = rng.uniform(-np.pi, np.pi, (N, K_MANY))
    boxes[..., 4], boxes[..., 5] = np.sin(yaw), np.cos(yaw)
    boxes[:, 100:110, 2] = rng.uniform(0.5, 3.0, (N, 10))            # some that leave marks inside it
    scores = rng.uniform(0, 1, (N, K_MANY)).astype(np.float32)
    layer = {"boxes": boxes, "scores": scores, "count": np.asarray([K_MANY, 290, 257], np.int32), "by": "score",
             "colour": (0, 0, 255), "colour_hi": (255, 255, 0), "fill_alpha": 40}
    return {"name": "many_s%d" % scale, "config": make_config(h, w),
            "kwargs": {"background": make_words(rng, h, w), "layers": [layer], "scale": scale}}


@functools.lru_cache(maxsize=None)
def all_cases():
    cases = [main_case(32, 32, s, (8, 8)) for s in (1, 2, 4)]
    cases += [main_case(24, 40, s, (12, 8)) for s in (1, 2, 4)]      # heat factors 2 and 5
    cases += [classes_case(), plain_case(), many_case()]
    return tuple(cases)


MAIN = "main_32x32_s2"


def case(name):
    return next(c for c in all_cases() if c["name"] == name)


def names():
    return [c["name"] for c in all_cases()]


def host_kwargs(c, **over):
    """the case as host_render_bev takes it: the layer dicts as BoxLayer objects"""
    from disconet_amd.render import BoxLayer
    kw = dict(c["kwargs"], **over)
    kw["layers"] = [BoxLayer(**l) if isinstance(l, dict) else l for l in kw.get("layers", ())]
    return kw


@functools.lru_cache(maxsize=None)
def host_image(name):
    """the host statement's canvas of a case, computed once and shared (read-only)"""
    from disconet_amd.render import host_render_bev
    c = case(name)
    img = host_render_bev(c["config"], **host_kwargs(c))
    img.setflags(write=False)
    return img


def to_device(c, **over):
    """the case as render_bev takes it: every array a device tensor"""
    import torch
    from disconet_amd.render import BoxLayer
    kw = dict(c["kwargs"], **over)
    for key in ("background", "classes", "palette", "heat"):
        if kw.get(key) is not None:
            kw[key] = torch.as_tensor(kw[key]).cuda()
    kw["layers"] = [BoxLayer(**{k: torch.as_tensor(v).cuda() if isinstance(v, np.ndarray) else v for k, v in l.items()})
                    for l in kw.get("layers", ())]
    return kw
