"""render.host_render_bev, the numpy statement of dn_render_bev (include/disconet_hip.h), without a GPU: against a plain
per-pixel restatement in Python floats, against answers listed by hand, and the pieces around it -- the PNG writer, the
tool's command line, the binding."""
import importlib.util
import math
import os
import re

import numpy as np
import pytest

from tests import render_cases as rc
from tests.conftest import ROOT


# ---------------------------------------------------------------------------
# the contract once more, pixel by pixel, in Python floats and ints (no numpy arithmetic, no window, no cull)
# ---------------------------------------------------------------------------
def _blend(below, over, a):
    return tuple((p * (255 - a) + c * a + 127) // 255 for p, c in zip(below, over))


def _rows_of(layer, i, x_lo, y_lo, voxel, S):
    """the painted rows of image i: (X, Y, c, s, A, B, colour), in row order"""
    from disconet_amd.render import ID_PALETTE
    rows = []
    count = layer.k if layer.count is None else max(0, min(layer.k, int(layer.count[i])))
    for j in range(count):
        x, y, w, h, s, c = (float(v) for v in layer.boxes[i, j])
        if not all(math.isfinite(v) for v in (x, y, w, h, s, c)):
            continue
        nrm = math.sqrt(s * s + c * c)
        if not nrm > 0 or not w > 0 or not h > 0:
            continue
        if layer.by == "score":
            z = float(layer.scores[i, j])
            z = (z if z < 1.0 else 1.0) if z > 0.0 else 0.0
            l = int(math.floor(z * 255.0))
            colour = tuple((a * (255 - l) + b * l + 127) // 255 for a, b in zip(layer.colour, layer.colour_hi))
        elif layer.by == "id":
            if int(layer.ids[i, j]) < 0:
                continue
            colour = tuple(int(v) for v in ID_PALETTE[int(layer.ids[i, j]) % 32])
        else:
            colour = layer.colour
        rows.append((((x - x_lo) / voxel) * S, ((y - y_lo) / voxel) * S, c / nrm, s / nrm, ((w / 2.0) / voxel) * S,
                     ((h / 2.0) / voxel) * S, colour))
    return rows


def restate(config, images, background=None, classes=None, palette=None, heat=None, heat_range=(0, 1), heat_alpha=160,
            layers=(), scale=2, ground=(255, 255, 255), point=(32, 32, 32), heat_colour=(220, 30, 30)):
    S = scale
    src = background if background is not None else classes if classes is not None else None
    h, w = (src.shape[1], src.shape[2]) if src is not None else (config.map_dims[0], config.map_dims[1])
    x_lo, y_lo, voxel = float(config.area_extents[0][0]), float(config.area_extents[1][0]), float(config.voxel_size[0])
    lo, hi = float(heat_range[0]), float(heat_range[1])
    out = {}
    for i in images:
        sets = [(l, _rows_of(l, i, x_lo, y_lo, voxel, float(S))) for l in layers]
        img = np.zeros((S * h, S * w, 3), dtype=np.uint8)
        for r in range(S * h):
            for q in range(S * w):
                px = tuple(ground)
                if background is not None:
                    m = min(bin(int(background[i, r // S, q // S]) & 0xffffffff).count("1"), 8)
                    px = tuple((g * (8 - m) + p * m + 4) // 8 for g, p in zip(ground, point))
                elif classes is not None:
                    label = int(classes[i, r // S, q // S])
                    if 0 <= label < len(palette):
                        px = tuple(int(v) for v in palette[label])
                if heat is not None:
                    v = float(heat[i, (r // S) // (h // heat.shape[1]), (q // S) // (w // heat.shape[2])])
                    t = (v - lo) / (hi - lo)
                    if not math.isnan(t):
                        l = int(math.floor(min(max(t, 0.0), 1.0) * 255.0))
                        px = _blend(px, heat_colour, (heat_alpha * l + 127) // 255)
                for layer, rows in sets:
                    t = float(S if layer.thickness is None else layer.thickness)
                    for X, Y, c, s, A, B, colour in rows:
                        dx, dy = (r + 0.5) - X, (q + 0.5) - Y
                        u, v = dx * c + dy * s, dy * c - dx * s
                        e = max(abs(u) - A, abs(v) - B)
                        if -t < e <= 0 or (layer.heading and 0 <= u <= A and abs(v) <= t / 2.0):
                            px = colour
                        elif e <= 0 and layer.fill_alpha > 0:
                            px = _blend(px, colour, layer.fill_alpha)
                img[r, q] = px
        out[i] = img
    return out


@pytest.mark.parametrize("name,images", [("main_32x32_s1", (0, 1, 2)), ("main_32x32_s2", (0, 1, 2)), ("main_32x32_s4", (0, 1)),
                                         ("classes_s2", (0, 2)), ("plain_s1", (0, 1, 2)), ("many_s2", (2,))])
def test_host_render_is_the_per_pixel_rule(name, images):
    c = rc.case(name)
    got = rc.host_image(name)
    want = restate(c["config"], images, **rc.host_kwargs(c))
    for i in images:
        assert got[i].shape == want[i].shape
        bad = np.argwhere((got[i] != want[i]).any(-1))
        assert len(bad) == 0, "image %d: %d pixels differ, first %s" % (i, len(bad), bad[:4].tolist())


def _share(a, b):
    return float((a != b).any(-1).mean())


def test_main_case_is_not_an_empty_picture():
    """every part of the rule owns at least 1 % of the main case's canvas, so that equal bytes mean something"""
    from disconet_amd.render import host_render_bev
    c = rc.case(rc.MAIN)
    kw = rc.host_kwargs(c)
    full = rc.host_image(rc.MAIN)
    no_layers = host_render_bev(c["config"], **dict(kw, layers=()))
    no_heat = host_render_bev(c["config"], **dict(kw, layers=(), heat=None))
    blank = host_render_bev(c["config"], **dict(kw, layers=(), heat=None, background=np.zeros_like(kw["background"])))
    for l in kw["layers"]:
        l.fill_alpha = 0
    no_fill = host_render_bev(c["config"], **kw)
    shares = {"outline": _share(no_fill, no_layers), "fill": _share(full, no_fill), "overlay": _share(no_layers, no_heat),
              "points": _share(no_heat, blank)}
    print(shares)
    assert all(v >= 0.01 for v in shares.values()), shares
    assert full.shape == (rc.N, 64, 64, 3) and full.dtype == np.uint8


# ---------------------------------------------------------------------------
# known answers
# ---------------------------------------------------------------------------
def _one_box(sin, cos, **style):
    from disconet_amd.render import BoxLayer, host_render_bev
    boxes = np.asarray([[[0.0, 0.0, 2.0, 1.0, sin, cos]]], dtype=np.float32)        # 8 x 4 canvas pixels about (16, 16)
    layer = BoxLayer(boxes, colour=(1, 2, 3), **style)
    return host_render_bev(rc.make_config(32, 32), layers=[layer], scale=1)[0]


def test_axis_aligned_box_and_its_quarter_turn():
    # local +x (the 2 m side) runs along canvas rows: rows 12..19, columns 14..17; thickness 1 keeps the ring of pixels
    # whose centre is within 1 of the edge, i.e. the outermost pixel all round
    ring = {(r, q) for r in range(12, 20) for q in range(14, 18) if r in (12, 19) or q in (14, 17)}
    assert len(ring) == 20
    img = _one_box(0.0, 1.0, heading=False)
    painted = {tuple(p) for p in np.argwhere((img == (1, 2, 3)).all(-1)).tolist()}
    assert painted == ring
    assert ((img == (1, 2, 3)).all(-1) | (img == 255).all(-1)).all()
    turned = _one_box(1.0, 0.0, heading=False)
    assert {tuple(p) for p in np.argwhere((turned == (1, 2, 3)).all(-1)).tolist()} == {(q, r) for r, q in ring}
    # the heading tick: from the centre along local +x, |v| <= 1/2: the two columns next to the axis, rows 16..19
    tick = {tuple(p) for p in np.argwhere((_one_box(0.0, 1.0) == (1, 2, 3)).all(-1)).tolist()} - ring
    assert tick == {(r, q) for r in range(16, 19) for q in (15, 16)}
    # a fill: the inner pixels blended at alpha 128 over white
    fill = _one_box(0.0, 1.0, heading=False, fill_alpha=128)
    inner = (255 * 127 + 1 * 128 + 127) // 255, (255 * 127 + 2 * 128 + 127) // 255, (255 * 127 + 3 * 128 + 127) // 255
    assert {tuple(p) for p in np.argwhere((fill == inner).all(-1)).tolist()} == {
        (r, q) for r in range(13, 19) for q in (15, 16)}


def test_a_later_set_wins():
    from disconet_amd.render import BoxLayer, host_render_bev
    cfg = rc.make_config(32, 32)
    a = BoxLayer(np.asarray([[[0.0, 0.0, 2.0, 1.0, 0.0, 1.0]]], np.float32), colour=(200, 0, 0), heading=False)
    b = BoxLayer(np.asarray([[[0.0, 0.0, 2.0, 1.0, 0.0, 1.0]]], np.float32), colour=(0, 0, 200), heading=False)
    ab, ba = host_render_bev(cfg, layers=[a, b], scale=2), host_render_bev(cfg, layers=[b, a], scale=2)
    assert (ab == (0, 0, 200)).all(-1).sum() > 0 and (ab == (200, 0, 0)).all(-1).sum() == 0
    assert (ba == (200, 0, 0)).all(-1).sum() == (ab == (0, 0, 200)).all(-1).sum() and (ba == (0, 0, 200)).all(-1).sum() == 0
    # within a set the later row wins
    both = BoxLayer(np.asarray([[[0.0, 0.0, 2.0, 1.0, 0.0, 1.0], [0.0, 0.0, 2.0, 1.0, 0.0, 1.0]]], np.float32),
                    scores=np.asarray([[0.0, 1.0]], np.float32), by="score", colour=(200, 0, 0), colour_hi=(0, 0, 200),
                    heading=False)
    assert (host_render_bev(cfg, layers=[both], scale=2) == ab).all()


def test_refused_arguments():
    from disconet_amd.render import BoxLayer, host_render_bev
    boxes = np.zeros((1, 2, 6), np.float32)
    cfg = rc.make_config(32, 32)
    with pytest.raises(ValueError):
        BoxLayer(boxes, by="score")
    with pytest.raises(ValueError):
        BoxLayer(boxes, thickness=0)
    with pytest.raises(ValueError):
        BoxLayer(boxes, scores=np.zeros((1, 3), np.float32))
    with pytest.raises(ValueError):
        host_render_bev(cfg, layers=[BoxLayer(boxes)], scale=3)
    with pytest.raises(ValueError):
        host_render_bev(cfg, layers=[BoxLayer(boxes)] * 5)
    with pytest.raises(ValueError):
        host_render_bev(rc.make_config(32, 30), layers=[BoxLayer(boxes)])                   # W % 4
    skew = rc.make_config(32, 32)
    skew.voxel_size = (0.25, 0.5, 0.4)
    with pytest.raises(ValueError):
        host_render_bev(skew, layers=[BoxLayer(boxes)])
    with pytest.raises(ValueError):
        host_render_bev(cfg, heat=np.zeros((1, 5, 8), np.float32))                          # 32 % 5


# ---------------------------------------------------------------------------
# PNG
# ---------------------------------------------------------------------------
def test_png_round_trip(tmp_path):
    from disconet_amd.render import read_png, write_png
    img = rc.host_image(rc.MAIN)[0]
    path = str(tmp_path / "main.png")
    write_png(path, img)
    back = read_png(path)
    assert back.dtype == np.uint8 and back.shape == img.shape and (back == img).all()
    odd = np.random.RandomState(0).randint(0, 256, (5, 7, 3)).astype(np.uint8)              # a width that is no multiple of 4
    write_png(str(tmp_path / "odd.png"), odd)
    assert (read_png(str(tmp_path / "odd.png")) == odd).all()
    with pytest.raises(ValueError):
        write_png(str(tmp_path / "bad.png"), odd[..., :2])
    try:
        from PIL import Image
    except ImportError:
        return
    with Image.open(path) as im:
        assert im.mode == "RGB" and (np.asarray(im) == img).all()


# ---------------------------------------------------------------------------
# the tool's command line, the binding
# ---------------------------------------------------------------------------
def _tool():
    spec = importlib.util.spec_from_file_location("render_tool_visualize_codet",
                                                  os.path.join(ROOT, "tools", "det", "visualize_codet.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_tool_parser_and_attention_refusal():
    from disconet_amd import ALL_DET_COM_MODES
    mod = _tool()
    args = mod.build_vis_parser().parse_args(["--com", "late", "--scale", "4", "--tracks", "1", "--frames", "2"])
    assert (args.com, args.scale, args.tracks, args.frames, args.attention, args.gt, args.map_hw) == (
        "late", 4, 1, 2, 0, "scene", 256)
    assert args.pre_nms_top_k == 300 and args.max_age == 1
    with pytest.raises(SystemExit):
        mod.build_vis_parser().parse_args(["--scale", "3"])
    for com in ALL_DET_COM_MODES:
        if com != "disco":
            with pytest.raises(SystemExit) as e:
                mod.main(["--com", com, "--attention", "1"])
            assert "--com disco only" in str(e.value)
    with pytest.raises(SystemExit):
        mod.main(["--com", "v2v"])
    assert mod.image_name("frame", 3, 5, 2) == "frame_f003_agent2_scene1.png"
    assert mod.image_name("attention", 0, 1, 1) == "attention_f000_agent1.png"


def test_library_exports_the_renderer():
    from disconet_amd import _lib, render
    assert "dn_render_bev" in _lib.SIGNATURES
    lib = _lib.load()
    assert lib.dn_render_bev is not None and lib.dn_version() >= 151
    header = open(os.path.join(ROOT, "include", "disconet_hip.h")).read()
    body = re.search(r"#define DN_RENDER_ID_PALETTE \{(.*?)\}", header, flags=re.S).group(1).replace("\\", " ")
    assert [int(v) for v in body.replace(",", " ").split()] == render.ID_PALETTE.reshape(-1).tolist()
    import ctypes
    assert ctypes.sizeof(render._RenderSet) == 64 and ctypes.sizeof(render._RenderDesc) == 128 + 4 * 64
    import disconet_amd
    for name in ("BoxLayer", "render_bev", "host_render_bev", "attention_sheet", "write_png", "read_png"):
        assert name in disconet_amd.__all__ and hasattr(disconet_amd, name)
