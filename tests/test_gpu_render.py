"""dn_render_bev on the MI355X against render.host_render_bev: every byte, on every case of tests/render_cases.py, from
the eager call and from a graph replay, through the library's own dicts, the DiscoGraph sheet and the tool."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import render_cases as rc

pytestmark = pytest.mark.gpu


def _same(got, want):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == want.shape and got.dtype == np.uint8
    bad = np.argwhere((got != want).any(-1))
    assert len(bad) == 0, "%d pixels differ, first (image, row, column) %s: %s against %s" % (
        len(bad), bad[:4].tolist(), got[tuple(bad[0])].tolist(), want[tuple(bad[0])].tolist())


@pytest.mark.parametrize("name", rc.names())
def test_render_equals_the_host_statement(name):
    from disconet_amd import render_bev
    c = rc.case(name)
    _same(render_bev(c["config"], **rc.to_device(c)), rc.host_image(name))


def test_two_runs_write_the_same_bytes_and_out_is_overwritten():
    from disconet_amd import render_bev
    c = rc.case(rc.MAIN)
    kw = rc.to_device(c)
    first = render_bev(c["config"], **kw)
    canvas = torch.full_like(first, 77)
    assert render_bev(c["config"], out=canvas, **kw) is canvas
    assert torch.equal(first, canvas)
    _same(canvas, rc.host_image(rc.MAIN))


def test_refused_on_the_device():
    from disconet_amd import BoxLayer, render_bev
    from disconet_amd._lib import DnError
    cfg = rc.make_config(32, 32)
    boxes = torch.zeros((1, 2, 6), device="cuda")
    with pytest.raises(DnError):
        render_bev(cfg, layers=[BoxLayer(boxes.cpu())])
    with pytest.raises(DnError):
        render_bev(cfg, layers=[BoxLayer(boxes.cpu().numpy())])
    with pytest.raises(ValueError):
        render_bev(cfg, layers=[BoxLayer(boxes)], out=torch.empty((1, 64, 64, 4), dtype=torch.uint8, device="cuda"))


# ---------------------------------------------------------------------------
# behind the tail: detect() and Sort.update(), eager and replayed
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tail():
    """a small model output (random heads on a 32 x 32 map, 3 images) and its detections"""
    from disconet_amd import Config, postprocess
    cfg = Config(map_hw=32)
    anchors = postprocess.make_anchors(cfg)
    g = torch.Generator().manual_seed(5)
    apl = 32 * 32 * len(cfg.anchor_size)
    result = {"cls": (torch.randn((3, apl, 2), generator=g) * 2).cuda(),
              "loc": (torch.randn((3, 32, 32, len(cfg.anchor_size), 1, 6), generator=g) * 0.3).cuda()}
    words = torch.as_tensor(rc.make_words(np.random.RandomState(3), 32, 32)).cuda()
    return cfg, anchors, result, words


def _host_det(det):
    from disconet_amd import postprocess
    rows = postprocess.detections_to_host(det)
    return postprocess.pad_detections([r[0] for r in rows], [r[1] for r in rows], width=det["scores"].shape[1])


def test_detections_and_tracks_render_as_their_host_twins(tail):
    from disconet_amd import BoxLayer, host_render_bev, postprocess, render_bev, tracking
    cfg, anchors, result, words = tail
    det = postprocess.detect(result, anchors, pre_nms_top_k=40, iou_thr=0.05)
    report = tracking.Sort(scale=1.0 / cfg.voxel_size[0]).update(det)
    got = render_bev(cfg, background=words, layers=[BoxLayer.detections(det, fill_alpha=60), BoxLayer.tracks(det, report)],
                     scale=2)
    host = _host_det(det)
    assert host["count"].min() >= 3                                  # something is drawn in every image
    twin = {"det_track": report["det_track"].cpu().numpy()}
    assert (twin["det_track"] >= 0).sum() >= 3
    want = host_render_bev(cfg, background=words.cpu().numpy(),
                           layers=[BoxLayer.detections(host, fill_alpha=60), BoxLayer.tracks(host, twin)], scale=2)
    _same(got, want)
    assert (want != host_render_bev(cfg, background=words.cpu().numpy(), scale=2)).any(-1).mean() >= 0.01
    # BoxLayer.host() is the same twin
    _same(got, host_render_bev(cfg, background=words.cpu().numpy(), scale=2,
                               layers=[BoxLayer.detections(det, fill_alpha=60).host(), BoxLayer.tracks(det, report).host()]))


def test_graph_replay_writes_the_eager_bytes(tail):
    from disconet_amd import BoxLayer, postprocess, render_bev
    from disconet_amd.graph import GraphedStep
    cfg, anchors, result, words = tail

    def step():
        det = postprocess.detect(result, anchors, pre_nms_top_k=40, iou_thr=0.05)
        return render_bev(cfg, background=words, layers=[BoxLayer.detections(det)], scale=4)

    eager = step().clone()
    graphed = GraphedStep(step)
    replay = graphed().clone()
    graphed.drain()
    assert torch.equal(replay, eager)
    # the captured step follows its static inputs: other heads, other picture, again the eager bytes
    saved = result["cls"].clone()
    result["cls"].copy_(saved.flip(0))
    try:
        replay2 = graphed().clone()
        graphed.drain()
        eager2 = step()
        assert torch.equal(replay2, eager2) and not torch.equal(replay2, eager)
    finally:
        result["cls"].copy_(saved)


# ---------------------------------------------------------------------------
# the DiscoGraph sheet
# ---------------------------------------------------------------------------
def test_attention_sheet_equals_the_host_composition():
    from disconet_amd import Config, DiscoNet, attention_sheet, host_render_bev, render
    from disconet_amd.synthetic import make_scene_batch
    cfg = Config(map_hw=128)
    torch.manual_seed(2)
    model = DiscoNet(cfg, kd_flag=0, num_agent=2).eval().cuda()
    bevs, trans, na = make_scene_batch(1, 2, 128)
    bevs = bevs.cuda()
    weights = render.disco_weights(model, bevs, trans.cuda(), na.cuda(), 1)
    assert tuple(weights.shape) == (1, 2, 2, 16 * 16)
    words = render.occupancy_words(bevs)                             # the dense grid through ops.scatter_dense_bits
    assert tuple(words.shape) == (2, 128, 128)
    dense = bevs.cpu().numpy()
    for ego in (0, 1):
        sheet = attention_sheet(cfg, words, weights, 0, ego, 2, scale=2)
        assert tuple(sheet.shape) == (256, 2 * 256, 3) and sheet.dtype == torch.uint8
        want = attention_sheet(cfg, dense[ego:ego + 1], weights.cpu().numpy(), 0, ego, 2, scale=2, render=host_render_bev)
        _same(sheet, want)
        plain = host_render_bev(cfg, background=dense[ego:ego + 1], scale=2)[0]
        assert (want[:, :256] != plain).any(-1).mean() >= 0.01      # the overlay is there
    # a padded ego has a list of one: its own map
    assert tuple(attention_sheet(cfg, words, weights, 0, 1, 1, scale=1).shape) == (128, 128, 3)


# ---------------------------------------------------------------------------
# the tool
# ---------------------------------------------------------------------------
def test_tool_writes_the_pictures(tmp_path):
    from disconet_amd.render import GT_COLOUR, SCORE_HI, SCORE_LO, read_png
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path / "vis")
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "det", "visualize_codet.py"), "--com", "disco",
                        "--num_agent", "2", "--frames", "1", "--map_hw", "128", "--attention", "1", "--logpath", out],
                       cwd=root, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert sorted(os.listdir(out)) == ["attention_f000_agent0.png", "attention_f000_agent1.png", "frame_f000_agent0.png",
                                       "frame_f000_agent1.png"], r.stdout
    ramp = {tuple((a * (255 - l) + b * l + 127) // 255 for a, b in zip(SCORE_LO, SCORE_HI)) for l in range(256)}
    for agent in (0, 1):
        img = read_png(os.path.join(out, "frame_f000_agent%d.png" % agent))
        assert img.shape == (256, 256, 3)
        colours = {tuple(c) for c in np.unique(img.reshape(-1, 3), axis=0).tolist()}
        assert tuple(GT_COLOUR) in colours
        assert colours & ramp
        assert read_png(os.path.join(out, "attention_f000_agent%d.png" % agent)).shape == (256, 512, 3)
