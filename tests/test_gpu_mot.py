"""Tracking evaluation on the GPU (tracking.ClearMot, dn_mot_step) against its host reference (tracking.HostClearMot).
The state lives on the device for the whole sequence and is never re-seeded from the host; after every frame the three
outputs, the status words and the whole state are compared AS BITS."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import mot_cases as C
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mixed():
    return C.mixed_sequence()


# ---- 1. mixed images -------------------------------------------------------------------------------------------------
def test_mixed_images_equal_host_bits(mixed):
    assert any(int(gt["count"][0]) == 0 for _, gt in mixed) and all(int(tracks["count"][2]) == 0 for tracks, _ in mixed)
    dev, host, outs = C.run_both(mixed, scale=C.SCALE)
    got, want = dev.compute(), host.compute()
    assert got == want and host.status_words().tolist() == [0, 0, 0]
    image = want["per_image"]
    assert image[0]["frames"] == 12 and image[0]["TP"] + image[0]["FN"] == 9 * 6      # three frames without ground truth
    assert image[2]["TP"] == 0 and image[2]["FP"] == 0 and image[2]["FN"] == 12 * 6 and image[2]["ML"] == 6
    assert image[1]["TP"] > 20 and want["overall"]["IDSW"] + want["overall"]["Frag"] >= 1
    assert any((out["flags"] & 4).any() for out in outs[1:])    # a segment starts after the first frame


# ---- 2. past one wave, both orientations, a real assignment ------------------------------------------------------------
def test_chain_past_one_wave_both_orientations():
    from disconet_amd import tracking
    frames = C.chain_frames()
    shapes = [(int(gt["count"][0]), int(tracks["count"][0])) for tracks, gt in frames]
    assert shapes == [(70, 65), (65, 70)]
    probe = tracking.HostClearMot(1, iou_threshold=0.3, scale=C.SCALE)
    for (tracks, gt), shape in zip(frames, shapes):
        probe.update(tracks, gt)
        score = probe.last_score[0]
        assert score.shape == shape and ((score > 0).sum(1) >= 2).any()      # a condition of the test: no trivial rows
    dev, host, outs = C.run_both(frames, iou_threshold=0.3, scale=C.SCALE)
    assert int((outs[0]["flags"][0] & 1).sum()) == 65 and int((outs[1]["flags"][0] & 1).sum()) == 65
    figures = dev.compute()["overall"]
    assert (figures["TP"], figures["FP"], figures["FN"]) == (130, 5, 5)
    # every ground truth took the track of its own chain position, not the neighbour's
    assert all(int(outs[0]["match"][0, r]) in (-1, int(frames[0][1]["ids"][0, r]) + 1) for r in range(70))


# ---- 3. the scripted sequence ----------------------------------------------------------------------------------------
def test_scripted_continuity_switch_and_gap():
    frames, want = C.scripted_sequence()
    dev, host, outs = C.run_both(frames, iou_threshold=0.5, scale=1.0)
    C.check_scripted(outs, dev.compute(), want)


# ---- 4. the status bits ----------------------------------------------------------------------------------------------
def _status_cases():
    box, far = C.rect_box(0.0, 0.0, 4.0, 2.0), C.rect_box(50.0, 0.0, 54.0, 2.0)
    many = [(i, C.rect_box(8.0 * i, 0.0, 8.0 * i + 4.0, 2.0)) for i in range(130)]
    return [(4, "max_gt_ids", C.gt_frame([[(256, box), (0, far)]])), (8, "twice", C.gt_frame([[(5, box), (5, far)]])),
            (2, "invalid", C.gt_frame([[(0, C.T.aligned(2.0, 1.0, 0.0, 2.0)), (1, far)]])),
            (1, "128", C.gt_frame([many], g=130))]


@pytest.mark.parametrize("case", range(4))
def test_status_bits_alone_and_sticky_until_reset(case):
    from disconet_amd import tracking
    bit, word, gt = _status_cases()[case]
    tracks = C.tracks_frame([[(1, (0.0, 0.0, 4.0, 2.0))]])
    clean = C.gt_frame([[(0, C.rect_box(0.0, 0.0, 4.0, 2.0))]], g=gt["ids"].shape[1])
    dev, host, outs = C.run_both([(tracks, gt), (tracks, clean)], scale=1.0)
    assert dev.status_words().tolist() == [bit]
    with pytest.raises(Exception, match=word):
        dev.compute()
    dev.reset()
    fresh = tracking.HostClearMot(1, scale=1.0)
    fresh.update(tracks, clean)
    fresh.reset()
    assert dev.status_words().tolist() == [0] and np.array_equal(dev.state_bytes(), fresh.state_bytes())
    got, want = C.to_host(dev.update(C.to_device(tracks), C.to_device(clean))), fresh.update(tracks, clean)
    C.assert_same_bits(got, want, "after reset")
    assert np.array_equal(dev.state_bytes(), fresh.state_bytes()) and dev.compute()["overall"]["TP"] == 1


# ---- 5. capture: the tracker and its evaluation in one graph -----------------------------------------------------------
def test_captured_sort_and_evaluation_equal_eager_and_host():
    import torch
    from disconet_amd import graph, tracking
    from disconet_amd.synthetic import make_track_sequence
    from tests import track_cases as T
    seq = make_track_sequence(10, 3, seed=2, p_miss=0.3, truth=True)
    static_det, static_gt = T.to_device(seq[0][0]), C.to_device(seq[0][2])
    sort, mot = tracking.Sort(scale=C.SCALE), tracking.ClearMot(1, scale=C.SCALE)
    step = graph.GraphedStep(lambda: mot.update(sort.update(static_det), static_gt))
    sort.reset()                                                 # the warm-up runs advanced the tracker ...
    mot.reset()                                                  # ... and were counted
    eager_sort, eager = tracking.Sort(scale=C.SCALE), tracking.ClearMot(1, scale=C.SCALE)
    host_sort, host = tracking.HostSort(scale=C.SCALE), tracking.HostClearMot(1, scale=C.SCALE)
    for f, (det, _, gt) in enumerate(seq):
        fresh_det, fresh_gt = T.to_device(det), C.to_device(gt)
        for key in static_det:
            static_det[key].copy_(fresh_det[key])
        for key in static_gt:
            static_gt[key].copy_(fresh_gt[key])
        got = C.to_host(step())
        C.assert_same_bits(got, C.to_host(eager.update(eager_sort.update(fresh_det), fresh_gt)), "replay %d vs eager" % (f + 1))
        C.assert_same_bits(got, host.update(host_sort.update(det), gt), "replay %d vs host" % (f + 1))
    step.drain()
    torch.cuda.synchronize()
    assert np.array_equal(mot.state_bytes(), eager.state_bytes()) and np.array_equal(mot.state_bytes(), host.state_bytes())
    assert mot.compute() == host.compute() and host.compute()["overall"]["TP"] > 50


# ---- 6. determinism --------------------------------------------------------------------------------------------------
def test_two_runs_write_the_same_state_bytes(mixed):
    from disconet_amd import tracking
    runs = []
    for _ in range(2):
        mot = tracking.ClearMot(1, scale=C.SCALE)
        for tracks, gt in mixed:
            out = mot.update(C.to_device(tracks), C.to_device(gt))
        runs.append((mot.state_bytes(), C.to_host(out)))
    assert np.array_equal(runs[0][0], runs[1][0]) and runs[0][0].any()
    C.assert_same_bits(runs[0][1], runs[1][1], "second run")


# ---- 7. the tool -----------------------------------------------------------------------------------------------------
def test_eval_sort_boxes_prints_the_host_figures():
    from disconet_amd import tracking
    from disconet_amd.synthetic import make_track_sequence
    tool = os.path.join(ROOT, "tools", "track", "eval_sort.py")
    run = subprocess.run([sys.executable, tool, "--com", "disco", "--source", "boxes", "--frames", "8", "--num_agent", "2",
                          "--batch", "1"], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    sort, host = tracking.HostSort(scale=C.SCALE), tracking.HostClearMot(1, scale=C.SCALE)
    for det, _, gt in make_track_sequence(8, 2, seed=0, truth=True):      # the tool's defaults
        host.update(sort.update(det), gt)
    want = host.compute()
    lines = run.stdout.splitlines()
    assert tracking.mot_line("overall", want["overall"]) in lines, run.stdout[-2000:]
    for a in range(2):
        assert tracking.mot_line("agent %d" % a, want["per_agent"][a]) in lines
    assert 0.0 < want["overall"]["MOTA"] < 1.0
