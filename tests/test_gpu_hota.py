"""HOTA on the GPU (tracking.Hota, dn_hota_step / dn_hota_finish) against its host reference (tracking.HostHota).  The
state lives on the device for the whole sequence and is never re-seeded from the host; after every frame `potential`, the
status words and the whole state are compared AS BITS, after the last frame finish()'s four tensors."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import hota_cases as H
from tests import idf_cases as I
from tests import mot_cases as C
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def generated():
    return C.generated_sequence(12, 3, 2, p_miss=0.3)


# ---- 1. generated sequences ------------------------------------------------------------------------------------------
def test_generated_images_equal_host_bits(generated):
    dev, host, outs = H.run_both(generated, scale=C.SCALE, **H.SIZES)
    assert host.status_words().tolist() == [0, 0, 0]
    image = dev.compute()["per_image"]
    for level in image:
        assert level["frames"] == level["logged"] == 12 and level["GT_Dets"] == 72 and level["GT_IDs"] == 6
        assert level["TP"][0] > 20 and level["TP"][18] < level["TP"][0] and 0.0 < level["HOTA"] < 1.0
    assert any(out["potential"].any() for out in outs)


def test_images_of_different_lengths_and_empty_frames():
    seq = H.ragged_sequence()
    shapes = {(int(gt["count"][i]) > 0, int(tracks["count"][i]) > 0) for tracks, gt in seq for i in range(3)}
    assert shapes == {(True, True), (False, True), (True, False), (False, False)}     # V = 0, C = 0 and both are there
    dev, host, _ = H.run_both(seq, scale=C.SCALE, **H.SIZES)
    assert host.status_words().tolist() == [0, 0, 0]
    image = dev.compute()["per_image"]
    assert [level["GT_Dets"] for level in image] == [72, 48, 60] and [level["logged"] for level in image] == [12] * 3
    assert image[1]["TP"][0] > 10 and image[2]["FN"][0] >= 12


# ---- 2. by hand ------------------------------------------------------------------------------------------------------
def test_swap_sequence_by_hand():
    dev, host, _ = H.run_both(I.swap_sequence()[0], scale=1.0, **H.SIZES)
    H.check_swap(dev)


def test_alpha_edges_by_hand():
    dev, host, _ = H.run_both([H.alpha_edge_frame()], scale=1.0, **H.SIZES)
    H.check_alpha_edges(dev)


def test_the_global_alignment_decides():
    dev, host, _ = H.run_both(H.alignment_sequence(), scale=1.0, **H.SIZES)
    H.check_alignment(dev)


# ---- 3. the largest launch -------------------------------------------------------------------------------------------
def test_128_tracks_and_128_ground_truths():
    frames = H.dense_frames()
    dev, host, _ = H.run_both(frames, scale=1.0, max_gt_ids=128, max_track_ids=256, max_frames=2)
    assert host.status_words().tolist() == [0]
    counts = dev.finish()["counts"].cpu().numpy()
    assert counts.tolist() == [[2, 2, 256, 256, 128, 129, 0, 0]]
    match = dev.matches(0)
    assert match.shape == (2, 128) and (match > 0).sum() > 200                       # nearly every row of both frames is kept
    assert len(set(match[0][match[0] > 0].tolist())) == int((match[0] > 0).sum())    # a matching: no track id twice
    level = dev.compute()["overall"]
    assert level["TP"][0] > 200 and level["TP"][18] == 0 and 0.0 < level["HOTA"] < 1.0


def test_assignment_past_one_wave_in_both_orientations():
    """mot_cases.chain_frames(): 70 ground truths x 65 tracks (the match kernel's rows are the tracks, its 70 columns the
    ground truths), then 65 x 70 -- the smallest frames whose columns cross a wave in either orientation."""
    from disconet_amd import tracking
    frames = C.chain_frames()
    sizes = dict(scale=C.SCALE, max_gt_ids=128, max_track_ids=256, max_frames=2)
    alone = tracking.HostHota(1, **sizes)                  # the conditions of the test, from the host reference alone
    for tracks, gt in frames:
        alone.update(tracks, gt)
    assert alone.status_words().tolist() == [0]
    log = alone.images[0]["log"]
    assert [(len(slot["gid"]), len(slot["tid"])) for slot in log] == [(70, 65), (65, 70)]
    for slot in log:                                       # some row holds two or more overlaps: the assignment is not trivial
        assert ((tracking._iou_matrix(slot["grect"], slot["trect"]) > 0).sum(1) >= 2).any()
    dev, host, _ = H.run_both(frames, **sizes)
    assert host.status_words().tolist() == [0]


# ---- 4. the rows that are ignored ------------------------------------------------------------------------------------
def test_duplicate_track_id_is_counted_nowhere():
    dev, host, outs = H.run_both([H.twice_frame()], scale=1.0, **H.SIZES)
    H.check_twice(outs[0], dev)


def test_the_log_fills():
    frames = I.swap_sequence()[0][:3]
    sizes = dict(H.SIZES, max_frames=2)
    two, _, _ = H.run_both(frames[:2], scale=1.0, **sizes)
    after_two, fin_two = two.state_bytes(), {key: value.cpu().numpy() for key, value in two.finish().items()}
    full, host, outs = H.run_both(frames, scale=1.0, **sizes)
    assert full.status_words().tolist() == [32] and not outs[2]["potential"].any()
    a = full.state_bytes()
    assert a[:8].view(np.int64)[0] == 3 and after_two[:8].view(np.int64)[0] == 2
    assert np.array_equal(a[8:32], after_two[8:32]) and np.array_equal(a[36:], after_two[36:])
    fin = {key: value.cpu().numpy() for key, value in full.finish().items()}
    H.assert_same_bits(fin, fin_two, "three frames into two slots", keys=("alpha_counts", "alpha_sums", "match"))
    assert fin["counts"].tolist() == [[3, 2, 4, 4, 2, 2, 32, 0]] and fin_two["counts"].tolist() == [[2, 2, 4, 4, 2, 2, 0, 0]]
    with pytest.raises(Exception, match="log was full"):
        full.compute()


@pytest.mark.parametrize("case", range(9))
def test_status_bits_alone_and_sticky_until_reset(case):
    from disconet_amd import tracking
    bit, word, frames, params = H.status_cases()[case]
    dev, host, outs = H.run_both(frames, scale=1.0, **params)
    assert dev.status_words().tolist() == [bit] and int(dev.finish()["counts"][0, 6]) == bit
    with pytest.raises(Exception, match=word):
        dev.compute()
    dev.reset()
    clean = frames[-1]
    fresh = tracking.HostHota(1, scale=1.0, **params)
    fresh.update(*clean)
    fresh.reset()
    assert dev.status_words().tolist() == [0] and np.array_equal(dev.state_bytes(), fresh.state_bytes())
    got, want = dev.update(C.to_device(clean[0]), C.to_device(clean[1])), fresh.update(*clean)
    H.assert_same_bits(got, want, "after reset")
    assert np.array_equal(dev.state_bytes(), fresh.state_bytes()) and dev.compute()["overall"]["TP"] == [1] * 19
    H.assert_same_end(dev, fresh)


# ---- 5. capture: the tracker and the three evaluations in one graph, the finish in a second ----------------------------
def test_captured_step_and_finish_equal_eager_and_host():
    import torch
    from disconet_amd import graph, tracking
    from disconet_amd.synthetic import make_track_sequence
    seq = make_track_sequence(10, 3, seed=2, p_miss=0.3, truth=True)
    static_det, static_gt = C.T.to_device(seq[0][0]), C.to_device(seq[0][2])
    sort, mot, idf = tracking.Sort(scale=C.SCALE), tracking.ClearMot(1, scale=C.SCALE), tracking.Identity(1, scale=C.SCALE)
    hota = tracking.Hota(1, scale=C.SCALE, **H.SIZES)

    def tracked():
        tracks = sort.update(static_det)
        return mot.update(tracks, static_gt), idf.update(tracks, static_gt), hota.update(tracks, static_gt)

    step = graph.GraphedStep(tracked)
    for stage in (sort, mot, idf, hota):                         # the warm-up runs advanced the tracker and were logged
        stage.reset()
    eager_sort, eager = tracking.Sort(scale=C.SCALE), tracking.Hota(1, scale=C.SCALE, **H.SIZES)
    host_sort, host_mot, host = (tracking.HostSort(scale=C.SCALE), tracking.HostClearMot(1, scale=C.SCALE),
                                 tracking.HostHota(1, scale=C.SCALE, **H.SIZES))
    for f, (det, _, gt) in enumerate(seq):
        fresh_det, fresh_gt = C.T.to_device(det), C.to_device(gt)
        for key in static_det:
            static_det[key].copy_(fresh_det[key])
        for key in static_gt:
            static_gt[key].copy_(fresh_gt[key])
        got_mot, _, got = step()
        got_mot, got = C.to_host(got_mot), {"potential": got["potential"].cpu().numpy()}
        H.assert_same_bits(got, eager.update(eager_sort.update(fresh_det), fresh_gt), "replay %d vs eager" % (f + 1))
        tracks = host_sort.update(det)
        H.assert_same_bits(got, host.update(tracks, gt), "replay %d vs host" % (f + 1))
        C.assert_same_bits(got_mot, host_mot.update(tracks, gt), "replay %d: ClearMot vs host" % (f + 1))
    step.drain()
    torch.cuda.synchronize()
    assert np.array_equal(hota.state_bytes(), eager.state_bytes()) and np.array_equal(hota.state_bytes(), host.state_bytes())
    want = {key: value.cpu().numpy() for key, value in hota.finish().items()}
    H.assert_same_bits(want, host.finish(), "eager finish vs host", keys=H.FIN_KEYS)
    H.assert_same_bits(eager.finish(), want, "the eager run's finish", keys=H.FIN_KEYS)
    finish = graph.GraphedStep(hota.finish)
    for replay in range(2):
        H.assert_same_bits(finish(), want, "finish replay %d" % (replay + 1), keys=H.FIN_KEYS)
    finish.drain()
    assert np.array_equal(hota.state_bytes(), host.state_bytes())            # the finish left the state alone
    assert hota.compute() == host.compute() and host.compute()["overall"]["TP"][0] > 50


# ---- 6. determinism and reuse ------------------------------------------------------------------------------------------
def test_two_runs_write_the_same_bytes_and_finish_leaves_the_state(generated):
    from disconet_amd import tracking
    runs = []
    for run in range(2):
        hota = tracking.Hota(1, scale=C.SCALE, **H.SIZES)
        for f, (tracks, gt) in enumerate(generated):
            hota.update(C.to_device(tracks), C.to_device(gt))
            if run == 1 and f == 5:                                # a finish in the middle of the sequence
                before = hota.state_bytes()
                middle = hota.compute()["overall"]
                assert np.array_equal(hota.state_bytes(), before) and middle["frames"] == 18 == middle["logged"]
        fin = hota.finish()
        runs.append((hota.state_bytes(),) + tuple(fin[key].cpu().numpy() for key in H.FIN_KEYS))
    assert runs[0][0].any() and runs[0][2][:, 0, 0].sum() > 60
    for a, b in zip(runs[0], runs[1]):
        assert np.array_equal(C.bits(a), C.bits(b))


# ---- 7. the tool -----------------------------------------------------------------------------------------------------
def test_eval_sort_boxes_prints_the_host_hota_figures():
    from disconet_amd import tracking
    from disconet_amd.synthetic import make_track_sequence
    tool = os.path.join(ROOT, "tools", "track", "eval_sort.py")
    run = subprocess.run([sys.executable, tool, "--com", "disco", "--source", "boxes", "--frames", "8", "--num_agent", "2",
                          "--batch", "1"], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    sort = tracking.HostSort(scale=C.SCALE)
    idf, host = tracking.HostIdentity(1, scale=C.SCALE), tracking.HostHota(1, scale=C.SCALE, max_frames=8)
    for det, _, gt in make_track_sequence(8, 2, seed=0, truth=True):      # the tool's defaults
        tracks = sort.update(det)
        idf.update(tracks, gt)
        host.update(tracks, gt)
    want, identity = host.compute(), idf.compute()
    lines = run.stdout.splitlines()
    assert tracking.hota_line("overall", want["overall"]) in lines, run.stdout[-2000:]
    for a in range(2):
        assert tracking.hota_line("agent %d" % a, want["per_agent"][a]) in lines
    assert lines.index(tracking.idf_line("overall", identity["overall"])) < lines.index(tracking.hota_line("agent 0", want["per_agent"][0]))
    assert 0.0 < want["overall"]["HOTA"] < 1.0
