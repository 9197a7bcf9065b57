"""Identity metrics on the GPU (tracking.Identity, dn_idf_step / dn_idf_finish) against their host reference
(tracking.HostIdentity).  The state lives on the device for the whole sequence and is never re-seeded from the host; after
every frame `overlaps`, the status words and the whole state are compared AS BITS, after the last frame finish()'s two
tensors."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import idf_cases as I
from tests import mot_cases as C
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mixed():
    return C.mixed_sequence()


# ---- 1. mixed images -------------------------------------------------------------------------------------------------
def test_mixed_images_equal_host_bits(mixed):
    assert any(int(gt["count"][0]) == 0 for _, gt in mixed) and all(int(tracks["count"][2]) == 0 for tracks, _ in mixed)
    dev, host, outs = I.run_both(mixed, scale=C.SCALE)
    assert host.status_words().tolist() == [0, 0, 0]
    image = dev.compute()["per_image"]
    assert image[0]["frames"] == 12 and image[0]["GT_Dets"] == 9 * 6           # three frames without ground truth
    assert image[2]["IDTP"] == 0 and image[2]["IDFN"] == 72 and image[2]["Dets"] == 0 and image[2]["IDs"] == 0
    assert image[2]["GT_IDs"] == 6 and image[1]["IDTP"] > 20 and 0.0 < image[1]["IDF1"] < 1.0
    assert any(out["overlaps"].any() for out in outs)


# ---- 2. a real assignment past one wave, both orientations and an idle image in one launch -----------------------------
@pytest.mark.parametrize("large", [False, True])
def test_seeded_matrices_both_orientations(large):
    shapes, matrices, frames, params = I.matrix_cases(large)
    assert [int(gt["count"][1]) for _, gt in frames[-9:]] == ([0] * 9 if large else [25] * 9)      # image 1 idles at the end
    dev, host, _ = I.run_both(frames, **params)
    assert dev.status_words().tolist() == [0, 0]
    I.check_matrix_run(dev, shapes, matrices)


# ---- 3. by hand ------------------------------------------------------------------------------------------------------
def test_scripted_sequence_by_hand():
    frames, _ = C.scripted_sequence()
    dev, host, outs = I.run_both(frames, iou_threshold=0.5, scale=1.0)
    got = [{"overlaps": o["overlaps"]} for o in outs]
    I.check_scripted(got, dev)


def test_swap_needs_the_global_assignment():
    frames, want = I.swap_sequence()
    dev, host, _ = I.run_both(frames, scale=1.0)
    I.check_swap(dev, want)


def test_the_same_track_id_twice_in_one_frame():
    """the one case that needs the atomic: two lanes bump the same matrix word and the same track_count word"""
    from disconet_amd import tracking
    dev, host, outs = I.run_both([I.twice_frame()], scale=1.0)
    I.check_twice(outs[0], dev)
    many = tracking.Identity(1, scale=1.0)                        # 100 rows with one id on one identity, several frames
    tracks = C.tracks_frame([[(7, I.A)] * 100], m=128)
    gt = C.to_device(I.twice_frame()[1])
    for _ in range(3):
        out = many.update(C.to_device(tracks), gt)
    assert out["overlaps"].cpu()[0].tolist() == [100, 0, 0, 0] and many.counts_matrix(0)[0, 6] == 300
    assert many.finish()["counts"].cpu()[0].tolist() == [3, 3, 300, 300, 1, 1, 0, 0]


# ---- 4. the status bits ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(7))
def test_status_bits_alone_and_sticky_until_reset(case):
    from disconet_amd import tracking
    bit, word, tracks, gt = I.status_cases()[case]
    clean = I.clean_frame(g=gt["ids"].shape[1])
    dev, host, outs = I.run_both([(tracks, gt), clean], scale=1.0)
    assert dev.status_words().tolist() == [bit] and int(dev.finish()["counts"][0, 6]) == bit
    with pytest.raises(Exception, match=word):
        dev.compute()
    dev.reset()
    fresh = tracking.HostIdentity(1, scale=1.0)
    fresh.update(*clean)
    fresh.reset()
    assert dev.status_words().tolist() == [0] and np.array_equal(dev.state_bytes(), fresh.state_bytes())
    got, want = dev.update(C.to_device(clean[0]), C.to_device(clean[1])), fresh.update(*clean)
    I.assert_same_bits(got, want, "after reset")
    assert np.array_equal(dev.state_bytes(), fresh.state_bytes()) and dev.compute()["overall"]["IDTP"] == 1
    I.assert_same_end(dev, fresh)


# ---- 5. capture: the tracker and both evaluations in one graph, the finish in a second ---------------------------------
def test_captured_step_and_finish_equal_eager_and_host():
    import torch
    from disconet_amd import graph, tracking
    from disconet_amd.synthetic import make_track_sequence
    seq = make_track_sequence(10, 3, seed=2, p_miss=0.3, truth=True)
    static_det, static_gt = C.T.to_device(seq[0][0]), C.to_device(seq[0][2])
    sort, mot, idf = tracking.Sort(scale=C.SCALE), tracking.ClearMot(1, scale=C.SCALE), tracking.Identity(1, scale=C.SCALE)

    def tracked():
        tracks = sort.update(static_det)
        return mot.update(tracks, static_gt), idf.update(tracks, static_gt)

    step = graph.GraphedStep(tracked)
    for stage in (sort, mot, idf):                               # the warm-up runs advanced the tracker and were counted
        stage.reset()
    eager_sort, eager = tracking.Sort(scale=C.SCALE), tracking.Identity(1, scale=C.SCALE)
    host_sort, host_mot, host = (tracking.HostSort(scale=C.SCALE), tracking.HostClearMot(1, scale=C.SCALE),
                                 tracking.HostIdentity(1, scale=C.SCALE))
    for f, (det, _, gt) in enumerate(seq):
        fresh_det, fresh_gt = C.T.to_device(det), C.to_device(gt)
        for key in static_det:
            static_det[key].copy_(fresh_det[key])
        for key in static_gt:
            static_gt[key].copy_(fresh_gt[key])
        got_mot, got = step()
        got_mot, got = C.to_host(got_mot), {"overlaps": got["overlaps"].cpu().numpy()}
        I.assert_same_bits(got, eager.update(eager_sort.update(fresh_det), fresh_gt), "replay %d vs eager" % (f + 1))
        tracks = host_sort.update(det)
        I.assert_same_bits(got, host.update(tracks, gt), "replay %d vs host" % (f + 1))
        C.assert_same_bits(got_mot, host_mot.update(tracks, gt), "replay %d: ClearMot vs host" % (f + 1))
    step.drain()
    torch.cuda.synchronize()
    assert np.array_equal(idf.state_bytes(), eager.state_bytes()) and np.array_equal(idf.state_bytes(), host.state_bytes())
    assert np.array_equal(mot.state_bytes(), host_mot.state_bytes())
    want = {key: value.cpu().numpy() for key, value in idf.finish().items()}
    I.assert_same_bits(want, host.finish(), "eager finish vs host", keys=("counts", "match"))
    finish = graph.GraphedStep(idf.finish)
    for replay in range(2):
        I.assert_same_bits(finish(), want, "finish replay %d" % (replay + 1), keys=("counts", "match"))
    finish.drain()
    assert np.array_equal(idf.state_bytes(), host.state_bytes())
    assert idf.compute() == host.compute() and host.compute()["overall"]["IDTP"] > 50


# ---- 6. determinism and reuse ------------------------------------------------------------------------------------------
def test_two_runs_write_the_same_bytes_and_finish_leaves_the_state(mixed):
    from disconet_amd import tracking
    runs = []
    for run in range(2):
        idf = tracking.Identity(1, scale=C.SCALE)
        for f, (tracks, gt) in enumerate(mixed):
            idf.update(C.to_device(tracks), C.to_device(gt))
            if run == 1 and f == 5:                                # a finish in the middle of the sequence
                before = idf.state_bytes()
                middle = idf.compute()["overall"]
                assert np.array_equal(idf.state_bytes(), before) and middle["frames"] == 18
        fin = idf.finish()
        runs.append((idf.state_bytes(), fin["counts"].cpu().numpy(), fin["match"].cpu().numpy()))
    assert runs[0][0].any() and runs[0][1][:, 3].sum() > 20
    for a, b in zip(runs[0], runs[1]):
        assert np.array_equal(C.bits(a), C.bits(b))


# ---- 7. the tool -----------------------------------------------------------------------------------------------------
def test_eval_sort_boxes_prints_the_host_identity_figures():
    from disconet_amd import tracking
    from disconet_amd.synthetic import make_track_sequence
    tool = os.path.join(ROOT, "tools", "track", "eval_sort.py")
    run = subprocess.run([sys.executable, tool, "--com", "disco", "--source", "boxes", "--frames", "8", "--num_agent", "2",
                          "--batch", "1"], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    sort = tracking.HostSort(scale=C.SCALE)
    mot, host = tracking.HostClearMot(1, scale=C.SCALE), tracking.HostIdentity(1, scale=C.SCALE)
    for det, _, gt in make_track_sequence(8, 2, seed=0, truth=True):      # the tool's defaults
        tracks = sort.update(det)
        mot.update(tracks, gt)
        host.update(tracks, gt)
    want, clear = host.compute(), mot.compute()
    lines = run.stdout.splitlines()
    assert tracking.idf_line("overall", want["overall"]) in lines, run.stdout[-2000:]
    assert tracking.mot_line("overall", clear["overall"]) in lines
    for a in range(2):
        assert tracking.idf_line("agent %d" % a, want["per_agent"][a]) in lines
        assert tracking.mot_line("agent %d" % a, clear["per_agent"][a]) in lines
    assert lines.index(tracking.mot_line("overall", clear["overall"])) < lines.index(tracking.idf_line("agent 0", want["per_agent"][0]))
    assert 0.0 < want["overall"]["IDF1"] < 1.0
