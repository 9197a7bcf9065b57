"""The tracker on the GPU (tracking.Sort, dn_track_step) against its host reference (tracking.HostSort).  The state
lives on the device for the whole sequence and is never re-seeded from the host; after every frame all integer outputs,
det_track, the status words, the fp64 rectangles and the state bytes are compared AS BITS."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import track_cases as C
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mixed():
    return C.mixed_sequence()


# ---- 1. mixed images -------------------------------------------------------------------------------------------------
def test_mixed_images_equal_host_bits(mixed):
    seq, invalid = mixed
    sort, host, outs, paths = C.run_both(seq, scale=C.SCALE)
    assert any(int(det["count"][0]) == 0 for det in seq) and all(int(det["count"][1]) == 8 for det in seq)
    assert host.status_words().tolist() == [0, 0, 2]            # the invalid rows: status bit 1 and no other trace
    for img, frame, row in invalid:
        assert outs[frame]["det_track"][img, row] == -1
    assert max(int(o["count"].max()) for o in outs) >= 4 and any("shortcut" in p for p in paths)
    with pytest.raises(Exception, match="image 2"):
        sort.status()


# ---- 2. past one wave, on the Hungarian path -------------------------------------------------------------------------
def test_chain_of_70_runs_the_hungarian_step():
    seq = C.chain_sequence()
    assert [int(d["count"][0]) for d in seq] == [70, 70, 67, 65, 70]
    sort, host, outs, paths = C.run_both(seq, scale=C.SCALE)
    assert paths[0] == ["none"] and all(p == ["hungarian"] for p in paths[1:])      # a condition of the test
    assert int(outs[0]["count"][0]) == 70 and (outs[1]["det_track"][0, :70] == np.arange(1, 71)).all()
    tracks = [int(np.frombuffer(host.state_bytes()[:16].tobytes(), dtype=np.int32)[2])]
    assert tracks == [70]                                       # 67 survivors of frame 4 + the three that came back
    assert sort.status() == 0


# ---- 3. capacity -----------------------------------------------------------------------------------------------------
def test_capacity_bits_are_sticky_until_reset():
    seq = [C.pad([C.grid_rows(6)], k=6), C.pad([C.grid_rows(2)], k=6)]
    sort, host, outs, _ = C.run_both(seq, scale=C.SCALE, max_tracks=4)
    assert outs[0]["det_track"][0].tolist() == [1, 2, 3, 4, -1, -1]
    assert sort.status_words().tolist() == [1]
    with pytest.raises(Exception, match="max_tracks"):
        sort.status()
    sort.reset()
    host.reset()
    assert sort.status() == 0 and np.array_equal(sort.state_bytes(), host.state_bytes())
    got, want = C.to_host(sort.update(C.to_device(seq[1]))), host.update(seq[1])
    C.assert_same_bits(got, want, "after reset")
    assert want["det_track"][0].tolist() == [1, 2, -1, -1, -1, -1]


def test_more_than_128_valid_rows_set_bit_2():
    seq = [C.pad([C.grid_rows(130)], k=136), C.pad([C.grid_rows(130)], k=136)]
    sort, host, outs, paths = C.run_both(seq, scale=C.SCALE)
    assert sort.status_words().tolist() == [4]
    assert (outs[0]["det_track"][0, :128] == np.arange(1, 129)).all() and (outs[0]["det_track"][0, 128:] == -1).all()
    assert paths[1] == ["shortcut"] and int(outs[1]["count"][0]) == 128


# ---- 4. ties ---------------------------------------------------------------------------------------------------------
def test_ties_take_the_lowest_index():
    sort, host, outs, paths = C.run_both(C.tie_sequence(), scale=C.SCALE)
    assert paths == [["none"], ["hungarian"], ["shortcut"], ["hungarian"], ["hungarian"]]
    assert outs[1]["det_track"][0].tolist() == [1, 2, -1, -1]     # two identical detections: the lower row keeps track 1
    assert outs[2]["det_track"][0].tolist() == [3, 4, 5, -1]      # every IoU 0: nothing matched, three births
    assert outs[3]["det_track"][0].tolist() == [1, 2, -1, -1]     # equal 2 x 2: track 1 / row 0, track 2 / row 1


# ---- 5. capture ------------------------------------------------------------------------------------------------------
def test_captured_step_equals_eager(mixed):
    from disconet_amd import graph, tracking
    seq = mixed[0][:10]
    static = C.to_device(seq[0])
    sort = tracking.Sort(scale=C.SCALE)
    step = graph.GraphedStep(lambda: sort.update(static))
    sort.reset()                                                 # the warm-up runs advanced the tracker
    eager, host = tracking.Sort(scale=C.SCALE), tracking.HostSort(scale=C.SCALE)
    for f, det in enumerate(seq):
        fresh = C.to_device(det)
        for key in static:
            static[key].copy_(fresh[key])
        got = C.to_host(step())
        C.assert_same_bits(got, C.to_host(eager.update(fresh)), "replay %d vs eager" % (f + 1))
        C.assert_same_bits(got, host.update(det), "replay %d vs host" % (f + 1))
    step.drain()
    assert np.array_equal(sort.state_bytes(), eager.state_bytes())
    assert np.array_equal(sort.state_bytes(), host.state_bytes())


# ---- 6. determinism --------------------------------------------------------------------------------------------------
def test_two_runs_write_the_same_state_bytes(mixed):
    from disconet_amd import tracking
    runs = []
    for _ in range(2):
        sort = tracking.Sort(scale=C.SCALE)
        for det in mixed[0]:
            out = sort.update(C.to_device(det))
        runs.append((sort.state_bytes(), C.to_host(out)))
    assert np.array_equal(runs[0][0], runs[1][0])
    C.assert_same_bits(runs[0][1], runs[1][1], "second run")


# ---- 7. the tool -----------------------------------------------------------------------------------------------------
def test_sort_codet_boxes_writes_the_host_rows(tmp_path):
    from disconet_amd import tracking
    from disconet_amd.synthetic import make_track_sequence
    tool = os.path.join(ROOT, "tools", "track", "sort_codet.py")
    run = subprocess.run([sys.executable, tool, "--com", "disco", "--source", "boxes", "--frames", "8", "--num_agent", "2",
                          "--batch", "1", "--logpath", str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    host = tracking.HostSort(scale=C.SCALE)
    want = [[], []]
    for f, (det, _) in enumerate(make_track_sequence(8, 2, seed=0)):      # the tool's defaults
        for img, rows in enumerate(tracking.mot_rows(host.update(det), f + 1)):
            want[img] += rows
    files = sorted(os.listdir(str(tmp_path)))
    assert files == ["tracks_agent0.txt", "tracks_agent1.txt"], files
    for img, name in enumerate(files):
        got = open(os.path.join(str(tmp_path), name)).read().splitlines()
        assert got == want[img] and len(got) > 8, name
    assert "kept a single track id" in run.stdout
