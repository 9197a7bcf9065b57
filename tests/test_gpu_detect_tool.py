"""tools/det/detect_codet.py: the evaluation entry point's run with the detection tail on the GPU after every frame."""
import ast
import os
import re
import subprocess
import sys

import pytest

from tests.conftest import ROOT

pytestmark = pytest.mark.gpu


def test_detect_codet_prints_detections_per_frame():
    tool = os.path.join(ROOT, "tools", "det", "detect_codet.py")
    r = subprocess.run([sys.executable, tool, "--com", "disco", "--num_agent", "2", "--frames", "2"], cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = re.findall(r"frame (\d+): .*detections per image (\[[^\]]*\]).*GPU: ([0-9.]+) ms", r.stdout)
    assert [int(f) for f, _, _ in lines] == [0, 1], r.stdout
    for _, counts, ms in lines:
        counts = ast.literal_eval(counts)
        assert len(counts) == 2 and all(1 <= c <= 300 for c in counts), counts
        assert float(ms) > 0
