"""The seg variant's two-command loop: tools/seg/train_seg.py --labels scene writes checkpoints with the det tool's keys and
resumes from them, tools/seg/eval_seg.py --resume (test_seg.py's run on the labelled scenes) scores the checkpoint with
mean IoU on the GPU and prints one parseable line per agent and one overall.  No quality threshold: what mIoU four steps
reach is unmeasured."""
import math
import os
import re
import subprocess
import sys

import pytest

from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

LINE = re.compile(r"^(agent \d+|overall): mIoU (\S+)  acc (\S+)  IoU ((?:\S+ ){7}\S+)  ignored (\d+)$", re.M)


def _run(tool, *argv):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "seg", tool)] + list(argv), cwd=ROOT, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def test_train_seg_checkpoints_resume_and_eval_seg_scores_them(tmp_path):
    import torch
    logs = str(tmp_path / "seg")
    train = ["--labels", "scene", "--num_agent", "2", "--batch", "1", "--nepoch", "2", "--steps_per_epoch", "2"]
    out = _run("train_seg.py", *train, "--logpath", logs)
    epochs = re.findall(r"^epoch (\d+): mean loss (\S+)", out, re.M)
    assert [int(e) for e, _ in epochs] == [1, 2] and all(math.isfinite(float(v)) for _, v in epochs), out
    ck = torch.load(os.path.join(logs, "epoch_2.pth"), map_location="cpu", weights_only=False)
    assert set(ck) == {"epoch", "model_state_dict", "optimizer_state_dict", "scheduler_state_dict", "loss"}      # the det tool's keys
    assert ck["epoch"] == 2 and ck["optimizer_state_dict"]["step"] == 4 and "outc.conv.weight" in ck["model_state_dict"]

    out = _run("train_seg.py", *train[:6], "--nepoch", "1", "--steps_per_epoch", "1", "--logpath", logs,
               "--resume", os.path.join(logs, "epoch_2.pth"))
    assert "resumed" in out and re.findall(r"^epoch (\d+):", out, re.M) == ["3"], out
    ck3 = torch.load(os.path.join(logs, "epoch_3.pth"), map_location="cpu", weights_only=False)
    assert ck3["epoch"] == 3 and ck3["optimizer_state_dict"]["step"] == 5
    assert not torch.equal(ck3["model_state_dict"]["outc.conv.weight"], ck["model_state_dict"]["outc.conv.weight"])

    out = _run("eval_seg.py", "--labels", "scene", "--num_agent", "2", "--batch", "1", "--frames", "2",
               "--resume", os.path.join(logs, "epoch_2.pth"))
    rows = LINE.findall(out)
    assert [name for name, *_ in rows] == ["agent 0", "agent 1", "overall"], out
    for name, miou, acc, ious, ignored in rows:
        assert 0.0 <= float(miou) <= 1.0 and 0.0 <= float(acc) <= 1.0 and int(ignored) == 0, (name, out)
        per_class = [float(v) for v in ious.split()]
        assert len(per_class) == 8 and all(math.isnan(v) or 0.0 <= v <= 1.0 for v in per_class)
        assert not math.isnan(per_class[0])                                 # the background is in every scene
    assert len(re.findall(r"^frame \d+: .* cross entropy ", out, re.M)) == 2
