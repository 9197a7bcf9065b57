"""dn_detect's host side without a GPU: the header declares both entry points and the binding has them, every argument
dn_detect refuses is refused before anything is launched (with a dn_last_error message), and detect() refuses what it
cannot run."""
import ctypes
import math
import os
import re

import pytest
import torch

from tests.conftest import ROOT


def _lib():
    from disconet_amd import _lib
    return _lib.load()


def test_header_declares_detect_and_binding_exists():
    from disconet_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "disconet_hip.h")).read(), flags=re.S)
    for name in ("dn_detect_workspace_bytes", "dn_detect"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.SIGNATURES
        assert getattr(_lib.load(), name) is not None
    assert _lib.load().dn_version() >= 135


def _call(top_k=300, iou_thr=0.01, ws_bytes=None, null=None, n=2, apl=4096):
    """dn_detect with fake (never dereferenced) device pointers: every refusal happens before a launch."""
    lib = _lib()
    need = lib.dn_detect_workspace_bytes(n, apl, max(1, min(top_k, 1024)))
    fake = ctypes.c_void_p(0x1000)
    ptrs = {k: (None if k == null else fake) for k in
            ("cls", "loc", "anchors", "boxes", "scores", "index", "count", "ws")}
    rc = lib.dn_detect(ptrs["cls"], ptrs["loc"], ptrs["anchors"], n, apl, top_k, 0, 0.0, iou_thr, ptrs["boxes"],
                       ptrs["scores"], ptrs["index"], ptrs["count"], ptrs["ws"], need if ws_bytes is None else ws_bytes,
                       None)
    return rc, lib.dn_last_error().decode()


@pytest.mark.parametrize("top_k", [0, 1025, -3])
def test_top_k_out_of_range_is_refused(top_k):
    rc, msg = _call(top_k=top_k)
    assert rc != 0 and "top_k" in msg


@pytest.mark.parametrize("thr", [-0.1, math.nan, math.inf])
def test_bad_iou_thr_is_refused(thr):
    rc, msg = _call(iou_thr=thr)
    assert rc != 0 and "iou_thr" in msg


def test_short_workspace_is_refused():
    lib = _lib()
    need = lib.dn_detect_workspace_bytes(2, 4096, 300)
    assert need > 2 * 4096 * 4                 # one key per anchor at least
    rc, msg = _call(ws_bytes=need - 1)
    assert rc != 0 and "workspace" in msg


@pytest.mark.parametrize("which", ["cls", "loc", "anchors", "boxes", "scores", "index", "count", "ws"])
def test_null_pointer_is_refused(which):
    rc, msg = _call(null=which)
    assert rc != 0 and "null" in msg


def test_workspace_query_refuses_what_detect_refuses():
    lib = _lib()
    assert lib.dn_detect_workspace_bytes(2, 4096, 0) == 0
    assert lib.dn_detect_workspace_bytes(2, 4096, 1025) == 0
    assert lib.dn_detect_workspace_bytes(0, 4096, 300) == 0
    assert lib.dn_detect_workspace_bytes(20, 393216, 300) >= 20 * 393216 * 4


def test_detect_refuses_cpu_tensors_and_large_top_k():
    from disconet_amd import _lib as L
    from disconet_amd import postprocess
    result = {"cls": torch.zeros(1, 64, 2), "loc": torch.zeros(1, 64, 6)}
    anchors = torch.zeros(64, 6)
    with pytest.raises(L.DnError):
        postprocess.detect(result, anchors)
    with pytest.raises(ValueError):
        postprocess.detect(result, anchors, pre_nms_top_k=1025)
    with pytest.raises(ValueError):
        postprocess.detect(result, anchors, pre_nms_top_k=0)
