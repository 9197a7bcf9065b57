"""Pins tests/fusion_fp64.py (the float64 reference of the fusion block) to the fp32 oracle and the committed
goldens, so that what the GPU tests compare the kernels with is the operation the goldens record.  No GPU."""
import os

import numpy as np
import pytest
import torch

from tests import cases
from tests import fusion_fp64 as f64


def test_warp64_matches_the_oracle_and_the_golden_at_the_unit_poses(golden_dir):
    """the bound (1e-5) is the one tests/test_gpu_fusion.py holds the kernel to at these six poses"""
    from oracle.disconet_ref import feature_transformation
    g = np.load(os.path.join(golden_dir, "warp_unit.npz"))
    feat = cases.warp_feature()
    for name, pose in cases.WARP_POSES.items():
        got = f64.warp64(feat[0], torch.from_numpy(pose))
        assert got.dtype == torch.float64
        want = feature_transformation(0, 0, feat.unsqueeze(0), torch.from_numpy(pose)[None], tuple(feat.shape))
        assert (got.float() - want).abs().max().item() <= 1e-5, name
        assert np.abs(got.float().numpy() - g[name]).max() <= 1e-5, name
    assert f64.warp64(feat[0], torch.from_numpy(cases.WARP_POSES["out_of_frame"])).abs().max().item() == 0.0
    assert (f64.warp64(feat[0], torch.eye(4)) - feat[0].double()).abs().max().item() <= 1e-12


def test_warp_many_is_warp64_per_pose_and_differentiable():
    poses, _ = f64.sweep(12, 16)
    maps = f64.sweep_maps(poses.shape[0], 3, 12, 16).double().requires_grad_(True)
    many = f64.warp_many(maps, poses)
    for k in range(0, poses.shape[0], 17):
        assert torch.equal(many[k], f64.warp64(maps[k], poses[k]))
    many.sum().backward()
    assert maps.grad is not None and torch.isfinite(maps.grad).all()


def test_fuse64_matches_the_oracle_loop_and_the_golden(golden_dir):
    """5 agents x [256, 32, 32]: fuse64 against cases.ref_fuse (the oracle's fp32 loop) and golden/fusion_5x256.npz,
    within the project's 1e-4; the fp32 loop of the helper is the oracle's, bit for bit"""
    g = np.load(os.path.join(golden_dir, "fusion_5x256.npz"))
    ref = cases.ref_model(256, 5)
    feat, trans, na = cases.fusion_inputs()
    want = cases.ref_fuse(ref, feat, trans, na)
    live = [int(na[0, 0])]
    fused, weights = f64.fuse64(f64.mlp_of(ref.pixel_weighted_fusion, 256), feat, trans, live, 5, 1)
    assert fused.dtype == torch.float64 and weights.shape == (1, 5, 5, 32 * 32)
    assert (fused.float() - want).abs().max().item() <= 1e-4
    assert np.abs(fused.float().numpy()[:, ::4, ::2, ::2] - g["fused"]).max() <= 1e-4
    assert (weights.sum(2) - 1).abs().max().item() <= 1e-12
    fused32, weights32 = f64.fuse32(f64.mlp_of(ref.pixel_weighted_fusion, 256, torch.float32), feat, trans, live, 5, 1)
    assert torch.equal(fused32, want)
    assert (weights32.double() - weights).abs().max().item() <= 1e-4


def test_fuse64_skip_rule_and_padded_agents():
    """only_v2i: an ego other than agent 0 sees itself and agent 0 only; agents beyond the live count pass through"""
    torch.manual_seed(0)
    A, B, c, h, w = 4, 2, 8, 8, 8
    from oracle.disconet_ref import PixelWeightedFusionSoftmax
    mlp = PixelWeightedFusionSoftmax(c).double().eval()
    feat = torch.randn(A * B, c, h, w).clamp_(min=0)
    poses, _ = f64.sweep(h, w)
    trans = poses[24:24 + B * A * A].reshape(B, A, A, 4, 4)
    fused, wts = f64.fuse64(mlp, feat, trans, [3, 1], A, B, only_v2i=True)
    assert (wts[0, 0, :3] > 0).all() and (wts[0, 0, 3] == 0).all()          # ego 0: itself + two neighbours
    assert (wts[0, 1, :2] > 0).all() and (wts[0, 1, 2:] == 0).all()         # ego 1: itself + agent 0
    assert (wts[0, 3] == 0).all() and torch.equal(fused[3 * B + 0], feat[3 * B + 0].double())   # padded
    assert torch.equal(wts[1, 0, 0], torch.ones(h * w, dtype=torch.float64))                   # alone: weight one
    assert torch.equal(fused[0 * B + 1], feat[0 * B + 1].double())


def test_unpack_fm_inverts_the_documented_order():
    """built element by element from the text of include/disconet_hip.h :: dn_warp_neighbors_fm"""
    h, w, c = 4, 16, 32
    want = torch.arange(h * w * c, dtype=torch.float32).reshape(h, w, c)
    block = torch.empty(h * w * c)
    for t in range(h * w // 32):
        for ks in range(c // 16):
            for r in range(2):
                for hh in range(2):
                    for j in range(32):
                        for e in range(4):
                            at = ((((t * (c // 16) + ks) * 2 + r) * 64) + 32 * hh + j) * 4 + e
                            block[at] = want.reshape(h * w, c)[32 * t + j, 16 * ks + 8 * hh + 4 * r + e]
    assert torch.equal(f64.unpack_fm(block, h, w, c), want)


@pytest.mark.parametrize("h,w", f64.MAP_SIZES)
def test_sweep_is_seeded_and_mostly_in_frame(h, w):
    poses, rigid = f64.sweep(h, w)
    again, _ = f64.sweep(h, w)
    assert torch.equal(poses, again) and poses.dtype == torch.float32
    n = poses.shape[0]
    assert n == 24 + 2 * len(f64.translations(h, w)) + f64.N_RANDOM
    R = poses[:, :2, :2].double()
    det = R[:, 0, 0] * R[:, 1, 1] - R[:, 0, 1] * R[:, 1, 0]
    assert int((det < 0).sum()) == f64.N_RANDOM // 5 and int((~rigid).sum()) == f64.N_RANDOM // 5
    assert (det[rigid].abs() - 1).abs().max() < 1e-6
    bw, bw_rigid = f64.sweep(h, w, backward=True)
    assert torch.equal(bw[:n], poses) and bw.shape[0] == n + 12 and bool(bw_rigid[n:].all())
    assert ((bw[n:, :2, :2].double().det().abs().sqrt() - 1).abs() > 3e-4).all()
    out = f64.warp_many(f64.sweep_maps(1, 2, h, w).expand(n, -1, -1, -1), poses)
    assert float((out.abs().amax((1, 2, 3)) > 0).float().mean()) >= 0.9
