"""A float64 reference of the DiscoGraph fusion block (pose warp, attention MLP, agent softmax, weighted
sum), plain torch on the CPU, and the pose sweep / map sizes the fusion tests share.  TEST infrastructure:
tests/test_fusion_fp64_cpu.py ties it to the fp32 oracle and the committed goldens, tests/test_gpu_fusion_fp64.py
and tests/test_gpu_train_ops.py compare the HIP kernels with it."""
import copy
import math

import numpy as np
import torch
import torch.nn.functional as F

# map sizes (h, w) of the warp tests: BASELINE's 32x32 first, squares, non-square, a ragged last 8x8 tile in both
# directions, and 17x33 whose h * w is no multiple of 32 (no fragment-major form)
MAP_SIZES = [(32, 32), (16, 16), (64, 64), (20, 28), (12, 16), (8, 40), (17, 33)]
FRAME_M = 64.0       # the warp's frame: x_trans = 4 t / 128 is in grid units of half a frame, so 64 m shift a map out of it


# --- the two-pass warp ------------------------------------------------------------------------
def _thetas(poses, dtype):
    """poses [n, 4, 4] -> (theta_rot, theta_trans) [n, 2, 3]: upstream feature_transformation's two affine maps"""
    p = poses.to(dtype)
    n = p.shape[0]
    rot = torch.zeros(n, 2, 3, dtype=dtype)
    rot[:, :, :2] = p[:, :2, :2]
    tr = torch.zeros(n, 2, 3, dtype=dtype)
    tr[:, 0, 0] = tr[:, 1, 1] = 1.0
    tr[:, 0, 2] = 4 * p[:, 0, 3] / 128
    tr[:, 1, 2] = -(4 * p[:, 1, 3]) / 128
    return rot, tr


def warp_many(maps, poses, dtype=torch.float64):
    """maps [n, C, h, w], poses [n, 4, 4]: map k under pose k -- rotate, zero-pad, translate (two bilinear
    resamples, zeros padding, align_corners=False) in `dtype`.  The pose entries are taken as the exact values of
    the matrix given (an fp32 matrix loses nothing on the way to float64).  Differentiable in `maps`.
    dtype=torch.float32 is the arithmetic of the fp32 oracle, whose distance from float64 sets the tests' bounds."""
    x = maps.to(dtype)
    rot, tr = _thetas(poses, dtype)
    size = tuple(x.shape)
    r = F.grid_sample(x, F.affine_grid(rot, size, align_corners=False), mode="bilinear", padding_mode="zeros",
                      align_corners=False)
    return F.grid_sample(r, F.affine_grid(tr, size, align_corners=False), mode="bilinear", padding_mode="zeros",
                         align_corners=False)


def warp64(nb, pose):
    """nb [C, h, w], pose [4, 4] -> [C, h, w] float64: the two-pass warp of the oracle (upstream
    feature_transformation) with everything in float64; differentiable"""
    return warp_many(nb.unsqueeze(0), torch.as_tensor(pose).unsqueeze(0))[0]


# --- the fusion loop --------------------------------------------------------------------------
def mlp_of(fusion_params, channels, dtype=torch.float64):
    """the oracle's PixelWeightedFusionSoftmax in eval mode and `dtype`, holding the parameters and BatchNorm
    statistics of the product's `pixel_weighted_fusion` (shared by name through the state_dict)"""
    from oracle.disconet_ref import PixelWeightedFusionSoftmax
    mlp = PixelWeightedFusionSoftmax(channels)
    mlp.load_state_dict(copy.deepcopy({k: v.detach().cpu() for k, v in fusion_params.state_dict().items()}))
    return mlp.to(dtype).eval()


def _fuse_loop(mlp, feat, trans, live, agents, batch, only_v2i, warp, dtype):
    A, B = agents, batch
    n, c, h, w = feat.shape
    assert n == A * B
    x = feat.to(dtype)
    fused = x.clone()                                   # padded agents pass through
    weights = torch.zeros(B, A, A, h * w, dtype=dtype)
    with torch.no_grad():
        for b in range(B):
            nb_live = max(0, min(int(live[b]), A))
            for i in range(nb_live):
                ego = x[i * B + b]
                nbrs = [ego]
                for j in range(nb_live):
                    if j == i or (only_v2i and i != 0 and j != 0):
                        continue
                    nbrs.append(warp(x[j * B + b], trans[b, i, j]))
                e = [torch.exp(torch.squeeze(mlp(torch.cat([ego, nb], 0).unsqueeze(0)))) for nb in nbrs]
                ssum = 0
                for ek in e:
                    ssum = ssum + ek
                acc = 0
                for k, (ek, nb) in enumerate(zip(e, nbrs)):
                    wk = ek / ssum
                    weights[b, i, k] = wk.reshape(-1)
                    acc = acc + wk * nb
                fused[i * B + b] = acc
    return fused, weights


def fuse64(mlp64, feat, trans, live, agents, batch, only_v2i=False):
    """The oracle's fusion loop (oracle/disconet_ref.py :: DiscoNetRef.forward) in float64.
    mlp64: mlp_of(...); feat [A*B, C, h, w] agent-major (image j*B + b); trans [B, A, A, 4, 4] fp32; live [B] counts.
    -> (fused [A*B, C, h, w], weights [B, A, A, h*w] in neighbour-list order: slot 0 the ego, then the neighbours
    that were warped in, ascending; unused slots and padded egos zero), both float64."""
    return _fuse_loop(mlp64, feat, trans, live, agents, batch, only_v2i, warp64, torch.float64)


def fuse32(mlp32, feat, trans, live, agents, batch, only_v2i=False):
    """the same loop with the fp32 oracle's own warp (feature_transformation) and an fp32 MLP: what the project set
    out to match, and whose distance from fuse64 bounds the kernels' softmax weights"""
    from oracle.disconet_ref import feature_transformation

    def warp(nb, pose):
        return feature_transformation(0, 0, nb[None, None], pose[None], (1,) + tuple(nb.shape))
    return _fuse_loop(mlp32, feat, trans, live, agents, batch, only_v2i, warp, torch.float32)


# --- the fragment-major order -------------------------------------------------------------------
def unpack_fm(block, h, w, c):
    """Inverse of the fragment-major order of include/disconet_hip.h :: dn_warp_neighbors_fm: a block of h*w*c floats
    laid out [tile t of 32 pixels][k-step ks of 16 channels][half r][lane = 32 hh + j] x 4 floats, holding
    channels 16 ks + 8 hh + 4 r + 0..3 of pixel 32 t + j  ->  [h, w, c]."""
    hw = h * w
    assert hw % 32 == 0 and c % 16 == 0 and block.numel() == hw * c
    v = block.reshape(hw // 32, c // 16, 2, 2, 32, 4)            # t, ks, r, hh, j, e
    return v.permute(0, 4, 1, 3, 2, 5).reshape(h, w, c)          # (t, j) -> pixel; (ks, hh, r, e) -> channel


# --- poses ------------------------------------------------------------------------------------
def pose(yaw, tx, ty, scale=1.0, reflect=False):
    m = np.eye(4, dtype=np.float64)
    c, s = math.cos(yaw) * scale, math.sin(yaw) * scale
    m[0, 0], m[0, 1], m[1, 0], m[1, 1] = c, -s, s, c
    if reflect:
        m[:2, 1] *= -1.0                                         # det = -1
    m[0, 3], m[1, 3] = tx, ty
    return m.astype(np.float32)


def translations(h, w):
    """(tx, ty) in metres: none, whole and half pixels, just inside / on / just outside the frame edge, far"""
    px, py = FRAME_M / w, FRAME_M / h                            # one pixel
    return [(0.0, 0.0), (3 * px, -2 * py), (-px, 5 * py), (2.5 * px, 1.5 * py), (0.5 * px, -3 * py),
            (31.999, 0.0), (32.0, 0.0), (32.001, 0.0), (0.0, -31.999), (0.0, 32.0), (-32.001, 32.001),
            (63.9, 0.0), (0.0, -63.9), (64.0, 0.0), (0.0, 64.1), (500.0, 500.0), (-500.0, 3.0), (1e4, -1e4)]


N_RANDOM = 200


def sweep(h, w, seed=1234, backward=False):
    """-> (poses [n, 4, 4] fp32, rigid [n] bool).  Rotations every 15 degrees; translations() alone and with yaw 0.3;
    200 random poses (yaw on the whole circle, +-40 m; every fifth a reflection, a tenth each at scale 0.7 and 1.6);
    backward: twelve near-rigid matrices (scale 1 +- 4e-4, inside train.fusion_poses' 1e-3 test) as well.
    rigid: what fusion_poses calls rigid (|R R^T - 1| < 1e-3, reflections included)."""
    out = [pose(math.radians(15 * k), 0.0, 0.0) for k in range(24)]
    for yaw in (0.0, 0.3):
        out += [pose(yaw, tx, ty) for tx, ty in translations(h, w)]
    rng = np.random.RandomState(seed)
    for k in range(N_RANDOM):
        yaw, tx, ty = rng.uniform(0, 2 * math.pi), rng.uniform(-40, 40), rng.uniform(-40, 40)
        scale = {3: 0.7, 7: 1.6}.get(k % 10, 1.0)
        out.append(pose(yaw, tx, ty, scale, reflect=k % 5 == 0))
    if backward:
        for k in range(12):
            yaw, tx, ty = rng.uniform(0, 2 * math.pi), rng.uniform(-20, 20), rng.uniform(-20, 20)
            out.append(pose(yaw, tx, ty, 1.0 + (4e-4 if k % 2 else -4e-4), reflect=k % 4 == 3))
    poses = torch.from_numpy(np.stack(out))
    R = poses[:, :2, :2].double()
    rigid = (R @ R.transpose(1, 2) - torch.eye(2, dtype=torch.float64)).abs().amax((1, 2)) < 1e-3
    return poses, rigid


def sweep_maps(n_images, c, h, w, seed=77):
    """signed randn maps [n_images, c, h, w] (a ReLU-clamped map hides sign errors of the warp)"""
    g = torch.Generator().manual_seed(seed * 1000 + h * 64 + w)
    return torch.randn(n_images, c, h, w, generator=g)
