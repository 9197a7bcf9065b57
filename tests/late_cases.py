"""Cases of the late-fusion tests (postprocess.late_fuse / host_late_fuse, `--com late`) and the no-fusion twin of
`--com lowerbound`.  TEST infrastructure, plain numpy / torch on the CPU: padded detection rows of every agent, the poses
of synthetic.make_trans_matrices(jitter_seed=3), rows planted on the contract's edges, and a DiscoNetRef whose fusion loop
leaves every agent's map as it is."""
import numpy as np
import torch

from disconet_amd.synthetic import make_trans_matrices
from oracle.disconet_ref import DiscoNetRef

# (agents, batch, live agents per scene, only_v2i): live counts below A, 0 and equal to A, eight agents, five agents
CONFIGS = [(4, 2, [3, 2], False), (4, 2, [4, 3], True), (8, 1, [8], False), (5, 2, [0, 5], False)]
EXTENTS = ((-32.0, 32.0), (-32.0, 32.0))
KEYS = ("boxes", "scores", "source", "count")


def trans_of(A, B):
    return make_trans_matrices(B, A, jitter_seed=3)


def random_rows(A, B, k_in, seed, counts="ragged", shuffle=True):
    """Random rows of every agent, in no order (`shuffle`), distinct scores in (0, 1): centres uniform over a square whose
    side grows with sqrt(A * k_in), so that a box meets a dozen others at every size and, from 64 rows on, some land
    outside the extents once carried; w in (1.5, 2.5), l in (3, 6), any yaw, a heading vector of any length in (0.5, 2)."""
    rng = np.random.RandomState(seed)
    n = A * B
    half = max(6.0, 1.2 * np.sqrt(A * k_in))
    boxes = np.zeros((n, k_in, 6), dtype=np.float32)
    boxes[..., 0:2] = rng.uniform(-half, half, (n, k_in, 2))
    boxes[..., 2] = rng.uniform(1.5, 2.5, (n, k_in))
    boxes[..., 3] = rng.uniform(3.0, 6.0, (n, k_in))
    yaw = rng.uniform(-np.pi, np.pi, (n, k_in))
    norm = rng.uniform(0.5, 2.0, (n, k_in))
    boxes[..., 4], boxes[..., 5] = norm * np.sin(yaw), norm * np.cos(yaw)
    scores = ((rng.permutation(n * k_in) + 1.0) / (n * k_in + 1.0)).astype(np.float32).reshape(n, k_in)
    if not shuffle:
        scores = -np.sort(-scores, axis=1)
    if counts == "ragged":
        count = rng.randint(max(1, k_in // 2), k_in + 1, n).astype(np.int32)
    else:
        count = np.full(n, k_in, dtype=np.int32)
    return {"boxes": boxes, "scores": scores, "count": count}


def copies(A, B, objects, k_in, seed, trans):
    """`objects` well-separated boxes per scene (a 9 m grid in agent 0's frame, inside +-14 m), every agent holding its own
    copy of each in its own frame (carried there in float64 with trans[b][j][0], rounded to fp32), distinct scores: under
    any pose of the list the copies of one object overlap almost wholly and two objects never meet."""
    rng = np.random.RandomState(seed)
    assert objects <= 16 and objects <= k_in
    det = {"boxes": np.zeros((A * B, k_in, 6), dtype=np.float32), "scores": np.zeros((A * B, k_in), dtype=np.float32),
           "count": np.full(A * B, objects, dtype=np.int32)}
    t64 = trans.numpy().astype(np.float64)
    scores = ((rng.permutation(A * B * objects) + 1.0) / (A * B * objects + 1.0)).reshape(A * B, objects)
    for b in range(B):
        cell = rng.permutation(16)[:objects]
        x = -13.5 + 9.0 * (cell // 4) + rng.uniform(-1.0, 1.0, objects)
        y = -13.5 + 9.0 * (cell % 4) + rng.uniform(-1.0, 1.0, objects)
        yaw = rng.uniform(-np.pi, np.pi, objects)
        for j in range(A):
            M = t64[b, j, 0]
            rows = det["boxes"][j * B + b]
            rows[:objects, 0] = M[0, 0] * x + M[0, 1] * y + M[0, 3]
            rows[:objects, 1] = M[1, 0] * x + M[1, 1] * y + M[1, 3]
            rows[:objects, 2], rows[:objects, 3] = 2.0, 4.5
            rows[:objects, 4] = M[1, 0] * np.cos(yaw) + M[1, 1] * np.sin(yaw)
            rows[:objects, 5] = M[0, 0] * np.cos(yaw) + M[0, 1] * np.sin(yaw)
    det["scores"][:, :objects] = scores
    return det


def plant_score_edges(det, B):
    """The contract's score and count edges, planted into a copy of random rows of k_in >= 8: NaN, -0 (a candidate, equal to
    +0), +0, a negative score, +inf and -inf (no candidates), one score shared by rows of three agents and by two rows of
    one agent, a count below 0 and one above k_in.  Returns the copy."""
    det = {k: v.copy() for k, v in det.items()}
    s, c = det["scores"], det["count"]
    n, k_in = s.shape
    assert k_in >= 8 and n >= 3 * B
    c[:] = k_in
    for img in range(n):
        s[img, 0] = np.float32("nan")
        s[img, 1] = np.float32(-0.0) if img % 2 else np.float32(0.0)
        s[img, 2] = np.float32(0.0) if img % 2 else np.float32(-0.0)
        s[img, 3] = np.float32(-0.25)
        s[img, 4] = np.float32("inf")
        s[img, 5] = np.float32("-inf")
        s[img, 6] = np.float32(0.5)                      # the same score in every agent ...
        s[img, 7] = np.float32(0.5)                      # ... and twice in each
    c[0] = -3                                            # agent 0, scene 0: no rows
    c[n - 1] = k_in + 5                                  # the last agent's last scene: clamped to k_in
    return det


def plant_extent_edge(det, trans, B, ego, nbr, b=0, ulps=(-3, -2, -1, 0, 1, 2, 3)):
    """Rows of neighbour `nbr`, scene b, whose centre lands a few fp32 ulps on either side of ego `ego`'s x_hi edge and of
    its y_lo edge once carried: the row whose float64 image is the edge point, stepped by whole ulps of its own x (y) in
    fp32.  Returns (the copy, the planted rows' indices)."""
    det = {k: v.copy() for k, v in det.items()}
    M = trans[b, ego, nbr].numpy().astype(np.float64)
    R, t = M[:2, :2], M[:2, 3]
    rows = []
    img = nbr * B + b
    r = 0
    for edge in ((EXTENTS[0][1], 3.0), (-7.0, EXTENTS[1][0])):
        p = np.linalg.solve(R, np.asarray(edge) - t).astype(np.float32)      # the edge point in the neighbour's frame
        for axis in (0, 1):
            for u in ulps:
                q = p.copy()
                for _ in range(abs(u)):
                    q[axis] = np.nextafter(q[axis], np.float32(np.inf if u > 0 else -np.inf))
                det["boxes"][img, r, 0:2] = q
                det["boxes"][img, r, 2:4] = (0.3, 0.3)   # small: the planted rows meet nothing
                det["scores"][img, r] = np.float32(0.9 + 0.001 * r)
                rows.append(r)
                r += 1
    det["count"][img] = max(int(det["count"][img]), r)
    return det, rows


def to_device(det, dev):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in det.items()}


def same_bytes(got, want):
    """[names of the outputs whose bytes differ]: device tensors (or numpy) against host_late_fuse's numpy arrays, padding included"""
    bad = []
    for k in KEYS:
        g = got[k].cpu().numpy() if isinstance(got[k], torch.Tensor) else got[k]
        w = want[k]
        if g.shape != w.shape or g.dtype != w.dtype or g.tobytes() != w.tobytes():
            bad.append(k)
    return bad


# ---------------------------------------------------------------------------
# the no-fusion twin of `--com lowerbound`
# ---------------------------------------------------------------------------
class NoFusionRef(DiscoNetRef):
    """DiscoNetRef whose fusion loop leaves local_com_mat as it is: every agent decodes its own layer-`layer` map (no
    attention block, no pixel_weighted_fusion parameters); trans_matrices and num_agent_tensor are never read"""

    def __init__(self, config, **kw):
        super().__init__(config, **kw)
        del self.pixel_weighted_fusion

    def forward(self, bevs, trans_matrices, num_agent_tensor, batch_size=1):
        bevs = bevs.permute(0, 1, 4, 2, 3)
        encoded = self.u_encoder(bevs)
        local_com_mat = self.build_local_communication_matrix(encoded[self.layer], batch_size)
        feat_fuse_mat = self.agents_to_batch(local_com_mat)
        encoded = list(encoded)
        encoded[self.layer] = feat_fuse_mat
        decoded = self.decoder(*encoded, batch_size, kd_flag=self.kd_flag)
        x = decoded[0]
        cls_preds = self.classification(x).permute(0, 2, 3, 1).contiguous()
        cls_preds = cls_preds.view(cls_preds.shape[0], -1, self.category_num)
        loc_preds = self.regression(x).permute(0, 2, 3, 1).contiguous()
        loc_preds = loc_preds.view(-1, loc_preds.size(1), loc_preds.size(2), self.anchor_num_per_loc, self.out_seq_len,
                                   self.box_code_size)
        result = {"loc": loc_preds, "cls": cls_preds}
        if self.kd_flag == 1:
            return (result, *decoded, feat_fuse_mat)
        return result


def build_nofusion_ref(map_hw, agents, seed=0, **kw):
    """as tests/reduce_fusion_ref.py :: build_reduce_ref: seeded, activations of O(1), non-trivial BatchNorm statistics"""
    from oracle.disconet_ref import RefConfig, kaiming_reinit, randomize_bn_stats
    torch.manual_seed(seed)
    model = NoFusionRef(RefConfig(map_hw), num_agent=agents, **kw)
    kaiming_reinit(model)
    randomize_bn_stats(model)
    return model.eval()
