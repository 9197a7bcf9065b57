"""Reference twins of the parameter-free fusions `sum` / `mean` / `max` (disconet_amd.fusion_modes), plain torch on the
CPU.  TEST infrastructure: the float64 / fp32 fusion loop built on tests/fusion_fp64.py :: warp_many, the error bounds the
tests derive from it, and a DiscoNetRef whose fusion loop is torch.stack(list).sum / mean / max."""
import torch

from oracle.disconet_ref import LAYER_CHANNEL, DiscoNetRef, feature_transformation
from tests import fusion_fp64 as f64

MODES = ("sum", "mean", "max")
FACTOR = 4.0            # tests/test_gpu_fusion_fp64.py's margin over the fp32 reference's own error, for the same reason


def reduce_stack(maps, mode):
    stack = torch.stack(list(maps))
    if mode == "sum":
        return stack.sum(0)
    if mode == "mean":
        return stack.mean(0)
    assert mode == "max"
    return torch.max(stack, dim=0)[0]


def lists_of(live, agents, batch, only_v2i=False, ego_first=0, ego_count=None):
    """[(b, i, [j, ...])] for every served ego in the contract's order: the neighbours of a live ego ascending, none for
    a padded one"""
    E = agents if ego_count is None else ego_count
    out = []
    for b in range(batch):
        n = max(0, min(int(live[b]), agents))
        for i in range(ego_first, ego_first + E):
            js = [j for j in range(n) if j != i and not (only_v2i and i != 0 and j != 0)] if i < n else []
            out.append((b, i, js))
    return out


class Loop:
    """The fusion loop over feat [A*B, C, h, w] (agent-major) in float64 AND fp32 with one set of warps, for all three
    modes: fused[dtype][mode] [E*B, C, h, w] (image (i - ego_first) * B + b), and what the bounds need --
        E_w     max |fp32 torch warp - float64 warp| over these warps
        nonzero / n_warps    warps that leave a non-zero map
        longest the longest list
        sum_abs max over elements of sum |terms| (float64) over a list
        zero_nb[(b, i)]  every neighbour of the ego is wholly out of frame (float64 and fp32 references both zero)"""

    def __init__(self, feat, trans, live, agents, batch, only_v2i=False, ego_first=0, ego_count=None):
        A, B = agents, batch
        E = A if ego_count is None else ego_count
        x = {torch.float64: feat.double(), torch.float32: feat.float()}
        self.fused = {dt: {m: torch.empty((E * B,) + tuple(feat.shape[1:]), dtype=dt) for m in MODES} for dt in x}
        self.E_w, self.nonzero, self.n_warps, self.longest, self.sum_abs, self.zero_nb = 0.0, 0, 0, 1, 0.0, {}
        for b, i, js in lists_of(live, A, B, only_v2i, ego_first, E):
            out = (i - ego_first) * B + b
            warps = {dt: [f64.warp_many(x[dt][j * B + b][None], trans[b, i, j][None], dt)[0] for j in js] for dt in x}
            all_zero = True
            for w64, w32 in zip(warps[torch.float64], warps[torch.float32]):
                self.E_w = max(self.E_w, (w32.double() - w64).abs().max().item())
                self.n_warps += 1
                self.nonzero += int(w64.abs().max().item() > 0)
                all_zero = all_zero and w64.abs().max().item() == 0 and w32.abs().max().item() == 0
            self.zero_nb[(b, i)] = all_zero
            self.longest = max(self.longest, 1 + len(js))
            terms = [x[torch.float64][i * B + b]] + warps[torch.float64]
            self.sum_abs = max(self.sum_abs, torch.stack(terms).abs().sum(0).max().item())
            for dt in x:
                for m in MODES:
                    self.fused[dt][m][out] = reduce_stack([x[dt][i * B + b]] + warps[dt], m)

    def bound(self, mode):
        return bound(mode, self.E_w, self.longest, self.sum_abs)


def bound(mode, E_w, longest, sum_abs):
    """The bound on |kernel - float64|.  E_w: max |fp32 torch warp - float64 warp| over the test's own warps; every warped
    term may be FACTOR * E_w off (the kernels form coordinates and contract multiply-adds in another order than torch), the
    ego's own term is exact; R = (len - 1) 2^-24 max sum |terms| is the rounding of the len - 1 fp32 adds.
        max: FACTOR E_w        mean: FACTOR E_w + R / len        sum: (len - 1) FACTOR E_w + R"""
    n = longest
    R = (n - 1) * 2.0 ** -24 * sum_abs
    return {"max": FACTOR * E_w, "mean": FACTOR * E_w + R / n, "sum": (n - 1) * FACTOR * E_w + R}[mode]


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


class ReduceRef(DiscoNetRef):
    """DiscoNetRef with the fusion loop of upstream SumFusion / MeanFusion / MaxFusion: torch.stack(list).sum / mean / max
    (no attention block, no pixel_weighted_fusion parameters)"""

    def __init__(self, config, mode, **kw):
        super().__init__(config, **kw)
        del self.pixel_weighted_fusion
        self.mode = mode

    def forward(self, bevs, trans_matrices, num_agent_tensor, batch_size=1):
        bevs = bevs.permute(0, 1, 4, 2, 3)
        encoded = self.u_encoder(bevs)
        feat_maps = encoded[self.layer]
        down = 2 ** self.layer
        size = (1, LAYER_CHANNEL[self.layer], self.map_hw // down, self.map_hw // down)
        local_com_mat = self.build_local_communication_matrix(feat_maps, batch_size)
        updated = [[local_com_mat[b, i] for i in range(self.agent_num)] for b in range(batch_size)]
        for b in range(batch_size):
            num_agent = int(num_agent_tensor[b, 0])
            for i in range(num_agent):
                lst = [local_com_mat[b, i]]
                for j in range(num_agent):
                    if j != i and not (self.only_v2i and i != 0 and j != 0):
                        lst.append(feature_transformation(b, j, local_com_mat, trans_matrices[b, i], size))
                updated[b][i] = reduce_stack(lst, self.mode)
        feat_fuse_mat = torch.cat([torch.stack([updated[b][i] for b in range(batch_size)]) for i in range(self.agent_num)], 0)
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


def build_reduce_ref(mode, map_hw, agents, seed=0, **kw):
    """as oracle.disconet_ref.build_ref_model(init="kaiming"): seeded, activations of O(1), non-trivial BatchNorm statistics"""
    from oracle.disconet_ref import RefConfig, kaiming_reinit, randomize_bn_stats
    torch.manual_seed(seed)
    model = ReduceRef(RefConfig(map_hw), mode, num_agent=agents, **kw)
    kaiming_reinit(model)
    randomize_bn_stats(model)
    return model.eval()
