"""The parameter-free collaboration baselines beside `--com disco`: `--com sum`, `mean` and `max` (upstream
coperception/models/det/{SumFusion,MeanFusion,MaxFusion}.py over FusionBase.forward).

Same backbone, pose warp, neighbour list, heads, losses and tail as DiscoNet; the fusion step is a reduction over the
ego's list [own map, warp(j -> i) for the live j != i ascending] instead of the attention block:

    sum   fp32 adds in list order            mean  that sum / len(list)            max  elementwise, torch.max(dim=0)

Inference: one launch, `ops.fuse_reduce` (csrc/fuse_reduce.hip) -- the warped maps are never written.  Training: the
engine keeps its shape (the warps are materialised; `max` needs them in its backward) with dn_fuse_reduce_lists /
_backward in the place of the attention MLP and the softmax combine.  The contract is include/disconet_hip.h ::
dn_fuse_reduce; `host_fuse_reduce` states it in plain torch on the CPU.

The two floors of the comparison live here too: `--com lowerbound` (NoFusion: the identity in place of the reduction, every
agent detects from its own view) and `--com late`, the same detector with postprocess.late_fuse behind its detection tail
(collaboration at the box level, dn_late_fuse).  COM_MODES keeps the four feature-level modes; DET_COM_MODES adds the two.
"""
import torch
import torch.nn.functional as F

from . import ops
from . import train_ops as T
from .model import DiscoNet
from .profiling import region
from .train import TrainEngine

COM_MODES = ("disco", "sum", "mean", "max")
# the modes of the det / track tools: `lowerbound` is the detector without collaboration, `late` that detector with
# postprocess.late_fuse behind its detection tail (collaboration at the box level; trained as `lowerbound`)
DET_COM_MODES = COM_MODES + ("lowerbound", "late")


# ---------------------------------------------------------------------------
# the contract, on the CPU
# ---------------------------------------------------------------------------
def _host_warp(nb, pose):
    """nb [C, h, w] fp32, pose [4, 4]: upstream feature_transformation -- rotate, zero-pad, translate (two bilinear
    resamples, zeros padding, align_corners=False), fp32"""
    x = nb.unsqueeze(0)
    p = pose.to(torch.float32)
    rot = torch.zeros(1, 2, 3)
    rot[0, :, :2] = p[:2, :2]
    tr = torch.zeros(1, 2, 3)
    tr[0, 0, 0] = tr[0, 1, 1] = 1.0
    tr[0, 0, 2] = 4 * p[0, 3] / 128
    tr[0, 1, 2] = -(4 * p[1, 3]) / 128
    size = tuple(x.shape)
    r = F.grid_sample(x, F.affine_grid(rot, size, align_corners=False), mode="bilinear", padding_mode="zeros",
                      align_corners=False)
    return F.grid_sample(r, F.affine_grid(tr, size, align_corners=False), mode="bilinear", padding_mode="zeros",
                         align_corners=False)[0]


def reduce_list(maps, mode):
    """the reduction of one ego's list (tensors of one shape), as the three upstream classes write it"""
    stack = torch.stack(list(maps))
    if mode == "sum":
        return stack.sum(0)
    if mode == "mean":
        return stack.mean(0)
    if mode == "max":
        return torch.max(stack, dim=0)[0]
    raise ValueError("mode must be one of %s (got %r)" % (sorted(ops.FUSE_MODES), mode))


def host_fuse_reduce(feat, trans, num_agent, batch, agents, mode, only_v2i=False, ego_first=0, ego_count=None):
    """ops.fuse_reduce's contract in plain torch on the CPU, fp32: feat [A*B, h, w, C] agent-major NHWC, trans
    [B, A, A, 4, 4], num_agent [B] live counts (clamped to 0..A) -> fused [ego_count*B, h, w, C], image
    (i - ego_first) * B + b.  A padded ego passes through; a dead neighbour is never read."""
    A, B = agents, batch
    E = A if ego_count is None else ego_count
    x = feat.detach().to(device="cpu", dtype=torch.float32).permute(0, 3, 1, 2)      # [A*B, C, h, w]
    trans = trans.detach().to(device="cpu", dtype=torch.float32)
    if x.shape[0] != A * B:
        raise ValueError("feat has %d images, expected agents * batch = %d" % (x.shape[0], A * B))
    if not (0 <= ego_first and E > 0 and ego_first + E <= A):
        raise ValueError("ego range [%d, %d) outside 0..%d" % (ego_first, ego_first + E, A))
    out = torch.empty((E * B,) + tuple(x.shape[1:]), dtype=torch.float32)
    for b in range(B):
        n = max(0, min(int(num_agent[b]), A))
        for i in range(ego_first, ego_first + E):
            ego = x[i * B + b]
            if i >= n:
                out[(i - ego_first) * B + b] = ego
                continue
            maps = [ego] + [_host_warp(x[j * B + b], trans[b, i, j]) for j in range(n)
                            if j != i and not (only_v2i and i != 0 and j != 0)]
            out[(i - ego_first) * B + b] = reduce_list(maps, mode)
    return out.permute(0, 2, 3, 1).contiguous()


# ---------------------------------------------------------------------------
# the models
# ---------------------------------------------------------------------------
class _ReduceFusionNet(DiscoNet):
    """DiscoNet's walk (encode, compression, `layer`, the overlap refusal, decode, heads, the range guard, the kd_flag
    output tuple) with a parameter-free fusion: no pixel_weighted_fusion, so the state_dict is DiscoNet's minus those
    keys (a DiscoNet checkpoint fails torch's strict check), and no attention plan."""

    com = None      # "sum" | "mean" | "max"

    def _create_fusion_params(self):
        pass

    def _fusion_plan(self, math):
        return {}

    def _train_engine_class(self):
        return ReduceTrainEngine

    def fuse(self, feat, trans_matrices, num_agent, batch_size, P, want_weights=False, ego_first=0, ego_count=None,
             sp_out=False):
        """ops.fuse_reduce over the layer-`layer` maps -> fp32 NHWC (sp_out is ignored: the decoder's first conv splits an
        NHWC input itself, _ConvLayer.run)"""
        if want_weights:
            raise ValueError("%s has no agent weights" % type(self).__name__)
        feat = ops.as_nhwc(feat)
        n, h, w, c = feat.shape
        E = self.agent_num if ego_count is None else ego_count
        map_bytes = 4.0 * h * w * c
        with region("fuse_reduce", "fuse_reduce_kernel", 0.0, map_bytes * (n + E * batch_size)):
            return ops.fuse_reduce(feat, trans_matrices, num_agent, batch_size, self.agent_num, self.com, self.only_v2i,
                                   ego_first, E)


class SumFusion(_ReduceFusionNet):
    com = "sum"


class MeanFusion(_ReduceFusionNet):
    com = "mean"


class MaxFusion(_ReduceFusionNet):
    com = "max"


class NoFusion(_ReduceFusionNet):
    """`--com lowerbound`: no collaboration -- the reduction is the identity, every agent detects from its own view.  Also
    the detector of `--com late`, whose collaboration happens behind the detection tail (postprocess.late_fuse)."""
    com = "lowerbound"

    def _train_engine_class(self):
        return NoFusionTrainEngine

    def fuse(self, feat, trans_matrices, num_agent, batch_size, P, want_weights=False, ego_first=0, ego_count=None,
             sp_out=False):
        """the served egos' own layer-`layer` maps: no launch, and trans_matrices / num_agent are never read"""
        if want_weights:
            raise ValueError("%s has no agent weights" % type(self).__name__)
        E = self.agent_num if ego_count is None else ego_count
        if not (0 <= ego_first and E > 0 and ego_first + E <= self.agent_num):
            raise ValueError("ego range [%d, %d) outside 0..%d" % (ego_first, ego_first + E, self.agent_num))
        if ego_first == 0 and E == self.agent_num:
            return feat                 # (NHWC or SP, as the encoder left it: the decoder takes either)
        return ops.as_nhwc(feat)[ego_first * batch_size:(ego_first + E) * batch_size]


_CLASSES = {"disco": DiscoNet, "sum": SumFusion, "mean": MeanFusion, "max": MaxFusion, "lowerbound": NoFusion,
            "late": NoFusion}


def build_model(com, config, **kw):
    """the detector of `--com com`: DiscoNet for "disco", the baseline's class for sum / mean / max, NoFusion for
    lowerbound and late; same constructor arguments"""
    if com not in _CLASSES:
        raise ValueError("--com must be one of %s (got %r)" % (", ".join(DET_COM_MODES), com))
    return _CLASSES[com](config, **kw)


# ---------------------------------------------------------------------------
# training
# ---------------------------------------------------------------------------
class ReduceTrainEngine(TrainEngine):
    """TrainEngine with the reduction in the place of the attention block: no fusion layers, no per-call BatchNorms;
    everything else (the lifts, the range guard, the fp32 fallback, the checkpoint keys) is the base engine's."""

    _KD_OK = False      # the distillation is DiscoGraph's (CoDetModule refuses kd_flag = 1)

    def __init__(self, model, *args, shard=None, **kw):
        if shard is not None:
            raise NotImplementedError("agent-parallel training of --com %s is not built (the sharded step is --com disco's)"
                                      % model.com)
        super().__init__(model, *args, shard=None, **kw)

    def _fusion_layers(self):
        return {}

    def _fusion_per_call_stats(self):
        return []

    def _fusion_fwd(self, maps, NI, NW, F):
        if NW:
            T.warp_list(maps, F["poses"], F["src_image"], out=maps[NI:])
        fused = torch.empty((F["ego_out"].numel(),) + tuple(maps.shape[1:]), dtype=torch.float32, device=maps.device)
        T.fuse_reduce_lists(maps, F["first"], F["map_image"], F["ego_out"], self.model.com, fused)
        self.fctx = dict(maps=maps, NI=NI, NW=NW, fused=fused)
        return fused

    def _fusion_bwd(self, dfused, G):
        F, c = self.F, self.fctx
        maps, NI, NW = c["maps"], c["NI"], c["NW"]
        dmaps = torch.empty_like(maps)      # every map is in exactly one list: every row is written
        T.fuse_reduce_lists_backward(dfused, maps, c["fused"], F["first"], F["map_image"], F["ego_out"], self.model.com, dmaps)
        if NW:
            T.warp_backward(dmaps[NI:], F["poses"], F["src_image"], dmaps[:NI], rigid=F["rigid"])
        return dmaps[:NI]


class NoFusionTrainEngine(ReduceTrainEngine):
    """`--com lowerbound`: the fused maps are the egos' own rows of the pair buffer and their gradient passes through.  The
    lists are those of a batch without live agents (every ego alone in its list: no warps, no poses gathered)."""

    def _fusion_lists(self, trans, num_agent_cpu, B, dev, poses=True):
        return super()._fusion_lists(trans, torch.zeros_like(num_agent_cpu), B, dev, poses=poses)

    def _fusion_fwd(self, maps, NI, NW, F):
        self.fctx = dict(maps=maps, NI=NI, NW=NW)
        return maps[:NI]

    def _fusion_bwd(self, dfused, G):
        return dfused
