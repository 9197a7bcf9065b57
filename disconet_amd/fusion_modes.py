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

`--com agent` (upstream AgentWiseWeightedFusion) is the first baseline with parameters of its own: a weight net with the four
1x1 layers of DiscoGraph's attention MLP plus conv1_5 = Conv2d(1, 1, (h, w)) gives ONE scalar per entry of the ego's list,
softmax over the list, weighted sum.  Upstream wraps the scalars in torch.tensor(...), which detaches them: the weight net is
never trained (no gradient reaches it, Adam skips it), only its BatchNorm running statistics move.  That is kept here.
Inference: ops.agent_fuse (warp, scores as an epilogue of fuse_mlp.hip's kernel, combine: csrc/agent_fuse.hip); training:
the base engine's MLP forward up to its last logits, then dn_agent_combine_lists / _backward.  The contract is
include/disconet_hip.h :: dn_agent_fuse; `host_agent_fuse` states it in plain torch on the CPU.  PARAM_COM_MODES names the
modes with parameters, ALL_DET_COM_MODES every mode of the det / track tools.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from . import train_ops as T
from .model import LAYER_CHANNEL, DiscoNet, _FusionParams, fuse_mlp_params_of
from .profiling import region
from .train import TrainEngine

COM_MODES = ("disco", "sum", "mean", "max")
# the modes of the det / track tools: `lowerbound` is the detector without collaboration, `late` that detector with
# postprocess.late_fuse behind its detection tail (collaboration at the box level; trained as `lowerbound`)
DET_COM_MODES = COM_MODES + ("lowerbound", "late")
# the collaboration strategies with parameters of their own, and every mode the det / track tools take
PARAM_COM_MODES = ("agent",)
ALL_DET_COM_MODES = DET_COM_MODES + PARAM_COM_MODES


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


def _host_fuse_walk(feat, trans, num_agent, batch, agents, only_v2i, ego_first, ego_count, fuse_list):
    """The walk the host contracts share: feat [A*B, h, w, C] agent-major NHWC, trans [B, A, A, 4, 4], num_agent [B] live
    counts (clamped to 0..A) -> fused [ego_count*B, h, w, C], image (i - ego_first) * B + b, fp32 on the CPU.  A padded ego
    passes through; a dead neighbour is never read; a live ego's image is fuse_list(b, i - ego_first, maps), maps = its own
    [C, h, w] map, then warp(j -> i) of the listed j (ops.ego_list)."""
    A, B = agents, batch
    E = A if ego_count is None else ego_count
    x = feat.detach().to(device="cpu", dtype=torch.float32).permute(0, 3, 1, 2)      # [A*B, C, h, w]
    trans = trans.detach().to(device="cpu", dtype=torch.float32)
    if x.shape[0] != A * B:
        raise ValueError("feat has %d images, expected agents * batch = %d" % (x.shape[0], A * B))
    if not (0 <= ego_first and E > 0 and ego_first + E <= A):
        raise ValueError("ego range [%d, %d) outside 0..%d" % (ego_first, ego_first + E, A))
    out = torch.empty((E * B,) + tuple(x.shape[1:]), dtype=torch.float32)
    with torch.no_grad():
        for b in range(B):
            n = max(0, min(int(num_agent[b]), A))
            for i in range(ego_first, ego_first + E):
                ego = x[i * B + b]
                if i >= n:
                    out[(i - ego_first) * B + b] = ego
                    continue
                maps = [ego] + [_host_warp(x[j * B + b], trans[b, i, j]) for j in ops.ego_list(i, n, only_v2i)[1:]]
                out[(i - ego_first) * B + b] = fuse_list(b, i - ego_first, maps)
    return out.permute(0, 2, 3, 1).contiguous()


def host_fuse_reduce(feat, trans, num_agent, batch, agents, mode, only_v2i=False, ego_first=0, ego_count=None):
    """ops.fuse_reduce's contract in plain torch on the CPU, fp32 (_host_fuse_walk's shapes): every live ego's list reduced
    by reduce_list."""
    return _host_fuse_walk(feat, trans, num_agent, batch, agents, only_v2i, ego_first, ego_count,
                           lambda b, il, maps: reduce_list(maps, mode))


def _host_scores(net, ego, nb):
    """s [h, w]: the weight net's layers 1-4 on cat[ego, nb] ([C, h, w] each), eval-mode BatchNorm, fp32"""
    x = torch.cat([ego, nb], 0).unsqueeze(0)
    for i in (1, 2, 3):
        conv, bn = getattr(net, "conv1_%d" % i), getattr(net, "bn1_%d" % i)
        x = F.relu(F.batch_norm(F.conv2d(x, conv.weight, conv.bias), bn.running_mean, bn.running_var, bn.weight, bn.bias,
                                False, 0.0, bn.eps))
    return F.relu(F.conv2d(x, net.conv1_4.weight, net.conv1_4.bias))[0, 0]


def agent_scalar(s, w5, b5):
    """a = relu(b5 + sum_p w5[p] s[p]) in the contract's order (include/disconet_hip.h :: dn_agent_fuse), fp32 on the CPU: the
    products rounded, tiles of 32 consecutive pixels (zeros past the end), within a tile the tree l with l + 16, + 8, + 4,
    + 2, + 1, the tiles' sums added one after the other ascending, then + b5 and the ReLU"""
    prod = s.reshape(-1).float() * w5.reshape(-1).float()
    tiles = (prod.numel() + 31) // 32
    v = torch.zeros(tiles * 32, dtype=torch.float32)
    v[:prod.numel()] = prod
    v = v.view(tiles, 32)
    for d in (16, 8, 4, 2, 1):
        v = v[:, :d] + v[:, d:2 * d]
    acc = v[0, 0]
    for t in range(1, tiles):
        acc = acc + v[t, 0]
    return torch.clamp(acc + b5.reshape(()).float(), min=0.0)


def agent_softmax(a):
    """w_k = exp(a_k - max a) / sum exp, the sum taken in list order, fp32; a [L]"""
    e = torch.exp(a - a.max())
    total = e[0]
    for k in range(1, e.numel()):
        total = total + e[k]
    return e / total


def weighted_sum(maps, w):
    """sum_k w_k map_k: the first product, then product by product in list order (each product rounded before its add)"""
    acc = w[0] * maps[0]
    for k in range(1, len(maps)):
        acc = acc + w[k] * maps[k]
    return acc


def host_agent_fuse(feat, trans, num_agent, batch, agents, net, only_v2i=False, ego_first=0, ego_count=None,
                    want_weights=False):
    """ops.agent_fuse's contract in plain torch on the CPU, fp32 (_host_fuse_walk's shapes); net: the weight net
    (agent_weighted_fusion's names, its BatchNorms in eval mode) -> fused (+ weights [B, ego_count, A] in list order)."""
    weights = torch.zeros(batch, agents if ego_count is None else max(ego_count, 0), agents, dtype=torch.float32)

    def fuse_list(b, il, maps):
        a = torch.stack([agent_scalar(_host_scores(net, maps[0], m), net.conv1_5.weight, net.conv1_5.bias) for m in maps])
        w = agent_softmax(a)
        weights[b, il, :len(maps)] = w
        return weighted_sum(maps, w)

    fused = _host_fuse_walk(feat, trans, num_agent, batch, agents, only_v2i, ego_first, ego_count, fuse_list)
    return (fused, weights) if want_weights else fused


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


class _AgentNetParams(_FusionParams):
    """upstream AgentWeightedFusion's parameter names: PixelWeightedFusionSoftmax's four 1x1 layers and conv1_5, whose kernel
    is the exchanged map's own (h, w) -- 32 x 32 at the reference's 256 x 256 input, upstream's state-dict shape"""

    def __init__(self, channel, h, w):
        super().__init__(channel)
        self.conv1_5 = nn.Conv2d(1, 1, kernel_size=(h, w))


class AgentWeightedFusion(DiscoNet):
    """`--com agent`: DiscoNet's walk with one scalar weight per agent of the ego's list (module docstring).  Its parameters
    are `agent_weighted_fusion.*`; it has no pixel_weighted_fusion, so a DiscoNet checkpoint fails torch's strict check."""

    com = "agent"

    def __init__(self, config, layer=3, *args, **kw):
        # (the weight net's last kernel spans the exchanged map: its size is needed before DiscoNet creates the parameters)
        self.__dict__["_fused_hw"] = (int(config.map_dims[0]) >> layer, int(config.map_dims[1]) >> layer)
        super().__init__(config, layer, *args, **kw)

    def _create_fusion_params(self):
        self.agent_weighted_fusion = _AgentNetParams(LAYER_CHANNEL[self.layer], *self._fused_hw)

    def _fusion_plan(self, math):
        """the weight net packed as DiscoNet's one-launch attention (whatever the conv engine's math: the scores are
        dn_disco_fuse_mlp's layers 1-4) and conv1_5 as it is"""
        f, C = self.agent_weighted_fusion, LAYER_CHANNEL[self.layer]
        if not ops.fuse_mlp_supported(C):
            raise ops._lib.DnError("--com agent: the weight net runs on %d-channel maps only where dn_fuse_mlp_supported "
                                   "(64, 128 or 256 channels: layer 1, 2 or 3)" % C)
        P = {}
        P["_fuse_mlp"], P["_fuse_mlp_tensors"] = fuse_mlp_params_of(f, C)
        P["_w5"] = f.conv1_5.weight.detach().float().contiguous()
        P["_b5"] = f.conv1_5.bias.detach().float().contiguous()
        return P

    def _train_engine_class(self):
        return AgentTrainEngine

    def fuse(self, feat, trans_matrices, num_agent, batch_size, P, want_weights=False, ego_first=0, ego_count=None,
             sp_out=False):
        """ops.agent_fuse over the layer-`layer` maps -> fp32 NHWC (+ the scalar weights [B, E, A] in list order with
        want_weights; sp_out is ignored: the decoder's first conv splits an NHWC input itself, _ConvLayer.run)"""
        feat = ops.as_nhwc(feat)
        n, h, w, c = feat.shape
        A, B = self.agent_num, batch_size
        E = A if ego_count is None else ego_count
        map_bytes, pairs = 4.0 * h * w * c, B * E * (A - 1)
        flops = 2.0 * B * E * h * w * (128.0 * c * (2 + (A - 1)) + A * (128 * 32 + 32 * 8 + 8))
        with region("agent_fuse", "agent_combine_kernel", flops, map_bytes * (n + 3 * pairs + 3 * E * B)):
            return ops.agent_fuse(feat, trans_matrices, num_agent, P["_fuse_mlp"], P["_w5"], P["_b5"], B, A, self.only_v2i,
                                  want_weights, ego_first, E)


_CLASSES = {"disco": DiscoNet, "sum": SumFusion, "mean": MeanFusion, "max": MaxFusion, "lowerbound": NoFusion,
            "late": NoFusion, "agent": AgentWeightedFusion}


def build_model(com, config, **kw):
    """the detector of `--com com`: DiscoNet for "disco", the baseline's class for sum / mean / max, NoFusion for
    lowerbound and late, AgentWeightedFusion for agent; same constructor arguments"""
    if com not in _CLASSES:
        raise ValueError("--com must be one of %s, %s (got %r)" % (", ".join(DET_COM_MODES), ", ".join(PARAM_COM_MODES), com))
    return _CLASSES[com](config, **kw)


# ---------------------------------------------------------------------------
# training
# ---------------------------------------------------------------------------
def _refuse_shard(model, shard):
    if shard is not None:
        raise NotImplementedError("agent-parallel training of --com %s is not built (the sharded step is --com disco's)"
                                  % model.com)


class ReduceTrainEngine(TrainEngine):
    """TrainEngine with the reduction in the place of the attention block: no fusion layers, no per-call BatchNorms;
    everything else (the lifts, the range guard, the fp32 fallback, the checkpoint keys) is the base engine's."""

    _KD_OK = False      # the distillation is DiscoGraph's (CoDetModule refuses kd_flag = 1)

    def __init__(self, model, *args, shard=None, **kw):
        _refuse_shard(model, shard)
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


class AgentTrainEngine(TrainEngine):
    """`--com agent`: the base engine's MLP forward on the weight net up to its last logits (the warps, the column-cut layer
    1, per-call BatchNorm statistics, mlp2, mlp3, conv1_4), then dn_agent_combine_lists.  As upstream, whose weights are
    torch.tensor(list of scalars), the weight net is never trained: no gradient enters it and its parameters are not stepped
    at all (they lie behind the trained ones in the flat buffer, and Adam -- weight decay included -- runs over the trained
    prefix).  Its three BatchNorms still move their running statistics once per call of the net."""

    _KD_OK = False      # the distillation is DiscoGraph's (CoDetModule refuses kd_flag = 1)

    def __init__(self, model, *args, shard=None, **kw):
        _refuse_shard(model, shard)
        super().__init__(model, *args, shard=None, **kw)

    def _param_order(self, model):
        frozen = {id(p) for p in model.agent_weighted_fusion.parameters()}
        order = super()._param_order(model)
        trained = [p for p in order if id(p) not in frozen]
        self._n_trained = sum((p.numel() + 3) // 4 * 4 for p in trained)      # (the flat buffer's 16-byte aligned views)
        return trained + [p for p in order if id(p) in frozen]

    def _fusion_net(self):
        return self.model.agent_weighted_fusion

    def _fusion_fwd(self, maps, NI, NW, F):
        c = self._fusion_mlp_fwd(maps, NI, NW, F)
        f = self._fusion_net()
        fused = torch.empty((F["ego_out"].numel(),) + tuple(maps.shape[1:]), dtype=torch.float32, device=maps.device)
        c["weights"] = T.agent_combine_lists(c["z4"], f.conv1_5.weight, f.conv1_5.bias, maps, F["first"], F["pair_index"],
                                             F["map_image"], F["ego_out"], fused)
        self.fctx = c
        return fused

    def _fusion_bwd(self, dfused, G):
        F, c = self.F, self.fctx
        maps, NI, NW = c["maps"], c["NI"], c["NW"]
        dmaps = torch.empty_like(maps)      # every map is in exactly one list: every row is written
        T.agent_combine_lists_backward(dfused, c["weights"], maps, F["first"], F["map_image"], F["ego_out"], dmaps)
        if NW:
            T.warp_backward(dmaps[NI:], F["poses"], F["src_image"], dmaps[:NI], rigid=F["rigid"])
        return dmaps[:NI]

    def optimizer_step(self):
        self.step_count += 1
        n = self._n_trained
        T.adam_step(self.flat_p[:n], self.flat_g[:n], self.flat_m[:n], self.flat_v[:n], self.step_count, self.lr, self.betas,
                    self.eps, self.weight_decay)
        self.model._plan = None          # eval-mode packed weights are stale now
