"""The detector of a `--com` mode with its tail: what the det and track tools run per frame.

    model (fusion_modes.build_model) -> the heads' dict -> postprocess.detect -> for `--com late` postprocess.late_fuse

`--com late` is the lowerbound detector (NoFusion) plus the box-level step behind its tail; that meaning lives here, in
Detector.tail, and nowhere else.  Detector copies nothing, reads nothing back and allocates only what detect() and
late_fuse() allocate themselves, so a call can be captured by graph.GraphedStep.
"""
import torch

from . import exchange as exchange_format
from . import postprocess
from .fusion_modes import build_model
from .synthetic import randomize_bn_stats


def heads(out):
    """the heads' dict {"cls", "loc"} of a forward's output: with kd_flag the model returns a tuple that begins with it"""
    return out[0] if isinstance(out, tuple) else out


def load_checkpoint(model, path):
    """load `path`'s "model_state_dict" into `model`; returns the checkpoint dict (epoch, optimizer state, ...)"""
    checkpoint = torch.load(path, map_location="cpu", weights_only=False)
    model.load_state_dict(checkpoint["model_state_dict"])
    return checkpoint


class Detector:
    def __init__(self, com, config, num_agent, batch_size, *, layer=3, kd_flag=0, compress_level=0, only_v2i=False,
                 pre_nms_top_k=300, iou_thr=0.01, score_thr=None, resume="", seed=0, device="cuda", exchange="f32",
                 exchange_cells=0):
        """com: one of ALL_DET_COM_MODES (build_model raises ValueError otherwise).  Without `resume` the weights are random:
        seeded before construction, so that a run can be reproduced, and the BatchNorm statistics are randomised
        (synthetic.randomize_bn_stats).  `epoch` is the loaded checkpoint's epoch, or None.
        exchange: the wire format of the exchanged map (exchange.FORMATS, model.exchange); anything but "f32" needs
        com = "disco" -- the baselines' one-launch kernels read own and neighbour maps from one tensor, lowerbound and
        late exchange no features.
        exchange_cells: how many cells of the exchanged map an agent sends (model.exchange_cells; 0: every cell), with any
        format; the same rule: anything but 0 needs com = "disco"."""
        if exchange_format.check_format(exchange) != "f32" and com != "disco":
            raise ValueError("exchange = %r needs --com disco (got --com %s): only the DiscoGraph fusion reads the "
                             "neighbours' maps through a tensor of their own" % (exchange, com))
        if exchange_cells and com != "disco":
            raise ValueError("exchange_cells = %r needs --com disco (got --com %s): only the DiscoGraph fusion reads the "
                             "neighbours' maps through a tensor of their own" % (exchange_cells, com))
        self.com, self.config, self.num_agent, self.batch_size = com, config, num_agent, batch_size
        self.only_v2i = bool(only_v2i)
        self.pre_nms_top_k, self.iou_thr, self.score_thr = pre_nms_top_k, iou_thr, score_thr
        torch.manual_seed(seed)
        self.model = build_model(com, config, layer=layer, kd_flag=kd_flag, num_agent=num_agent,
                                 compress_level=compress_level, only_v2i=self.only_v2i)
        self.epoch = None
        if resume:
            self.epoch = load_checkpoint(self.model, resume).get("epoch")
        else:
            randomize_bn_stats(self.model)
        self.model.exchange = exchange
        self.model.exchange_cells = exchange_cells
        self.model.eval().to(device)
        self.model._check_exchange()                # a budget outside [0, P] is refused here, not at the first frame
        self.anchors = postprocess.make_anchors(config, device=device)

    def forward(self, bevs, trans, num_agent_tensor):
        """the heads' dict of the eval-mode forward"""
        with torch.no_grad():
            return heads(self.model(bevs, trans, num_agent_tensor, self.batch_size))

    def tail(self, result, trans, num_agent_tensor):
        """detect()'s dict of the heads' outputs; for `--com late` every agent's boxes merged in each ego's frame,
        duplicates suppressed (late_fuse's dict)"""
        det = postprocess.detect(result, self.anchors, pre_nms_top_k=self.pre_nms_top_k, iou_thr=self.iou_thr,
                                 score_thr=self.score_thr)
        if self.com == "late":
            det = postprocess.late_fuse(det, trans, num_agent_tensor, self.batch_size, self.num_agent, iou_thr=self.iou_thr,
                                        only_v2i=self.only_v2i, extents=self.config.area_extents[:2])
        return det

    def __call__(self, bevs, trans, num_agent_tensor):
        return self.tail(self.forward(bevs, trans, num_agent_tensor), trans, num_agent_tensor)
