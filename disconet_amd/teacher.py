"""Distillation teacher on the HIP path.

Surface of upstream:coperception/models/det/TeacherNet.py :: TeacherNet (built by
`train_codet.py --kd_flag 1 --resume_teacher <ckpt>`, /root/reference/README.md:58-59):

    TeacherNet(config)
    forward(bevs [N, 1, H, W, Z]) -> (x_8, x_7, x_6, x_5, x_3, x_2)     NCHW-shaped views

the early-fusion teacher: holistic-view voxels through the MotionNet backbone (encoder +
decoder of one `stpn` module), no communication.  The same conv engine and packed-weight plan
as DiscoNet, minus the fusion block; inference only (the teacher is frozen during KD).
"""
import os

import torch
import torch.nn as nn

from . import ops
from .model import (_DEC_CONVS, _BackboneNet, _ClsHeadParams, _EncoderParams, _RegHeadParams, _bn_name, _conv_math,
                    _pack_layers, backbone_layers)


class _BackboneParams(_EncoderParams):
    """upstream Backbone.py :: STPN_KD parameter names (one module holds encoder and decoder)"""

    def __init__(self, in_channels):
        super().__init__(in_channels, 0)
        for name, cin, cout in _DEC_CONVS:
            setattr(self, name, nn.Conv2d(cin, cout, 3, 1, 1))
            setattr(self, _bn_name(name), nn.BatchNorm2d(cout))


class TeacherNet(_BackboneNet):
    def __init__(self, config, in_channels=13):
        super().__init__()
        self.stpn = _BackboneParams(in_channels)
        self.classification = _ClsHeadParams(config)
        self.regression = _RegHeadParams(config, 1 if config.only_det else config.pred_len)
        self.conv_math = os.environ.get("DISCONET_CONV_MATH", "sp")

    def train(self, mode=True):
        if mode:
            raise NotImplementedError("TeacherNet is the frozen distillation teacher: eval() only")
        return super().train(mode)

    def _plan_key(self):
        return (_conv_math(self.conv_math),)

    def _build_plan(self):
        # the backbone's convs only: dense float voxels in (no stem pair), no fused 1x1 layers, no heads
        return _pack_layers(backbone_layers(self.stpn, self.stpn), ops.MATH_MODES[self.conv_math])

    def forward_nhwc(self, bevs):
        """-> (x8, x7, x6, x5, x3, x2) as dense NHWC tensors (what the KD kernel reads)"""
        if self.training:
            raise NotImplementedError("TeacherNet: eval() only")
        if not bevs.is_cuda:
            raise ops._lib.DnError("TeacherNet.forward needs GPU tensors; there is no CPU path")
        P = self._get_plan()
        enc = self.encode(bevs, P)
        return tuple(ops.as_nhwc(t) for t in self.decode(enc, P) + (enc[3], enc[2]))

    def forward(self, bevs):
        with torch.no_grad():
            return tuple(t.permute(0, 3, 1, 2) for t in self.forward_nhwc(bevs))
