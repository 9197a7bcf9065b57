"""MI355X-native `--com disco` (DiscoNet) collaborative-perception hot path.

Host side (this package) mirrors the reference's Python class surface; all
compute is in libdisconet_hip.so (disconet_amd/csrc, C ABI in
include/disconet_hip.h).  See DESIGN.md.
"""
from .config import Config
from .model import DiscoNet
from .fusion_modes import (ALL_DET_COM_MODES, COM_MODES, DET_COM_MODES, PARAM_COM_MODES, AgentTrainEngine, AgentWeightedFusion,
                           MaxFusion, MeanFusion, NoFusion, SumFusion, build_model)
from .postprocess import StratifiedAP, gt_strata, late_fuse
from .detector import Detector, load_checkpoint
from . import exchange, holistic, lidar, render, targets
from .render import BoxLayer, attention_sheet, host_render_bev, read_png, render_bev, write_png
from .seg import HostMeanIoU, MeanIoU, SegDiscoNet, SegModule
from .holistic import holistic_views
from .teacher import TeacherNet
from .targets import assign_targets
from .train import CoDetModule, TrainEngine

__all__ = ["Config", "DiscoNet", "SumFusion", "MeanFusion", "MaxFusion", "NoFusion", "AgentWeightedFusion", "AgentTrainEngine", "COM_MODES", "DET_COM_MODES", "PARAM_COM_MODES", "ALL_DET_COM_MODES", "build_model", "late_fuse", "Detector", "load_checkpoint", "TeacherNet", "CoDetModule", "TrainEngine", "SegDiscoNet", "SegModule", "MeanIoU", "HostMeanIoU", "targets",
           "assign_targets", "holistic", "holistic_views", "lidar", "render", "BoxLayer", "render_bev", "host_render_bev", "attention_sheet", "write_png",
           "read_png", "StratifiedAP", "gt_strata", "exchange"]
