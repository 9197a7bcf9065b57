"""Segmentation variant of `--com disco` on the MI355X path (BASELINE.json
configs[3]: "DiscoNet seg head, 5-agent, 256x256 BEV").

Surface of upstream:coperception/models/seg/DiscoNet.py :: DiscoNet on SegModelBase (recollection:
the source is not in the mount -- /root/reference/coperception is an empty submodule directory; the
only mounted mention of the task is /root/reference/README.md:15):

    SegDiscoNet(n_channels=13, n_classes=8, num_agent=5, kd_flag=False, compress_level=0, only_v2i=False)
    forward(bevs [A*B, n_channels, H, W] (NCHW, as the reference's SegModule feeds it),
            trans_matrices [B, A, A, 4, 4], num_agent_tensor [B, A])
        -> logits [A*B, n_classes, H, W]      (kd_flag: + x9, x8, x7, x6, x5, fused x4)

a bilinear UNet (DoubleConv / Down / Up / OutConv under the reference's state_dict names) with the
DiscoGraph fusion of the det model at the 512-channel bottleneck.  Parameters live in ordinary
torch modules that are never called; the eval forward packs them once and runs

    3x3 convs (18) + outc     dn_spconv2d on split-planar activations (csrc/conv_sp.hip); the skip
                              concat of the Up blocks is the conv's two-source operand gather
    MaxPool2d(2)              dn_sp_maxpool2          (csrc/seg_ops.hip)
    Upsample x2 bilinear      dn_sp_upsample2_bilinear
    fusion at x4              dn_warp_neighbors + attention MLP + dn_disco_fuse_tail (C = 512)
    cross entropy (SegModule) dn_seg_ce_loss: value + d/d(logits)
    mean IoU (MeanIoU)        dn_seg_confusion: arg-max + per-image confusion counts, on the device behind the forward

There is no torch / CPU fallback.  Training: SegModule.step (seg_train.py: the detector's training engine + the
UNet's max-pool / bilinear-upsample backward kernels).
"""
import numpy as np
import torch
import torch.nn as nn

from . import ops
from .model import ConvRow, _FusionParams, _pack_layers, _PlanModule, attention_mlp_plan, disco_fuse


class _DoubleConv(nn.Module):
    def __init__(self, cin, cout, mid=None):
        super().__init__()
        mid = mid or cout
        self.double_conv = nn.Sequential(nn.Conv2d(cin, mid, 3, padding=1), nn.BatchNorm2d(mid), nn.ReLU(),
                                         nn.Conv2d(mid, cout, 3, padding=1), nn.BatchNorm2d(cout), nn.ReLU())


class _Down(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.maxpool_conv = nn.Sequential(nn.MaxPool2d(2), _DoubleConv(cin, cout))


class _Up(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.up = nn.Upsample(scale_factor=2, mode="bilinear", align_corners=True)
        self.conv = _DoubleConv(cin, cout, cin // 2)


class _OutConv(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, 1)


def unet_layers(m):
    """the UNet's convs in plan order: the two 3x3 convs of each DoubleConv (<block>a, <block>b), then the 1x1 outc"""
    blocks = [("inc", m.inc)]
    for k in (1, 2, 3, 4):
        blocks += [("down%d" % k, getattr(m, "down%d" % k).maxpool_conv[1]), ("up%d" % k, getattr(m, "up%d" % k).conv)]
    for name, dc in blocks:
        seq = dc.double_conv
        yield ConvRow(name + "a", seq[0].weight, seq[0].bias, seq[1], 3, 1, None)
        yield ConvRow(name + "b", seq[3].weight, seq[3].bias, seq[4], 3, 1, None)
    yield ConvRow("outc", m.outc.conv.weight, m.outc.conv.bias, None, 1, 1, None)


class SegDiscoNet(_PlanModule):
    FUSE_CHANNELS = 512

    def __init__(self, n_channels=13, n_classes=8, num_agent=5, kd_flag=False, compress_level=0,
                 only_v2i=False):
        super().__init__()
        if compress_level:
            raise NotImplementedError("seg variant: compress_level > 0 is not built")
        self.n_channels, self.n_classes = n_channels, n_classes
        self.agent_num, self.kd_flag, self.only_v2i = num_agent, kd_flag, only_v2i
        self.inc = _DoubleConv(n_channels, 64)
        self.down1, self.down2, self.down3, self.down4 = _Down(64, 128), _Down(128, 256), _Down(256, 512), _Down(512, 512)
        self.up1, self.up2, self.up3, self.up4 = _Up(1024, 256), _Up(512, 128), _Up(256, 64), _Up(128, 64)
        self.outc = _OutConv(64, n_classes)
        self.pixel_weighted_fusion = _FusionParams(self.FUSE_CHANNELS)

    # train(): SegModule.step / SegTrainStep run the explicit HIP training graph (seg_train.py); the module's own forward()
    # stays the eval plan -- a train()-mode forward() through autograd is not provided.

    # ------------------------------------------------------------------
    def _build_plan(self):
        # every conv on the SP engine; the attention MLP at C = 512 as two 1x1 launches on the NHWC engine + the tail kernel
        P = _pack_layers(unet_layers(self), 2)
        P.update(attention_mlp_plan(self.pixel_weighted_fusion, self.FUSE_CHANNELS, 2, fuse_mlp=False))
        return P

    def fuse(self, x4, trans, num_agent, batch_size, P):
        """DiscoGraph fusion of the bottleneck maps: x4 SpTensor / NHWC [A*B, h, w, 512] -> NHWC"""
        return disco_fuse(x4, trans, num_agent, batch_size, P, self.agent_num, self.only_v2i)

    def forward(self, bevs, trans_matrices, num_agent_tensor, batch_size=None):
        if self.training:
            raise NotImplementedError("SegDiscoNet.forward in train() mode: use SegModule.step (disconet_amd/seg_train.py), "
                                      "the explicit HIP training step; forward() is the eval plan")
        if isinstance(bevs, ops.SpTensor):
            x, dev = bevs, bevs.device
        else:
            if not bevs.is_cuda:
                raise ops._lib.DnError("SegDiscoNet.forward needs GPU tensors; there is no CPU path")
            dev = bevs.device
            # [A*B, C, H, W] -> channels-last rows (a no-copy view when the caller permuted an NHWC
            # voxel batch, as the reference's SegModule does)
            x = bevs.permute(0, 2, 3, 1)
            if x.dtype != torch.float32 or not x.is_contiguous():
                x = x.float().contiguous()
        A = self.agent_num
        n = x.shape[0]
        B = n // A if batch_size is None else batch_size
        if n != A * B:
            raise ValueError("bevs has %d images, expected num_agent*batch_size = %d" % (n, A * B))
        trans = trans_matrices.to(device=dev, dtype=torch.float32).contiguous()
        num_agent = num_agent_tensor[:, 0].to(device=dev, dtype=torch.int32).contiguous()
        P = self._get_plan()

        def double(name, src0, src1=None):
            return P[name + "b"].run(P[name + "a"].run(src0, src1))

        x1 = double("inc", x)
        x2 = double("down1", ops.sp_maxpool2(x1))
        x3 = double("down2", ops.sp_maxpool2(x2))
        x4 = double("down3", ops.sp_maxpool2(x3))
        fused = self.fuse(x4, trans, num_agent, B, P)
        x4f = ops.as_sp(fused)
        x5 = double("down4", ops.sp_maxpool2(x4f))
        # Up: cat([skip, upsampled], channel) -> DoubleConv: the concat is the conv's two-source gather
        x6 = double("up1", x4f, ops.sp_upsample2_bilinear(x5))
        x7 = double("up2", x3, ops.sp_upsample2_bilinear(x6))
        x8 = double("up3", x2, ops.sp_upsample2_bilinear(x7))
        x9 = double("up4", x1, ops.sp_upsample2_bilinear(x8))
        logits = P["outc"].run(x9).nhwc().permute(0, 3, 1, 2)         # NCHW-shaped view of NHWC rows
        if self.kd_flag:
            nchw = lambda t: ops.as_nhwc(t).permute(0, 3, 1, 2)
            return logits, nchw(x9), nchw(x8), nchw(x7), nchw(x6), nchw(x5), nchw(fused)
        return logits


class SegModule:
    """upstream:coperception/utils/SegModule.py :: SegModule, the evaluation half: forward + the
    per-pixel cross entropy on the HIP path (value and gradient w.r.t. the logits)."""

    def __init__(self, model, optimizer=None, lr=1e-3):
        self.model = model
        self._optimizer, self._lr, self._trainer = optimizer, lr, None

    # the training engine behind step() (seg_train.SegTrainEngine; None until the first step built it)
    engine = property(lambda self: self._trainer.engine if self._trainer is not None else None)

    def step(self, data, batch_size=None):
        """upstream SegModule.step: one training step (train-mode forward with batch statistics, cross entropy,
        explicit HIP reverse pass, Adam) -> {"loss": float}.  The training engine is built on first use (its flat
        parameter buffer re-points the module's Parameters: build after the model is on the GPU)."""
        return self.build_engine()._trainer.step(data, batch_size)

    def build_engine(self):
        """build the training engine now (step() does it on first use): a tool that resumes needs `engine` before the first
        step, to load the optimizer state into it.  -> self"""
        if self._trainer is None:
            from .seg_train import SegTrainStep
            self._trainer = SegTrainStep(self.model, self._optimizer, self._lr)
        return self

    def loss(self, logits, labels, want_grad=True):
        """logits [N, classes, H, W] (the model's NCHW-shaped, channels-last view), labels [N, H, W]
        -> (loss float, dlogits NCHW-shaped or None)"""
        z = logits.permute(0, 2, 3, 1)
        if not z.is_contiguous():
            z = z.contiguous()
        loss, grad = ops.seg_ce_loss(z, labels, want_grad)
        return float(loss), (grad.permute(0, 3, 1, 2) if grad is not None else None)

    def evaluate(self, data, batch_size, metric=None):
        """the eval forward + the cross entropy -> {"loss": float, "pred": [A*B, H, W] int64}.  metric: a MeanIoU -- it is
        updated on the device (one dn_seg_confusion launch, no sync) and `pred` comes from that launch; the images whose
        BEV is empty (the padded agent slots: SegTrainStep.step's rule, sum <= 1e-4) are ignored by the metric whatever
        their labels are.  metric=None: exactly the forward, the loss and logits.argmax(1)."""
        with torch.no_grad():
            out = self.model(data["bev_seq"], data["trans_matrices"], data["num_agent"], batch_size)
        logits = out[0] if isinstance(out, tuple) else out
        loss, _ = self.loss(logits, data["labels"], want_grad=False)
        if metric is None:
            return {"loss": loss, "pred": logits.argmax(1)}
        bev = data["bev_seq"]
        bev = bev.nhwc() if isinstance(bev, ops.SpTensor) else bev
        live = bev.reshape(bev.shape[0], -1).sum(1) > 1e-4               # on the device, no sync
        pred = metric.update(logits, data["labels"], live=live, want_pred=True)
        return {"loss": loss, "pred": pred.long()}


# ---------------------------------------------------------------------------
# mean IoU: the seg variant's figure of merit
# ---------------------------------------------------------------------------
# Upstream's tools/seg/test_seg.py keeps this bookkeeping on the host; its source is not available to this project, so what
# it computes is RECALLED, NOT PINNED: the contract is this project's own -- include/disconet_seg.h (dn_seg_confusion) for the
# counts, miou_figures for the arithmetic, HostMeanIoU the numpy statement that the device equals bit for bit.
def host_argmax(rows):
    """the prediction rule of dn_seg_confusion on float32 rows [P, classes] (numpy): the index of the first NaN if the row
    has one, else the index of the first maximum (-0.0 == +0.0; all -inf -> 0) -> [P] int32.  (== torch.argmax / numpy.argmax)"""
    z = np.asarray(rows, dtype=np.float32)
    nan = np.isnan(z)
    top = np.where(nan, -np.inf, z).max(1)
    first_max = (z == top[:, None]).argmax(1)               # argmax of booleans: the first True
    return np.where(nan.any(1), nan.argmax(1), first_max).astype(np.int32)


def miou_figures(confusion, ignored, ignore_classes=()):
    """One confusion matrix [classes, classes] int64 (rows = label, columns = prediction) -> {"confusion", "iou" [classes]
    float64 = TP / (TP + FP + FN), NaN for a class absent from both labels and predictions, "mIoU" = the mean over the
    non-NaN classes not in ignore_classes (NaN if there is none), "accuracy" = trace / total over ALL classes (NaN without a
    live pixel), "ignored": int}.  The sums are integers; every figure is one float64 division, the mean adds in class order."""
    conf = np.asarray(confusion, dtype=np.int64)
    classes = conf.shape[0]
    tp = np.diagonal(conf)
    union = conf.sum(1) + conf.sum(0) - tp                  # TP + FN  +  TP + FP  -  TP
    iou = np.full(classes, np.nan, dtype=np.float64)
    total, count = 0.0, 0
    for c in range(classes):
        if union[c] > 0:
            iou[c] = float(tp[c]) / float(union[c])
            if c not in ignore_classes:
                total += iou[c]
                count += 1
    pixels = int(conf.sum())
    return {"confusion": conf, "iou": iou, "mIoU": total / count if count else float("nan"),
            "accuracy": float(int(tp.sum())) / float(pixels) if pixels else float("nan"), "ignored": int(ignored)}


def miou_line(name, figures):
    """the tools' line: `<name>: mIoU 0.1234  acc 0.5678  IoU 0.9 0.1 nan ...  ignored N`"""
    return "%s: mIoU %.4f  acc %.4f  IoU %s  ignored %d" % (
        name, figures["mIoU"], figures["accuracy"], " ".join("%.4f" % v for v in figures["iou"]), figures["ignored"])


class _MeanIoUBase:
    """what MeanIoU and HostMeanIoU share: the state's shape and compute()'s arithmetic on its host copy"""

    def __init__(self, n_images, classes=8):
        if not (2 <= int(classes) <= 32) or int(n_images) < 1:
            raise ValueError("MeanIoU: %d images x %d classes (at least 1 image, 2 .. 32 classes)" % (n_images, classes))
        self.n_images, self.classes = int(n_images), int(classes)

    def _rows(self, logits):
        """the model's NCHW-shaped channels-last view [n, classes, H, W] or NHWC [n, H, W, classes] -> NHWC.  A 4-d shape
        with classes in both places is ambiguous and refused unless it is a channels-last view (unit stride at dimension 1
        and not at the last one): hand NHWC rows as [n, pixels, classes] then."""
        c = self.classes
        if logits.ndim < 2 or logits.shape[0] != self.n_images or (logits.shape[-1] != c and (logits.ndim != 4 or logits.shape[1] != c)):
            raise ValueError("MeanIoU: logits %s for %d images x %d classes" % (tuple(logits.shape), self.n_images, c))
        nchw = logits.ndim == 4 and logits.shape[1] == c
        if nchw and logits.shape[-1] == c:
            nchw = self._channel_stride(logits, 1) == 1 and self._channel_stride(logits, 3) != 1
            if not nchw:
                raise ValueError("MeanIoU: logits %s could be NCHW or NHWC at %d classes; pass the model's channels-last "
                                 "view or NHWC rows as [n, pixels, classes]" % (tuple(logits.shape), c))
        if nchw:
            return logits.transpose(0, 2, 3, 1) if isinstance(logits, np.ndarray) else logits.permute(0, 2, 3, 1)
        return logits

    @staticmethod
    def _channel_stride(t, d):
        return t.strides[d] // t.itemsize if isinstance(t, np.ndarray) else t.stride(d)

    def state_host(self):
        raise NotImplementedError

    def compute(self, agents=None, ignore_classes=()):
        """-> {"per_image": [figures] * n_images, "per_agent": [figures] * agents ([] without `agents`; image = agent * B + b),
        "overall": figures}, figures as miou_figures.  Per agent and overall the confusion matrices are summed (integers)
        before the one division: the mIoU of all pixels, not a mean of per-image mIoUs."""
        state = self.state_host()
        c = self.classes
        conf, ignored = state[:, :c * c].reshape(self.n_images, c, c), state[:, c * c]
        ignore_classes = tuple(int(k) for k in ignore_classes)
        out = {"per_image": [miou_figures(conf[i], ignored[i], ignore_classes) for i in range(self.n_images)], "per_agent": []}
        if agents is not None:
            if agents < 1 or self.n_images % agents:
                raise ValueError("MeanIoU.compute: %d images do not split over %d agents" % (self.n_images, agents))
            b = self.n_images // agents
            out["per_agent"] = [miou_figures(conf[a * b:(a + 1) * b].sum(0), ignored[a * b:(a + 1) * b].sum(), ignore_classes)
                                for a in range(agents)]
        out["overall"] = miou_figures(conf.sum(0), ignored.sum(), ignore_classes)
        return out


class MeanIoU(_MeanIoUBase):
    """mean IoU on the GPU: the state [n_images, classes^2 + 1] int64 stays on the device, update() is one dn_seg_confusion
    launch without a sync (capturable behind the forward), compute() copies the state once."""

    def __init__(self, n_images, classes=8, device="cuda"):
        super().__init__(n_images, classes)
        self.state = torch.zeros((self.n_images, self.classes * self.classes + 1), dtype=torch.int64, device=device)

    def reset(self):
        self.state.zero_()

    def update(self, logits, labels, live=None, want_pred=False):
        z = self._rows(logits)
        if z.dtype != torch.float32 or z.stride(-1) != 1:
            z = z.float().contiguous()
        return ops.seg_confusion(z, labels, self.state, live, want_pred)

    def state_host(self):
        return self.state.cpu().numpy()


class HostMeanIoU(_MeanIoUBase):
    """The numpy statement of dn_seg_confusion + MeanIoU with the same interface (numpy arrays or CPU tensors in): the
    reference of the bit-for-bit tests.  Written for its bits, not for speed."""

    def __init__(self, n_images, classes=8, device=None):
        super().__init__(n_images, classes)
        self.state = np.zeros((self.n_images, self.classes * self.classes + 1), dtype=np.int64)

    def reset(self):
        self.state[:] = 0

    def update(self, logits, labels, live=None, want_pred=False):
        host = lambda t: t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
        c, n = self.classes, self.n_images
        z = self._rows(host(logits))
        y = host(labels)
        if y.dtype.kind not in "iu":
            raise ValueError("HostMeanIoU: labels must be integers (got %s)" % y.dtype)
        y = y.astype(np.int64).reshape(n, -1)
        pred = host_argmax(z.reshape(-1, c)).reshape(n, -1)
        if y.shape != pred.shape:
            raise ValueError("HostMeanIoU: %d labels for %d pixels" % (y.size, pred.size))
        alive = np.ones(n, dtype=bool) if live is None else host(live).reshape(n) != 0
        for img in range(n):
            counted = (y[img] >= 0) & (y[img] < c) if alive[img] else np.zeros(y.shape[1], dtype=bool)
            np.add.at(self.state[img], y[img][counted] * c + pred[img][counted], 1)
            self.state[img, c * c] += int((~counted).sum())
        return pred.reshape(host(labels).shape) if want_pred else None

    def state_host(self):
        return self.state.copy()
