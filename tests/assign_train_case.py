"""The fixed training case of tests/test_gpu_assign.py::test_training_moves_the_metric and its float64 oracle twin.  TEST
infrastructure.  `python -m tests.assign_train_case` runs the twin on the CPU (a few minutes) and prints the figures that
the test's floor is derived from."""
import copy

import numpy as np
import torch

HW, AGENTS, BATCH, SEED, BOXES = 128, 2, 1, 3, 16
STEPS, LR = 120, 1e-3
TOP_K, NMS_IOU = 300, 0.01


def scene(device=None):
    from disconet_amd.synthetic import make_box_scene_batch
    return make_box_scene_batch(BATCH, AGENTS, HW, seed=SEED, boxes_per_scene=BOXES, device=device)


def ref_model():
    from tests import cases
    return cases.ref_model(HW, AGENTS, kd_flag=0, init="torch")


def oracle_ap(ref, s, anchors):
    """AP@0.5 / AP@0.7 of the oracle model in eval() mode on the scene, through the oracle's own tail"""
    from oracle import postprocess_ref as R
    ref.eval()
    with torch.no_grad():
        out = ref(s["bev_seq"], s["trans_matrices"], s["num_agent"], BATCH)
    res = out[0] if isinstance(out, tuple) else out
    cls, loc = res["cls"].double().numpy(), res["loc"].double().numpy()
    n = cls.shape[0]
    dets, scs, gts = [], [], []
    for i in range(n):
        b, sc = R.detections_from_logits(cls[i], loc[i].reshape(-1, 6), anchors.reshape(-1, 6), pre_nms_top_k=TOP_K,
                                         iou_thr=NMS_IOU)
        dets.append(b)
        scs.append(sc)
        gts.append(s["gt_boxes"][i, :int(s["gt_count"][i])].numpy())
    return [R.average_precision(dets, scs, gts, t) for t in (0.5, 0.7)]


def oracle_run(steps=STEPS, verbose=True):
    """float64 twin: the oracle model (same initial weights), torch.optim.Adam, oracle/train_ref.py losses, the targets of
    targets.host_assign_targets on the same scene -> (losses per step, [AP@0.5, AP@0.7] untrained, the same trained)"""
    import torch.nn.functional as F
    from disconet_amd import Config, postprocess as P, targets as T
    from oracle.train_ref import train_step
    s = scene()
    anchors = P.make_anchors(Config(map_hw=HW), device="cpu")
    t = T.host_assign_targets(anchors, s["gt_boxes"], s["gt_count"])
    labels = torch.from_numpy(t["labels"])
    reg = torch.from_numpy(t["reg_targets"]).reshape(AGENTS * BATCH, HW, HW, 6, 1, 6)
    mask = torch.from_numpy(t["reg_loss_mask"]).reshape(AGENTS * BATCH, HW, HW, 6, 1)
    ref = copy.deepcopy(ref_model()).double()
    ref.u_encoder.conv_pre_1.register_forward_pre_hook(lambda m, inp: (inp[0].double(),))
    orig = F.grid_sample
    F.grid_sample = lambda inp, grid, **kw: orig(inp, grid.to(inp.dtype), **kw)
    try:
        a64 = anchors.double().numpy()
        before = oracle_ap(ref, s, a64)
        opt = torch.optim.Adam(ref.parameters(), lr=LR)
        losses = []
        for it in range(steps):
            l_cls, l_loc = train_step(ref, opt, s["bev_seq"], s["trans_matrices"], s["num_agent"], BATCH, labels, reg, mask)
            losses.append(l_cls + l_loc)
            if verbose:
                print("oracle step %d: loss %.6f (cls %.6f loc %.6f)" % (it, losses[-1], l_cls, l_loc), flush=True)
                if (it + 1) % 40 == 0 and it + 1 < steps:
                    print("  after %d steps: AP@0.5 / AP@0.7 %s" % (it + 1, oracle_ap(ref, s, a64)), flush=True)
        after = oracle_ap(ref, s, a64)
    finally:
        F.grid_sample = orig
    return losses, before, after


if __name__ == "__main__":
    import time
    t0 = time.time()
    losses, before, after = oracle_run()
    print("%d steps at lr %g" % (STEPS, LR))
    print("oracle float64: mean loss first five %.6f, last five %.6f" % (np.mean(losses[:5]), np.mean(losses[-5:])))
    print("oracle float64: AP@0.5 / AP@0.7 untrained %.4f / %.4f, trained %.4f / %.4f  (%.0f s)" % (
        before[0], before[1], after[0], after[1], time.time() - t0))
