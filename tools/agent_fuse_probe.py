#!/usr/bin/env python
"""Call times of the fusion step of `--com agent` against `--com disco`'s and against its composition on the device.

At 5 agents x batch 4 and 8 agents x batch 4, 32 x 32 x 256 maps, every agent live:
  agent_fuse       ops.agent_fuse: the pose warp, the score launch (an epilogue of csrc/fuse_mlp.hip's kernel) and the combine
                   launch (csrc/agent_fuse.hip)
  disco_fuse       DiscoNet.fuse (warp + the one-launch attention kernel) writing the SP form the model's decoder reads;
  disco_fuse_nhwc  the same writing fp32 NHWC rows, as agent_fuse does
  composition      ops.warp_neighbors, then the weight net as torch matmuls over every (ego, map) pair, the scalar, torch's
                   softmax and the weighted sum on the device
each timed eager and as a hipGraph replay, alternating between the forms, with device events around windows of --calls calls;
the median of --windows windows after a warm-up.  These are CALL times (launch overhead and the gaps between the launches of
a form included), not kernel times.  The bytes are computed from the shapes: what each form must read and write in HBM if
nothing stayed in a cache.  Prints one JSON line and writes it to profiles/agent_fuse_probe.json (--out).

    python tools/agent_fuse_probe.py [--windows 7] [--calls 200] [--out profiles/agent_fuse_probe.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from disconet_amd import AgentWeightedFusion, Config, DiscoNet, _lib, ops  # noqa: E402
from disconet_amd.graph import GraphedStep  # noqa: E402
from disconet_amd.synthetic import make_trans_matrices, randomize_bn_stats  # noqa: E402

H, W, C = 32, 32, 256
SIZES = ((5, 4), (8, 4))


def folded(net):
    """the weight net as (W^T, scale, shift) per layer with the eval-mode BatchNorms folded, conv1_4 and conv1_5"""
    layers = []
    for i in (1, 2, 3):
        conv, bn = getattr(net, "conv1_%d" % i), getattr(net, "bn1_%d" % i)
        scale, shift = ops.fold_bn(conv.bias, bn, conv.weight.shape[0])
        layers.append((conv.weight.detach().reshape(conv.weight.shape[0], -1).t().contiguous(), scale, shift))
    return layers, net.conv1_4.weight.detach().reshape(8), net.conv1_4.bias.detach(), \
        net.conv1_5.weight.detach().reshape(H, W), net.conv1_5.bias.detach()


def composition(feat, trans, na, B, A, net):
    layers, w4, b4, w5, b5 = net
    warped = ops.warp_neighbors(feat, trans, na, B, A)                                  # [B, A, A-1, h, w, c]
    ego = feat.view(A, B, H, W, C).transpose(0, 1).unsqueeze(2)                         # [B, A, 1, h, w, c]
    stack = torch.cat([ego, warped], 2)                                                 # the lists: own map first
    x = torch.cat([ego.expand_as(stack), stack], -1)
    for wt, scale, shift in layers:
        x = torch.relu(x @ wt * scale + shift)
    s = torch.relu(x @ w4 + b4)                                                         # [B, A, A, h, w]
    a = torch.relu((s * w5).sum((-1, -2)) + b5)
    wk = torch.softmax(a, -1)
    return (wk[..., None, None, None] * stack).sum(2)


def window_ms(fn, calls):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / calls


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "agent_fuse_probe.json"))
    args = ap.parse_args(argv)
    if args.windows < 5:
        raise SystemExit("--windows must be at least 5 (the median of fewer windows is not reported)")
    dev = torch.device("cuda:0")
    mib = lambda maps: round(maps * H * W * C * 4 / 2.0 ** 20, 1)
    rows = []
    for A, B in SIZES:
        torch.manual_seed(0)
        feat = torch.randn(A * B, H, W, C, device=dev).clamp_(min=0)
        trans = make_trans_matrices(B, A, jitter_seed=0).to(dev)
        na = torch.full((B,), A, dtype=torch.int32, device=dev)
        disco = DiscoNet(Config(), num_agent=A).eval().to(dev)
        agent = AgentWeightedFusion(Config(), num_agent=A)
        randomize_bn_stats(agent)
        with torch.no_grad():      # positive conv1_5 weights and bias: no scalar is clamped, the weights are not uniform
            w5 = agent.agent_weighted_fusion.conv1_5.weight
            w5.copy_((torch.rand_like(w5) + 0.5) * (12.0 / (H * W)))
            agent.agent_weighted_fusion.conv1_5.bias.fill_(0.25)
        agent = agent.eval().to(dev)
        Pd, Pa = disco._get_plan(), agent._get_plan()
        net = folded(agent.agent_weighted_fusion)
        n, pairs = A * B, A * B * (A - 1)
        forms = {"agent_fuse": lambda: agent.fuse(feat, trans, na, B, Pa),
                 "disco_fuse": lambda: disco.fuse(feat, trans, na, B, Pd, sp_out=True),
                 "disco_fuse_nhwc": lambda: disco.fuse(feat, trans, na, B, Pd),
                 "composition": lambda: composition(feat, trans, na, B, A, net)}
        with torch.no_grad():
            got, wk = agent.fuse(feat, trans, na, B, Pa, want_weights=True)
            err = (got - composition(feat, trans, na, B, A, net).transpose(0, 1).reshape(n, H, W, C)).abs().max().item()
            if not err < 1e-4:
                raise SystemExit("agent_fuse and the composition disagree (%g)" % err)
            graphs = {k: GraphedStep(fn, range_guard=False) for k, fn in forms.items()}
            timed = {}
            for k in forms:
                timed[("eager", k)] = forms[k]
                timed[("graph", k)] = graphs[k]
            for fn in timed.values():      # warm-up: allocator, clocks
                window_ms(fn, args.calls)
            samples = {k: [] for k in timed}
            for _ in range(args.windows):  # alternating: one window of every form per round
                for k, fn in timed.items():
                    samples[k].append(window_ms(fn, args.calls))
        torch.cuda.synchronize()
        row = {"agents": A, "batch": B, "map": [H, W, C], "live": A, "max_abs_diff_vs_composition": err,
               "weight_spread": round(float((wk.max(-1)[0] - wk.min(-1)[0]).min()), 4),
               "bytes_mib": {"agent_fuse": {"warp_read": mib(n), "warp_written": mib(pairs), "score_read": mib(n + pairs),
                                            "combine_read": mib(n + pairs), "combine_written": mib(n)},
                             "disco_fuse": {"warp_read": mib(n), "warp_written": mib(pairs), "attention_read": mib(n + pairs),
                                            "attention_written": mib(n)},
                             "composition": {"warp_read": mib(n), "warp_written": mib(pairs), "cat_written": mib(3 * (n + pairs)),
                                             "layer1_read": mib(2 * (n + pairs)), "sum_read": mib(n + pairs),
                                             "sum_written": mib(n)}},
               "call_ms_median": {}}
        for (how, k), v in samples.items():
            row["call_ms_median"].setdefault(how, {})[k] = round(statistics.median(v), 4)
        rows.append(row)
    out = {"tool": "tools/agent_fuse_probe.py", "what": "call time per fusion step (device events around windows of calls), ms; median of the windows",
           "windows": args.windows, "calls_per_window": args.calls, "dn_version": _lib.load().dn_version(),
           "device": torch.cuda.get_device_name(0), "range_flags": ops.sp_range_flags(), "sizes": rows}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
