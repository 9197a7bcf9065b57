#!/usr/bin/env python
"""Call times of the fusion step of `--com sum | mean | max` against what it replaces and against `--com disco`'s.

At 5 agents x batch 4 and 8 agents x batch 4, 32 x 32 x 256 maps, every agent live, for every mode:
  fuse_reduce   ops.fuse_reduce: the warp and the reduction in one launch (csrc/fuse_reduce.hip)
  composition   ops.warp_neighbors, then torch.cat([ego, warped]) and .sum / .mean / .max over the agents on the device
  disco_fuse    DiscoNet.fuse (warp + the one-launch attention kernel), the same for every mode
each timed eager and as a hipGraph replay, alternating between the forms, with device events around windows of --calls
calls; the median of --windows windows after a warm-up.  These are CALL times (launch overhead and the gaps between the
launches of a form included), not kernel times.  The bytes are computed from the shapes: what each form must read and write
in HBM if nothing stayed in a cache.  Prints one JSON line and writes it to profiles/fuse_reduce_probe.json (--out).

    python tools/fuse_reduce_probe.py [--windows 7] [--calls 200] [--out profiles/fuse_reduce_probe.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from disconet_amd import Config, DiscoNet, _lib, ops  # noqa: E402
from disconet_amd.graph import GraphedStep  # noqa: E402
from disconet_amd.synthetic import make_trans_matrices  # noqa: E402

H, W, C = 32, 32, 256
SIZES = ((5, 4), (8, 4))
MODES = ("sum", "mean", "max")


def composition(feat, trans, na, B, A, mode):
    warped = ops.warp_neighbors(feat, trans, na, B, A)                                  # [B, A, A-1, h, w, c]
    ego = feat.view(A, B, H, W, C).transpose(0, 1).unsqueeze(2)                         # [B, A, 1, h, w, c]
    stack = torch.cat([ego, warped], 2)
    if mode == "sum":
        return stack.sum(2)
    if mode == "mean":
        return stack.mean(2)
    return stack.max(2)[0]


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fuse_reduce_probe.json"))
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
        model = DiscoNet(Config(), num_agent=A).eval().to(dev)
        P = model._get_plan()
        n, pairs = A * B, A * B * (A - 1)
        forms = {"disco_fuse": lambda: model.fuse(feat, trans, na, B, P, sp_out=True)}
        for m in MODES:
            forms["fuse_reduce/" + m] = lambda m=m: ops.fuse_reduce(feat, trans, na, B, A, m)
            forms["composition/" + m] = lambda m=m: composition(feat, trans, na, B, A, m)
        with torch.no_grad():
            for m in MODES:      # the two forms compute the same thing
                err = (forms["fuse_reduce/" + m]() - composition(feat, trans, na, B, A, m).transpose(0, 1).reshape(n, H, W, C)).abs().max().item()
                if not err < 1e-4:
                    raise SystemExit("fuse_reduce and the composition disagree (%s, %g)" % (m, err))
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
        row = {"agents": A, "batch": B, "map": [H, W, C], "live": A,
               "bytes_mib": {"fuse_reduce": {"read": mib(n), "written": mib(n)},
                             "composition": {"warp_written": mib(pairs), "cat_read": mib(n + pairs), "cat_written": mib(n + pairs),
                                             "reduce_read": mib(n + pairs), "reduce_written": mib(n), "warp_read": mib(n)},
                             "disco_fuse": {"warp_read": mib(n), "warp_written": mib(pairs), "attention_read": mib(n + pairs),
                                            "attention_written": mib(n)}},
               "call_ms_median": {}}
        for (how, k), v in samples.items():
            row["call_ms_median"].setdefault(how, {})[k] = round(statistics.median(v), 4)
        rows.append(row)
    out = {"tool": "tools/fuse_reduce_probe.py", "what": "call time per fusion step (device events around windows of calls), ms; median of the windows",
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
