#!/usr/bin/env python
"""Call times of the selective-exchange kernels and what a cell budget adds to the fusion call.

At 20 and 32 images x 32 x 32 x 256 (5 and 8 agents x batch 4, the exchanged level-3 map of the benchmark), for a capacity of
K = P/2, P/4, P/8, P/16 cells in every format of disconet_amd.exchange.FORMATS ("f32" included):
  encode   ops.exchange_encode_cells into a standing wire buffer (score + select + pack: three launches)
  decode   ops.exchange_decode_cells of that wire into a standing map (one launch)
  fuse     DiscoNet.fuse of the eval forward with model.exchange = the format and model.exchange_cells = K
           (exchange.roundtrip(cells=K) + the frame counter + warp + the one-launch attention), eager and as a graph replay
next to `fuse/f32/0`, the same call with every cell sent as fp32: the path of the parent commit, nothing new launched.
Device events around windows of calls, the forms alternating, the median of the windows after a warm-up window.  CALL
times (launch overhead, torch.empty and the gaps between launches included), not kernel times.  The bytes are computed
from the shapes.  Before anything is timed the device's wire and decoded map are compared with the host statement
(exchange.host_encode_cells / host_decode_cells), byte for byte.  Prints one JSON line and writes it to
profiles/exchange_cells_probe.json (--out).

    python tools/exchange_cells_probe.py [--windows 7] [--calls 200] [--out profiles/exchange_cells_probe.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from disconet_amd import Config, DiscoNet, _lib, exchange, ops  # noqa: E402
from disconet_amd.graph import GraphedStep  # noqa: E402
from disconet_amd.synthetic import make_trans_matrices  # noqa: E402

H, W, C = 32, 32, 256
SIZES = ((5, 4), (8, 4))
CAPACITIES = tuple(H * W // d for d in (2, 4, 8, 16))
EMPTY = 0.7                      # the share of all-zero cells of the probe's maps


def window_ms(fn, calls):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / calls


def same_bits(got, want):
    """equal in every bit, NaN positions compared as positions (the contract fixes no NaN payload)"""
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.uint8), want[~nan].view(np.uint8))


def check_against_host(feat, fmt, cells):
    x = feat.cpu().numpy()
    want_wire = exchange.host_encode_cells(x, fmt, cells)
    wire = ops.exchange_encode_cells(feat, fmt, cells)
    got = wire.cpu().numpy()
    at = 16 + (2 * cells + 15) // 16 * 16
    ok = np.array_equal(got[:, :at], want_wire[:, :at])
    if fmt == "f16":
        ok = ok and same_bits(got[:, at:].copy().view(np.float16), want_wire[:, at:].copy().view(np.float16))
    else:
        ok = ok and np.array_equal(got[:, at:], want_wire[:, at:])
    back = ops.exchange_decode_cells(wire, fmt, H, W, C, cells).cpu().numpy()
    return bool(ok and same_bits(back, exchange.host_decode_cells(want_wire, fmt, H, W, C, cells)))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exchange_cells_probe.json"))
    args = ap.parse_args(argv)
    if args.windows < 5:
        raise SystemExit("--windows must be at least 5 (the median of fewer windows is not reported)")
    dev = torch.device("cuda:0")
    mib = lambda nbytes: round(nbytes / 2.0 ** 20, 2)
    rows = []
    for A, B in SIZES:
        torch.manual_seed(0)
        n = A * B
        feat = torch.randn(n, H, W, C, device=dev).clamp_(min=0)
        feat[torch.rand(n, H, W, device=dev) < EMPTY] = 0                 # post-ReLU maps over mostly empty ground
        nonzero = exchange.host_scores(feat.cpu().numpy()) > 0
        trans = make_trans_matrices(B, A, jitter_seed=0).to(dev)
        na = torch.full((B,), A, dtype=torch.int32, device=dev)
        model = DiscoNet(Config(), num_agent=A).eval().to(dev)
        P = model._get_plan()
        eager_only, both, nbytes, equal, sent = {}, {}, {}, {}, {}

        def fuse_as(fmt, cells):
            def run():
                model.exchange, model.exchange_cells = fmt, cells
                return model._fuse_exchanged(feat, trans, na, B, P)
            return run

        both["fuse/f32/0"] = fuse_as("f32", 0)
        with torch.no_grad():
            for cells in CAPACITIES:
                count = exchange.host_select(feat.cpu().numpy(), cells)[1]
                sent[str(cells)] = round(float(count.mean()), 2)
                for fmt in exchange.FORMATS:
                    key = "%s/%d" % (fmt, cells)
                    equal[key] = check_against_host(feat, fmt, cells)
                    if not equal[key]:
                        raise SystemExit("the device's %s bytes at %d cells differ from exchange.host_encode_cells / "
                                         "host_decode_cells" % (fmt, cells))
                    msg = exchange.cells_message_bytes(fmt, H, W, C, cells)
                    wire = torch.empty((n, msg), dtype=torch.uint8, device=dev)
                    back = torch.empty_like(feat)
                    ops.exchange_encode_cells(feat, fmt, cells, out=wire)
                    eager_only["encode/" + key] = lambda fmt=fmt, cells=cells, wire=wire: ops.exchange_encode_cells(feat, fmt, cells, out=wire)
                    eager_only["decode/" + key] = lambda fmt=fmt, cells=cells, wire=wire, back=back: ops.exchange_decode_cells(
                        wire, fmt, H, W, C, cells, out=back)
                    both["fuse/" + key] = fuse_as(fmt, cells)
                    nbytes[key] = {"message_bytes_per_agent": msg,
                                   "sent_bytes_per_agent_mean": round(exchange.sent_bytes(fmt, C, float(count.mean())), 1),
                                   "encode_read_mib": mib(n * H * W * C * 4 + n * cells * C * 4),
                                   "encode_written_mib": mib(n * msg + n * H * W * 4), "decode_read_mib": mib(n * msg),
                                   "decode_written_mib": mib(n * H * W * C * 4)}
            graphs = {k: GraphedStep(fn, range_guard=False) for k, fn in both.items()}
            timed = {("eager", k): fn for k, fn in eager_only.items()}
            for k in both:
                timed[("eager", k)] = both[k]
                timed[("graph", k)] = graphs[k]
            for fn in timed.values():      # warm-up: allocator, clocks
                window_ms(fn, args.calls)
            samples = {k: [] for k in timed}
            for _ in range(args.windows):  # alternating: one window of every form per round
                for k, fn in timed.items():
                    samples[k].append(window_ms(fn, args.calls))
        torch.cuda.synchronize()
        model.exchange, model.exchange_cells = "f32", 0
        row = {"agents": A, "batch": B, "map": [H, W, C], "images": n, "cells_of_a_map": H * W,
               "non_zero_cells_per_image_mean": round(float(nonzero.sum(axis=1).mean()), 2),
               "cells_sent_per_image_mean": sent, "equals_host_statement": equal,
               "message_bytes_per_agent_f32_all_cells": exchange.message_bytes("f32", H, W, C), "bytes": nbytes,
               "call_ms_median": {}, "added_ms": {}}
        for (how, k), v in samples.items():
            row["call_ms_median"].setdefault(how, {})[k] = round(statistics.median(v), 4)
        for how, med in row["call_ms_median"].items():
            row["added_ms"][how] = {k[len("fuse/"):]: round(v - med["fuse/f32/0"], 4) for k, v in med.items()
                                    if k.startswith("fuse/") and k != "fuse/f32/0"}
        rows.append(row)
    out = {"tool": "tools/exchange_cells_probe.py", "what": "call time (device events around windows of calls), ms; median of the "
           "windows; keys are form/format/cells; added_ms = DiscoNet.fuse with the format and the cell budget minus fuse/f32/0 (every "
           "cell as fp32: the parent path) in the same run", "windows": args.windows, "calls_per_window": args.calls,
           "empty_cell_share_of_the_maps": EMPTY, "dn_version": _lib.load().dn_version(), "device": torch.cuda.get_device_name(0),
           "range_flags": ops.sp_range_flags(), "sizes": rows}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
