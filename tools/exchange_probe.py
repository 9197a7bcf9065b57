#!/usr/bin/env python
"""Call times of the feature-exchange kernels and what a wire format adds to the fusion call.

At 5 agents x batch 4 (20 x 32 x 32 x 256 maps, the benchmark's) and 8 agents x batch 4 (32 maps), every agent live, for
every format of disconet_amd.exchange.FORMATS:
  encode   ops.exchange_encode into a standing wire buffer (f32: the identity, no launch, no row)
  decode   ops.exchange_decode of that wire into a standing map
  fuse     DiscoNet.fuse of the eval forward with model.exchange = the format (exchange.roundtrip + warp + the one-launch
           attention kernel); with f32 this is the parent path, and `added_ms` of a format is its fuse minus f32's
each timed eager and as a hipGraph replay, alternating between the forms, with device events around windows of --calls
calls; the median of --windows windows after a warm-up.  These are CALL times (launch overhead and the gaps between the
launches of a form included), not kernel times.  The bytes are computed from the shapes: what each launch must read and
write in HBM if nothing stayed in a cache.  The same run checks the device's wire and decoded floats against the numpy
statement (exchange.host_encode / host_decode), byte for byte.  Prints one JSON line and writes it to
profiles/exchange_probe.json (--out).

    python tools/exchange_probe.py [--windows 7] [--calls 200] [--out profiles/exchange_probe.json]
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
WIRE_FORMATS = tuple(f for f in exchange.FORMATS if f != "f32")


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


def check_against_host(feat, fmt):
    x = feat.cpu().numpy()
    want_wire = exchange.host_encode(x, fmt)
    wire = ops.exchange_encode(feat, fmt)
    got = wire.cpu().numpy()
    ok = same_bits(got.view(np.float16), want_wire.view(np.float16)) if fmt == "f16" else np.array_equal(got, want_wire)
    back = ops.exchange_decode(wire, fmt, H, W, C).cpu().numpy()
    return bool(ok and same_bits(back, exchange.host_decode(want_wire, fmt, H, W, C)))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exchange_probe.json"))
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
        trans = make_trans_matrices(B, A, jitter_seed=0).to(dev)
        na = torch.full((B,), A, dtype=torch.int32, device=dev)
        model = DiscoNet(Config(), num_agent=A).eval().to(dev)
        P = model._get_plan()
        forms, nbytes, equal = {}, {}, {}

        def fuse_as(fmt):
            def run():
                model.exchange = fmt
                return model._fuse_exchanged(feat, trans, na, B, P)
            return run

        forms["fuse/f32"] = fuse_as("f32")
        with torch.no_grad():
            for fmt in WIRE_FORMATS:
                equal[fmt] = check_against_host(feat, fmt)
                if not equal[fmt]:
                    raise SystemExit("the device's %s bytes differ from exchange.host_encode / host_decode" % fmt)
                msg = exchange.message_bytes(fmt, H, W, C)
                wire = torch.empty((n, msg), dtype=torch.uint8, device=dev)
                back = torch.empty_like(feat)
                ops.exchange_encode(feat, fmt, out=wire)
                forms["encode/" + fmt] = lambda fmt=fmt, wire=wire: ops.exchange_encode(feat, fmt, out=wire)
                forms["decode/" + fmt] = lambda fmt=fmt, wire=wire, back=back: ops.exchange_decode(wire, fmt, H, W, C, out=back)
                forms["fuse/" + fmt] = fuse_as(fmt)
                nbytes[fmt] = {"message_bytes_per_agent": msg, "encode_read_mib": mib(n * H * W * C * 4),
                               "encode_written_mib": mib(n * msg), "decode_read_mib": mib(n * msg),
                               "decode_written_mib": mib(n * H * W * C * 4)}
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
        model.exchange = "f32"
        row = {"agents": A, "batch": B, "map": [H, W, C], "images": n, "equals_host_statement": equal,
               "message_bytes_per_agent_f32": exchange.message_bytes("f32", H, W, C), "bytes": nbytes,
               "call_ms_median": {}, "added_ms": {}}
        for (how, k), v in samples.items():
            row["call_ms_median"].setdefault(how, {})[k] = round(statistics.median(v), 4)
        for how, med in row["call_ms_median"].items():
            row["added_ms"][how] = {fmt: round(med["fuse/" + fmt] - med["fuse/f32"], 4) for fmt in WIRE_FORMATS}
        rows.append(row)
    out = {"tool": "tools/exchange_probe.py", "what": "call time (device events around windows of calls), ms; median of the windows; "
           "added_ms = DiscoNet.fuse with the format minus with f32 (the parent path) in the same run",
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
