#!/usr/bin/env python
"""Time of the lattice head's act() tail: ops.lattice_act (torch.rand + one cn_lattice_act launch) against its torch
restatement (torch.rand + ops.lattice_act_torch: ~20 launches) on the same logits, per call, HIP events around
--iters calls, the two alternating over --rounds rounds (median reported, every round listed). One JSON line.
Needs a GPU.

Usage: python tools/lattice_act_time.py [--rows 4096] [--iters 2000] [--rounds 5] [--json FILE]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from crowdnav_dsrnn_amd import ops  # noqa: E402

DEV = "cuda:0"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lattice_act_time: needs a GPU")
    torch.manual_seed(0)
    E = args.rows
    logits = 2.0 * torch.randn((E, ops.LATTICE), device=DEV)

    def kernel():
        return ops.lattice_act(logits, False)

    def restated():
        u = torch.rand((E,), dtype=torch.float32, device=DEV)
        return ops.lattice_act_torch(logits, u)[:2]

    def timed(fn):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for _ in range(args.iters):
            fn()
        ev[1].record()
        ev[1].synchronize()
        return ev[0].elapsed_time(ev[1]) * 1e3 / args.iters   # us per call

    with torch.no_grad():
        for fn in (kernel, restated):   # warm-up: code objects, allocator
            for _ in range(50):
                fn()
        torch.cuda.synchronize()
        rounds = [(timed(kernel), timed(restated)) for _ in range(args.rounds)]
    row = {"rows": E, "iters": args.iters,
           "cn_lattice_act_us": round(statistics.median(r[0] for r in rounds), 3),
           "torch_restatement_us": round(statistics.median(r[1] for r in rounds), 3),
           "rounds_us": [[round(a, 3), round(b, 3)] for a, b in rounds], "device": torch.cuda.get_device_name(0)}
    line = json.dumps(row)
    print(line, flush=True)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
