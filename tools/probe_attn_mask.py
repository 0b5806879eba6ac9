"""Diagnostic: per-launch time of the masked spatial attention kernels (cn_spatial_attn_mask_fwd / _bwd) at C4's PPO
minibatch shape (R = 128 x 2,048 rows, N = 10 slots, H = 256) with full masks and with Bernoulli(0.5) masks, next to
cn_spatial_attn_fwd / _bwd and cn_spatial_attn_var_fwd / _bwd (full counts) of a baseline library (--baseline: e.g.
the parent commit's, built with `python -m crowdnav_dsrnn_amd.build --out <lib>` in a checkout of it; default: this
build's own) in the same process. Method of tools/probe_attn_var.py: HIP events around `reps` launches, three
alternating rounds. One JSON row per (round, kernel) on stdout and, with --out, appended to that file."""
import argparse
import ctypes
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from crowdnav_dsrnn_amd import _lib  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--baseline", default=None, help="library whose fixed and _var kernels are the baseline")
    ap.add_argument("--rows", type=int, default=128 * 2048)
    ap.add_argument("--N", type=int, default=10)
    ap.add_argument("--H", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    R, N, H = a.rows, a.N, a.H
    L = _lib.lib()
    base = L
    if a.baseline:
        base = ctypes.CDLL(a.baseline)
        vp, i64 = ctypes.c_void_p, ctypes.c_int64
        base.cn_spatial_attn_fwd.argtypes = [vp, i64, ctypes.c_int, ctypes.c_int, ctypes.c_float] + [vp] * 5
        base.cn_spatial_attn_bwd.argtypes = [vp, i64, ctypes.c_int, ctypes.c_int, ctypes.c_float] + [vp] * 7 + [i64, vp, i64]
        base.cn_spatial_attn_var_fwd.argtypes = [vp, i64, ctypes.c_int, ctypes.c_int] + [vp] * 7
        base.cn_spatial_attn_var_bwd.argtypes = [vp, i64, ctypes.c_int, ctypes.c_int] + [vp] * 9 + [i64, vp, i64]
    dev = "cuda:0"
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    hs = torch.randn((R, N, H), generator=g, device=dev)
    u = torch.randn((R, H), generator=g, device=dev) * 0.05
    c = torch.randn((R,), generator=g, device=dev) * 0.05
    out = torch.empty((R, H), device=dev)
    attn = torch.empty((R, N), device=dev)
    dout = torch.randn((R, H), generator=g, device=dev)
    dattn = torch.randn((R, N), generator=g, device=dev)
    dhs = torch.empty_like(hs)
    due = torch.empty((R, H + 4), device=dev)
    count = torch.full((R,), N, dtype=torch.int32, device=dev)
    ones = torch.ones((R, N), device=dev)
    half = (torch.rand((R, N), generator=g, device=dev) < 0.5).float()
    scale = 1.25
    rs = torch.full((R,), scale, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()  # noqa: E731

    def fixed_fwd():
        assert base.cn_spatial_attn_fwd(st, R, N, H, scale, p(hs), p(u), p(c), p(out), p(attn)) == 0

    def fixed_bwd():
        assert base.cn_spatial_attn_bwd(st, R, N, H, scale, p(hs), p(u), p(attn), p(dout), p(dattn), p(dhs), p(due),
                                        H + 4, p(due) + 4 * H, H + 4) == 0

    def var_fwd():
        assert base.cn_spatial_attn_var_fwd(st, R, N, H, p(count), p(rs), p(hs), p(u), p(c), p(out), p(attn)) == 0

    def var_bwd():
        assert base.cn_spatial_attn_var_bwd(st, R, N, H, p(count), p(rs), p(hs), p(u), p(attn), p(dout), p(dattn),
                                            p(dhs), p(due), H + 4, p(due) + 4 * H, H + 4) == 0

    def masked(mask):
        def fwd():
            _lib.check(L.cn_spatial_attn_mask_fwd(st, R, N, H, p(mask), p(rs), p(hs), p(u), p(c), p(out), p(attn)))

        def bwd():
            _lib.check(L.cn_spatial_attn_mask_bwd(st, R, N, H, p(mask), p(rs), p(hs), p(u), p(attn), p(dout), p(dattn),
                                                  p(dhs), p(due), H + 4, p(due) + 4 * H, H + 4))
        return fwd, bwd

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.reps

    ff, fb = masked(ones)
    hf, hb = masked(half)
    # the backward kernels read the attention their own forward wrote: each pair runs forward first
    cases = [("fixed (baseline)", fixed_fwd, fixed_bwd), ("var, full counts (baseline)", var_fwd, var_bwd),
             ("mask, full", ff, fb), ("mask, Bernoulli(0.5)", hf, hb)]
    share = float(half.mean())
    fh = open(a.out, "a") if a.out else None
    for rnd in range(a.rounds):
        for name, fwd, bwd in cases:
            row = {"probe": "attn_mask", "round": rnd, "case": name, "R": R, "N": N, "H": H, "reps": a.reps,
                   "baseline": os.path.basename(a.baseline) if a.baseline else "own", "visible_share": share,
                   "fwd_us": round(timed(fwd), 1), "bwd_us": round(timed(bwd), 1)}
            line = json.dumps(row)
            print(line, flush=True)
            if fh:
                fh.write(line + "\n")
    if fh:
        fh.close()


if __name__ == "__main__":
    main()
