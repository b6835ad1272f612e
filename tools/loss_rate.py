#!/usr/bin/env python3
"""Rate of the training loss + regression-head backward (dffw_loss_heads) beside the forward heads (dffw_op_regress on the same four
score volumes) in the same process: B=32, 10 x 256 x 256.  Median of --runs timed runs (HIP events around --iters calls on one stream)
after warm-up.  Bytes counted per call: the four score volumes, gt, mask, conf and the focus distances read once, four predictions and
four gradient volumes written.  One JSON line per case.

    python tools/loss_rate.py [--runs 7] [--iters 20]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


def timed(fn, runs, iters):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(iters):
            fn()
        t1.record()
        torch.cuda.synchronize()
        ms.append(t0.elapsed_time(t1) / iters)
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    from dffinthewild_amd import engine
    B, N, H, W = 32, 10, 256, 256
    g = torch.Generator(device="cuda").manual_seed(0)
    scores = [(torch.rand((B, N, H >> (3 - k), W >> (3 - k)), device="cuda", generator=g) * 2 - 1) * 30 for k in range(4)]
    fd = 0.1 + 1.4 * torch.rand((B, N, 1, 1), device="cuda", generator=g)
    gt = 0.1 + 1.4 * torch.rand((B, H, W), device="cuda", generator=g)
    mask = (torch.rand((B, H, W), device="cuda", generator=g) < 0.7).view(torch.uint8)
    conf = torch.rand((B, H, W), device="cuda", generator=g) + 0.05
    ws = torch.empty(engine.loss_workspace_bytes(B, N, H, W), dtype=torch.uint8, device="cuda")
    sbytes = sum(s.numel() for s in scores) * 4
    cases = {
        "regress x4 (forward heads)": (lambda: [engine.op_regress(s, fd, H, W) for s in scores], sbytes + 4 * B * H * W * 4),
        "loss_heads, loss only": (lambda: engine.op_loss_heads(scores, fd, gt, mask, conf, grads=False, workspace=ws), sbytes + B * H * W * (4 * 4 + 4 + 1 + 4 + 4 + 1)),
        "loss_heads, loss + backward": (lambda: engine.op_loss_heads(scores, fd, gt, mask, conf, workspace=ws), 2 * sbytes + B * H * W * (4 * 4 + 4 + 1 + 4 + 4 + 1)),
    }
    base = None
    for name, (fn, nbytes) in cases.items():
        med, lo, hi = timed(fn, a.runs, a.iters)
        base = base or med
        print(json.dumps({"case": name, "B": B, "N": N, "H": H, "W": W, "ms_median": round(med, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4),
                          "us_per_stack": round(med * 1e3 / B, 2), "GBps": round(nbytes / med / 1e6, 1), "x_forward_heads": round(med / base, 2)}))
    print("kernels:", ";".join(engine.op_kernels()))


if __name__ == "__main__":
    main()
