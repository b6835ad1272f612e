#!/usr/bin/env python3
"""Rate of the regression heads' backward under an upstream gradient (dffw_heads_backward) beside the training loss + backward
(dffw_loss_heads) on the same four score volumes, in the same process and alternating: B=32, 10 x 256 x 256.  Per round one timed run of
each (HIP events around --iters calls on one stream); median, min and max over --runs rounds after warm-up.  Bytes counted per call:
heads_backward reads the four score volumes, four upstream gradients and the focus distances and writes four gradient volumes; loss_heads
reads the scores, gt, mask, conf and the focus distances and writes four predictions and four gradient volumes.  One JSON line per case.

    python tools/heads_grad_rate.py [--runs 7] [--iters 20]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


def timed_once(fn, iters):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters


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
    gps = [torch.randn((B, H, W), device="cuda", generator=g) for _ in range(4)]
    out = [torch.empty_like(s) for s in scores]
    ws = torch.empty(engine.loss_workspace_bytes(B, N, H, W), dtype=torch.uint8, device="cuda")
    sbytes = sum(s.numel() for s in scores) * 4
    cases = {
        "loss_heads, loss + backward": (lambda: engine.op_loss_heads(scores, fd, gt, mask, conf, workspace=ws), 2 * sbytes + B * H * W * (4 * 4 + 4 + 1 + 4)),
        "heads_backward, four heads": (lambda: engine.op_heads_backward(scores, fd, gps, H, W, out=out), 2 * sbytes + B * H * W * 4 * 4),
    }
    kernels = {}
    for name, (fn, _) in cases.items():
        for _ in range(5):
            fn()
        kernels[name] = ";".join(engine.op_kernels())
    torch.cuda.synchronize()
    ms = {name: [] for name in cases}
    for _ in range(a.runs):
        for name, (fn, _) in cases.items():
            ms[name].append(timed_once(fn, a.iters))
    base = statistics.median(ms["loss_heads, loss + backward"])
    for name, (fn, nbytes) in cases.items():
        med, lo, hi = statistics.median(ms[name]), min(ms[name]), max(ms[name])
        print(json.dumps({"case": name, "B": B, "N": N, "H": H, "W": W, "ms_median": round(med, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4),
                          "spread_ms": round(hi - lo, 4), "us_per_stack": round(med * 1e3 / B, 2), "GBps": round(nbytes / med / 1e6, 1),
                          "x_loss_backward": round(med / base, 2)}))
    for name, k in kernels.items():
        print("kernels of %s: %s" % (name, k))


if __name__ == "__main__":
    main()
