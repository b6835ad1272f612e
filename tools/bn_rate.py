#!/usr/bin/env python3
"""Rate of train-mode BatchNorm (dffw_bn_train_forward / dffw_bn_train_backward, enqueue-only on activation records, ReLU on, no residual) at
8 channels 10 x 256 x 256 with B = 8 and at 64 channels 10 x 32 x 32 with B = 32, beside PyTorch's F.batch_norm(training=True) forward +
backward on the fp32 NCDHW tensor of the same shape in the same process.  Median of --runs timed runs (HIP events around --iters calls on
one stream) after warm-up.  GB/s against the algorithmic bytes: forward x read twice and y written (3 record volumes); backward x, grad_y
and y read twice and grad_x written (7 record volumes); PyTorch forward + backward 3 + 5 fp32 volumes.  One JSON line per case.

    python tools/bn_rate.py [--runs 7] [--iters 20] [--precision bf16x3]
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

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


def records(t, prec):
    """(B,C,N,H,W) float32 -> the activation records [pixel][part][channel] as an int16 tensor."""
    v = t.permute(0, 2, 3, 4, 1).reshape(-1, t.shape[1])
    if prec == "fp16":
        parts = [v.half().view(torch.int16)]
    else:
        hi = v.bfloat16()
        parts = [hi.view(torch.int16)] + ([(v - hi.float()).bfloat16().view(torch.int16)] if prec == "bf16x3" else [])
    return torch.stack(parts, 1).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--precision", default="bf16x3")
    a = ap.parse_args()
    from dffinthewild_amd import engine
    lib, prec = engine.lib, engine.PRECISIONS[a.precision]
    parts = 2 if a.precision == "bf16x3" else 1
    g = torch.Generator(device="cuda").manual_seed(0)
    for B, C, N, H, W in ((8, 8, 10, 256, 256), (32, 64, 10, 32, 32)):
        x = torch.randn((B, C, N, H, W), device="cuda", generator=g)
        gy = torch.randn((B, C, N, H, W), device="cuda", generator=g)
        xr, gr = records(x, a.precision), records(gy, a.precision)
        yr, gxr = torch.empty_like(xr), torch.empty_like(xr)
        gamma, beta = torch.rand(C, device="cuda", generator=g) + 0.5, torch.rand(C, device="cuda", generator=g) - 0.5
        mean, invstd, dg, db = (torch.empty(C, device="cuda") for _ in range(4))
        nws = lib.dffw_bn_train_workspace_bytes(B, C, N, H, W)
        ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
        stream = engine._stream_ptr(0)
        p = lambda t: t.data_ptr()

        def fwd():
            engine._check(lib.dffw_bn_train_forward(0, prec, p(xr), B, C, N, H, W, p(gamma), p(beta), engine.BN_EPS, 0.1, None, None, None, 1, p(yr), p(mean),
                                                    p(invstd), p(ws), nws, stream), "dffw_bn_train_forward")

        def bwd():
            engine._check(lib.dffw_bn_train_backward(0, prec, p(xr), p(yr), p(gr), B, C, N, H, W, p(gamma), p(mean), p(invstd), 1, p(gxr), None, p(dg), p(db),
                                                     p(ws), nws, stream), "dffw_bn_train_backward")

        xt = x.clone().requires_grad_(True)
        gt, bt = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)

        def torch_fb():
            y = F.batch_norm(xt, None, None, gt, bt, True, 0.1, engine.BN_EPS)
            torch.autograd.grad(y, (xt, gt, bt), gy)

        vol = B * N * H * W * C
        rec = vol * parts * 2
        cases = [("dffw_bn_train_forward", fwd, 3 * rec), ("dffw_bn_train_backward", bwd, 7 * rec), ("dffw forward + backward", lambda: (fwd(), bwd()), 10 * rec),
                 ("torch F.batch_norm forward + backward (fp32 NCDHW)", torch_fb, 8 * vol * 4)]
        for name, fn, nbytes in cases:
            med, lo, hi = timed(fn, a.runs, a.iters)
            print(json.dumps({"case": name, "precision": a.precision if name.startswith("dffw") else "fp32", "B": B, "C": C, "N": N, "H": H, "W": W,
                              "ms_median": round(med, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4), "MB": round(nbytes / 1e6, 1),
                              "GBps": round(nbytes / med / 1e6, 1), "Gelem_per_s": round(vol / med / 1e6, 2)}), flush=True)
        fwd()
        print("kernels:", ";".join(engine.op_kernels()))


if __name__ == "__main__":
    main()
