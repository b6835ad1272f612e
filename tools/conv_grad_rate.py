#!/usr/bin/env python3
"""Rate of the conv backward on three layers of the aggregation network at B=32, 10 x 256 x 256: dres2.conv2 (64 -> 64 at
32 x 32), dres4.conv2 (16 -> 16 at 128 x 128) and dres2.conv3 (64 -> 64, stride (1,2,2), 32 x 32 -> 16 x 16).  Median of --runs runs.

wgrad is timed enqueue-only (dffw_conv_wgrad on record buffers, HIP events around --iters calls): kernel time, with its TFLOP/s (2 * MACs of the
contraction).  forward and dgrad have no enqueue-only single-layer entry: they are timed as whole dffw_op_conv3d / dffw_op_conv3d_backward calls,
which also convert the fp32 NCDHW tensors to records and back, allocate and synchronise -- an upper limit of the kernels' time, not a kernel time.
One JSON line per layer.

    python tools/conv_grad_rate.py [--runs 7] [--iters 10] [--precision bf16x3]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

LAYERS = [   # name, Cin, Cout, kernel, stride, pad, H = W of the input
    ("dres2.conv2", 64, 64, (3, 3, 3), (1, 1, 1), (1, 1, 1), 32),
    ("dres4.conv2", 16, 16, (3, 3, 3), (1, 1, 1), (1, 1, 1), 128),
    ("dres2.conv3", 64, 64, (3, 3, 3), (1, 2, 2), (1, 1, 1), 32),
]


def median_ms(fn, runs):
    fn()
    out = []
    for _ in range(runs):
        out.append(fn())
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--precision", default="bf16x3")
    a = ap.parse_args()
    from dffinthewild_amd import engine
    lib, c_int, vp = engine.lib, ctypes.c_int, ctypes.c_void_p
    prec, parts = engine.PRECISIONS[a.precision], 2 if a.precision == "bf16x3" else 1
    B, N = 32, 10
    g = torch.Generator(device="cuda").manual_seed(0)
    for name, cin, cout, k, s, p, hw in LAYERS:
        ho = hw // s[1]
        x = torch.rand((B, cin, N, hw, hw), device="cuda", generator=g) * 2 - 1
        gy = torch.rand((B, cout, N, ho, ho), device="cuda", generator=g) * 2 - 1
        w = (torch.rand((cout, cin) + k) * 2 - 1) * 0.05
        # records of the same shapes: any finite 16-bit data times alike
        dt = torch.float16 if a.precision == "fp16" else torch.bfloat16
        xr = (torch.rand((B * N * hw * hw, parts, cin), device="cuda", generator=g) - 0.5).to(dt)
        yr = (torch.rand((B * N * ho * ho, parts, cout), device="cuda", generator=g) - 0.5).to(dt)
        k3, s3, p3 = (c_int * 3)(*k), (c_int * 3)(*s), (c_int * 3)(*p)
        nbytes = lib.dffw_conv_wgrad_workspace_bytes(B, cin, N, hw, hw, cout, k3, s3, p3, 0)
        ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        gw = torch.empty((cout, cin) + k, device="cuda")
        stream = engine._stream_ptr(0)

        def wgrad():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.iters):
                rc = lib.dffw_conv_wgrad(0, prec, vp(xr.data_ptr()), B, cin, N, hw, hw, vp(yr.data_ptr()), cout, k3, s3, p3, 0, vp(gw.data_ptr()),
                                         vp(ws.data_ptr()), nbytes, stream)
                assert rc == 0, lib.dffw_last_error()
            t1.record()
            torch.cuda.synchronize()
            return t0.elapsed_time(t1) / a.iters

        def wall(fn):
            def run():
                torch.cuda.synchronize()
                t = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                return (time.perf_counter() - t) * 1e3
            return run

        ms_w = median_ms(wgrad, a.runs)
        kernels = ";".join(engine.op_kernels())
        ms_f = median_ms(wall(lambda: engine.op_conv3d(x, w, stride=s, pad=p, precision=a.precision)), a.runs)
        fwd_kernel = engine.last_conv_kernel()
        ms_d = median_ms(wall(lambda: engine.op_conv3d_backward(x, w, gy, stride=s, pad=p, precision=a.precision, need=("x",))), a.runs)
        flops = 2.0 * B * N * ho * ho * cin * cout * 27
        print(json.dumps({"layer": name, "precision": a.precision, "B": B, "N": N, "H": hw, "W": hw, "cin": cin, "cout": cout, "stride": s[1],
                          "wgrad_ms": round(ms_w, 4), "wgrad_TFLOPs": round(flops / ms_w / 1e9, 2), "wgrad_workspace_MB": round(nbytes / 2 ** 20, 1),
                          "forward_op_call_ms": round(ms_f, 3), "dgrad_op_call_ms": round(ms_d, 3), "forward_kernel": fwd_kernel,
                          "dgrad_kernel": engine.last_conv_kernel(), "wgrad_kernels": kernels}))


if __name__ == "__main__":
    main()
