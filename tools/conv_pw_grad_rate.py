#!/usr/bin/env python3
"""Rate of the pointwise conv backward's record forms on the heaviest pair of the family: the 8-channel attention tail at
full resolution, k311 (3x1x1, pad (1,0,0)) and k111 (1x1x1) at B = 8, 10 x 256 x 256, and the gradient mask-and-add on the same volume.
Median of --runs runs.

All three are timed enqueue-only (dffw_conv_pw_wgrad / dffw_grad_combine on record buffers, HIP events around --iters calls): kernel time, the
finish launch included.  GB/s is against the bytes the operation needs by construction: the weight gradient reads g and f once each, the
mask-and-add reads a, y and b and writes out.  One JSON line per case.

    python tools/conv_pw_grad_rate.py [--runs 7] [--iters 20] [--precision bf16x3]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

CASES = [("attention.0 (3x1x1)", (3, 1, 1), (1, 0, 0)), ("attention.2 (1x1x1)", (1, 1, 1), (0, 0, 0))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--precision", default="bf16x3")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a rate is measured on the GPU"
    from dffinthewild_amd import engine
    lib, c_int, vp = engine.lib, ctypes.c_int, ctypes.c_void_p
    prec, parts = engine.PRECISIONS[a.precision], 2 if a.precision == "bf16x3" else 1
    B, N, H, W, C = 8, 10, 256, 256, 8
    M = B * N * H * W
    dt = torch.float16 if a.precision == "fp16" else torch.bfloat16
    g = torch.Generator(device="cuda").manual_seed(0)
    # records of the shapes: any finite 16-bit data times alike
    rec = [(torch.rand((M, parts, C), device="cuda", generator=g) - 0.5).to(dt) for _ in range(4)]
    rec_bytes = M * parts * C * 2
    stream = engine._stream_ptr(0)

    def timed(call):
        def run():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.iters):
                rc = call()
                assert rc == 0, lib.dffw_last_error()
            t1.record()
            torch.cuda.synchronize()
            return t0.elapsed_time(t1) / a.iters
        run()
        return statistics.median(run() for _ in range(a.runs))

    for name, k, p in CASES:
        k3, p3 = (c_int * 3)(*k), (c_int * 3)(*p)
        nbytes = lib.dffw_conv_pw_wgrad_workspace_bytes(B, C, N, H, W, C, k3, p3)
        ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        gw = torch.empty((C, C) + k, device="cuda")
        ms = timed(lambda: lib.dffw_conv_pw_wgrad(0, prec, vp(rec[0].data_ptr()), B, C, N, H, W, vp(rec[1].data_ptr()), C, k3, p3, vp(gw.data_ptr()),
                                                  vp(ws.data_ptr()), nbytes, stream))
        print(json.dumps({"case": name, "precision": a.precision, "B": B, "N": N, "H": H, "W": W, "cin": C, "cout": C, "wgrad_ms": round(ms, 4),
                          "GBps_g_and_f_once": round(2 * rec_bytes / ms / 1e6, 1), "GFLOPs": round(2.0 * M * C * C * k[0] / ms / 1e6, 1),
                          "wgrad_workspace_MB": round(nbytes / 2 ** 20, 1), "kernels": ";".join(engine.op_kernels())}))
    for name, y, b, n_io in (("grad_combine mask", rec[1], None, 3), ("grad_combine mask + add", rec[1], rec[2], 4), ("grad_combine add", None, rec[2], 3)):
        ms = timed(lambda: lib.dffw_grad_combine(0, prec, vp(rec[0].data_ptr()), vp(y.data_ptr()) if y is not None else None,
                                                 vp(b.data_ptr()) if b is not None else None, B, C, N, H, W, vp(rec[3].data_ptr()), stream))
        print(json.dumps({"case": name, "precision": a.precision, "B": B, "N": N, "H": H, "W": W, "C": C, "ms": round(ms, 4),
                          "GBps_reads_and_write": round(n_io * rec_bytes / ms / 1e6, 1), "kernels": ";".join(engine.op_kernels())}))


if __name__ == "__main__":
    main()
