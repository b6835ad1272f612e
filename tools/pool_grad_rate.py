#!/usr/bin/env python3
"""Rate of the pool backward's record forms at B = 8 where the network runs them: the (1,2,2) max pool of the 8-channel
volume at 10 x 256 x 256 and of the 16-channel volume at 10 x 128 x 128 (the second branch of the two res_stride_conv_3d blocks), the
(1,2,2) average at the same volumes for comparison, and the pyramid's three averages at 32 channels on 10 x 64 x 64.  Median of --runs runs.

Timed enqueue-only (dffw_pool_backward / dffw_pool3_backward on record buffers, HIP events around --iters calls): kernel time.  GB/s is
against the bytes the operation needs by construction -- max reads g and x and writes out; avg reads g and writes out; the pyramid reads g2,
g4, g8 and writes out -- beside the HBM copy rate engine.probe_peaks() measures in the same run.  Every case states its working set (all
operands) and whether it fits the 256 MB last-level cache, where repeated calls keep it.  One JSON line per case.

    python tools/pool_grad_rate.py [--runs 7] [--iters 20] [--precision bf16x3]
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

LLC_BYTES = 256 * 2 ** 20
# (name, mode, k, C, H, W); N = 10
CASES = [("max 2 @ 8ch 256x256", "max", 2, 8, 256, 256), ("avg 2 @ 8ch 256x256", "avg", 2, 8, 256, 256),
         ("max 2 @ 16ch 128x128", "max", 2, 16, 128, 128), ("avg 2 @ 16ch 128x128", "avg", 2, 16, 128, 128),
         ("pyramid @ 32ch 64x64", "pyramid", 8, 32, 64, 64)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--precision", default="bf16x3")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a rate is measured on the GPU"
    torch.set_num_threads(min(16, torch.get_num_threads()))
    from dffinthewild_amd import engine
    lib, vp = engine.lib, ctypes.c_void_p
    prec, parts = engine.PRECISIONS[a.precision], 2 if a.precision == "bf16x3" else 1
    B, N = 8, 10
    dt = torch.float16 if a.precision == "fp16" else torch.bfloat16
    gen = torch.Generator(device="cuda").manual_seed(0)
    stream = engine._stream_ptr(0)
    _, hbm = engine.probe_peaks(0)

    def records(pixels, C):     # any finite 16-bit data times alike
        return (torch.rand((pixels, parts, C), device="cuda", generator=gen) - 0.5).to(dt)

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

    for name, mode, k, C, H, W in CASES:
        M = B * N * H * W
        full = M * parts * C * 2      # bytes of one record volume at the input resolution
        out = records(M, C)
        if mode == "pyramid":
            gs = [records(M // (kk * kk), C) for kk in (2, 4, 8)]
            need = full + full // 4 + full // 16 + full // 64
            ms = timed(lambda: lib.dffw_pool3_backward(0, prec, vp(gs[0].data_ptr()), vp(gs[1].data_ptr()), vp(gs[2].data_ptr()), None, B, C, N, H, W,
                                                       vp(out.data_ptr()), stream))
        else:
            g = records(M // (k * k), C)
            x = records(M, C) if mode == "max" else None
            need = full + full // (k * k) + (full if x is not None else 0)
            ms = timed(lambda: lib.dffw_pool_backward(0, prec, engine.POOL_MODES[mode], k, vp(g.data_ptr()), vp(x.data_ptr()) if x is not None else None, None,
                                                      B, C, N, H, W, vp(out.data_ptr()), stream))
        print(json.dumps({"case": name, "precision": a.precision, "B": B, "N": N, "H": H, "W": W, "C": C, "ms": round(ms, 4),
                          "GBps_by_construction": round(need / ms / 1e6, 1), "hbm_copy_GBps": round(hbm, 1), "working_set_MB": round(need / 2 ** 20, 1),
                          "fits_256MB_llc": need <= LLC_BYTES, "kernels": ";".join(engine.op_kernels())}))


if __name__ == "__main__":
    main()
