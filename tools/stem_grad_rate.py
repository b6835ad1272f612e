#!/usr/bin/env python3
"""Rate of the stem's weight gradient where training runs it: the full-resolution image stack at 10 x 224 x 224, B = 4
(2.0 M pixels x 1 944 filter elements) and B = 1.  Median of --runs runs.

Timed enqueue-only (dffw_stem_wgrad on a record buffer of grad_y and the fp32 stack, HIP events around --iters calls, a tenth of a second per
window): the time of a call, both launches.  "useful" TFLOP/s counts 2 x pixels x 1 944 once per call; "issued" counts what the MFMAs do for it (16 x 16 tiles with 8 of 16 rows
and 243 of 256 columns live, three products in split-bf16), beside the MFMA rate engine.probe_peaks() measures in the same run.  One JSON line
per case.

    python tools/stem_grad_rate.py [--runs 7] [--iters 1000] [--precision bf16x3]
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

CASES = [(4, 10, 224, 224), (1, 10, 224, 224)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--precision", default="bf16x3")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a rate is measured on the GPU"
    torch.set_num_threads(min(16, torch.get_num_threads()))
    from dffinthewild_amd import engine
    lib, vp = engine.lib, ctypes.c_void_p
    prec, parts = engine.PRECISIONS[a.precision], 2 if a.precision == "bf16x3" else 1
    dt = torch.float16 if a.precision == "fp16" else torch.bfloat16
    gen = torch.Generator(device="cuda").manual_seed(0)
    stream = engine._stream_ptr(0)
    mfma, _ = engine.probe_peaks(0)
    for B, N, H, W in CASES:
        M = B * N * H * W
        x = torch.rand((B, 3, N, H, W), device="cuda", generator=gen) - 0.5
        gy = (torch.rand((M, parts, 8), device="cuda", generator=gen) - 0.5).to(dt)     # any finite 16-bit data times alike
        wsb = lib.dffw_stem_wgrad_workspace_bytes(B, N, H, W)
        ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
        gw = torch.empty(engine.STEM_WEIGHT_SHAPE, device="cuda")

        def run():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.iters):
                rc = lib.dffw_stem_wgrad(0, prec, vp(x.data_ptr()), vp(gy.data_ptr()), B, N, H, W, vp(gw.data_ptr()), vp(ws.data_ptr()), wsb, stream)
                assert rc == 0, lib.dffw_last_error()
            t1.record()
            torch.cuda.synchronize()
            return t0.elapsed_time(t1) / a.iters
        run()
        ms = statistics.median(run() for _ in range(a.runs))
        useful = 2.0 * M * 8 * 243
        issued = 2.0 * M * 16 * 256 * (3 if parts == 2 else 1)
        print(json.dumps({"case": "stem wgrad", "precision": a.precision, "B": B, "N": N, "H": H, "W": W, "ms": round(ms, 4),
                          "useful_TFLOPs": round(useful / ms / 1e9, 2), "issued_mfma_TFLOPs": round(issued / ms / 1e9, 1), "mfma_peak_TFLOPs": round(mfma, 1),
                          "workspace_MB": round(wsb / 2 ** 20, 2), "kernels": ";".join(engine.op_kernels())}))


if __name__ == "__main__":
    main()
