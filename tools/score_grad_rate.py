#!/usr/bin/env python3
"""Rate of the score convs' backward on records at the volumes the network runs them on: k111 at 8 channels, B = 8,
10 x 256 x 256 (classif3's volume) and k333 at 32 channels, B = 32, 10 x 32 x 32 (confidence.2's): the data gradient without and with a second
gradient b, and the weight gradient with its finish launch.  Median of --runs runs.

Timed enqueue-only (dffw_score_conv_dgrad / dffw_score_conv_wgrad on record buffers, HIP events around --iters calls): kernel time.  GB/s is
against the bytes the operation needs by construction -- g read once; dgrad: b read once where given, out written once; wgrad: x read once --
beside the HBM copy rate engine.probe_peaks() measures in the same run.  Every case states its working set and whether it fits the 256 MB
last-level cache, where repeated calls keep it.  One JSON line per case.

    python tools/score_grad_rate.py [--runs 7] [--iters 20] [--precision bf16x3]
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
# (name, kernel, pad, C, B, N, H, W)
CASES = [("k111 @ 8ch B=8 10x256x256", 1, 0, 8, 8, 10, 256, 256), ("k333 @ 32ch B=32 10x32x32", 3, 1, 32, 32, 10, 32, 32)]


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

    for name, k, p, C, B, N, H, W in CASES:
        M = B * N * H * W
        kk, pp = (ctypes.c_int * 3)(k, k, k), (ctypes.c_int * 3)(p, p, p)
        full, gbytes = M * parts * C * 2, M * 4      # one record volume; the fp32 planar score gradient
        g = torch.rand(M, device="cuda", generator=gen) - 0.5
        w = torch.rand(C * k ** 3, device="cuda", generator=gen) - 0.5
        x, b, out = records(M, C), records(M, C), records(M, C)
        gw = torch.empty(C * k ** 3, device="cuda")
        wsb = lib.dffw_score_conv_wgrad_workspace_bytes(B, C, N, H, W, kk, pp)
        ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
        forms = {
            "dgrad": (gbytes + full, lambda: lib.dffw_score_conv_dgrad(0, prec, vp(g.data_ptr()), B, C, N, H, W, vp(w.data_ptr()), kk, pp, None,
                                                                       vp(out.data_ptr()), stream)),
            "dgrad + b": (gbytes + 2 * full, lambda: lib.dffw_score_conv_dgrad(0, prec, vp(g.data_ptr()), B, C, N, H, W, vp(w.data_ptr()), kk, pp,
                                                                               vp(b.data_ptr()), vp(out.data_ptr()), stream)),
            "wgrad + finish": (gbytes + full, lambda: lib.dffw_score_conv_wgrad(0, prec, vp(x.data_ptr()), vp(g.data_ptr()), B, C, N, H, W, kk, pp,
                                                                                vp(gw.data_ptr()), vp(ws.data_ptr()), wsb, stream)),
        }
        for form, (need, call) in forms.items():
            ms = timed(call)
            print(json.dumps({"case": name, "form": form, "precision": a.precision, "B": B, "N": N, "H": H, "W": W, "C": C, "ms": round(ms, 4),
                              "GBps_by_construction": round(need / ms / 1e6, 1), "hbm_copy_GBps": round(hbm, 1), "working_set_MB": round(need / 2 ** 20, 1),
                              "fits_256MB_llc": need <= LLC_BYTES, "workspace_bytes": wsb, "kernels": ";".join(engine.op_kernels())}), flush=True)


if __name__ == "__main__":
    main()
