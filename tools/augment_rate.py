#!/usr/bin/env python3
"""Rate of the training-sample assembly (dffw_augment_stack) beside pack_stack on the same source in the same process: pack_stack moves
the same bytes with no arithmetic, so it is the yardstick.  Per case: median of --runs timed runs (HIP events around --iters calls on one
stream) after warm-up, for uint8 and float32 sources, the identity pose and a transposing pose (flip_x, angle 1), with labels.

    B=32 x 10 x 256 x 256 (whole image)      B=8 x 15 x 256 x 256 cropped from 540 x 960

Bytes counted per call: source window + 12 B per output element + labels (gt in, gt / mask out).  One JSON line per case, then the
copy rate dffw_probe_peaks measures on this GPU.

    python tools/augment_rate.py [--runs 7] [--iters 20]
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
    from dffinthewild_amd import engine, pipeline
    peak_m, peak_b = ctypes.c_float(), ctypes.c_float()
    engine._check(engine.lib.dffw_probe_peaks(0, ctypes.byref(peak_m), ctypes.byref(peak_b), None), "dffw_probe_peaks")
    g = torch.Generator(device="cuda").manual_seed(0)
    for B, N, H, W, h in ((32, 10, 256, 256, 256), (8, 15, 540, 960, 256)):
        src = torch.randint(0, 256, (B, N, H, W, 3), dtype=torch.uint8, device="cuda", generator=g)
        gt = torch.rand((B, H, W), device="cuda", generator=g)
        crop = [((7 * b) % (H - h + 1), (13 * b) % (W - h + 1)) for b in range(B)]
        for dtype in (torch.uint8, torch.float32):
            raw = src.to(dtype)
            es = raw.element_size()
            st = raw.stride()
            strides = (ctypes.c_int64 * 5)(st[0], st[1], st[2], st[3], st[4])
            FS = torch.empty((B, 3, N, h, h), device="cuda")
            gt_o, mask_o = torch.empty((B, h, h), device="cuda"), torch.empty((B, h, h), dtype=torch.bool, device="cuda")
            stream, P = engine._stream_ptr(0), (lambda t: ctypes.c_void_p(t.data_ptr()))
            for norm in ("f32", "f64"):
                flag = (0 if dtype == torch.uint8 else 1) | (engine.RAW_NORM_F64 if norm == "f64" else 0)
                # both through the C ABI with preallocated outputs: the kernels, not the Python wrappers, are timed.
                # pack_stack takes one window for the batch: the first sample's
                off = (crop[0][0] * st[2] + crop[0][1] * st[3]) * es
                pk = lambda: engine.lib.dffw_pack_stack(0, ctypes.c_void_p(raw.data_ptr() + off), flag, strides, B, N, h, h, h, h, P(FS), stream)   # noqa: E731
                assert pk() == 0
                pk_ms = timed(pk, a.runs, a.iters)[0]
                stack_bytes = B * N * h * h * 3 * (es + 4)
                for pose, fx, k in (("identity", 0.0, 0), ("transposing", 1.0, 1)):
                    rec = torch.tensor([[y, x, 1.3, 0.05, 0.8, fx, 0.0, k] for y, x in crop], dtype=torch.float64, device="cuda")
                    for labels in (False, True):
                        fn = lambda: engine.lib.dffw_augment_stack(0, P(raw), flag, strides, B, N, H, W, h, h, P(rec), k & 1, P(FS), P(gt) if labels else None,   # noqa: E731
                                                                   None, P(gt_o) if labels else None, P(mask_o) if labels else None, None, 1, 0.1, 0.9, 0.0, stream)
                        assert fn() == 0
                        med, lo, hi = timed(fn, a.runs, a.iters)
                        nbytes = stack_bytes + (B * h * h * 9 if labels else 0)
                        print(json.dumps({"B": B, "N": N, "source": [H, W], "window": h, "src": str(dtype).split(".")[1], "chain": norm, "pose": pose,
                                          "labels": labels, "kernels": engine.op_kernels(), "us_per_call": round(1000 * med, 2),
                                          "us_min_max": [round(1000 * lo, 2), round(1000 * hi, 2)], "us_per_stack": round(1000 * med / B, 3),
                                          "GBps": round(nbytes / med / 1e6, 1), "pack_stack_us_per_call": round(1000 * pk_ms, 2),
                                          "ratio_to_pack_stack": round(med / pk_ms, 3), "share_of_probe_copy_rate": round(nbytes / med / 1e6 / peak_b.value, 3)}),
                              flush=True)
            if dtype == torch.uint8:   # the Python wrapper on the same case (its torch.empty calls and the upload of the parameter record included)
                wr = lambda: pipeline.augment_stack(raw, "NHWC", contrast=1.3, brightness=0.05, gamma=0.8, flip_x=1.0, flip_y=0.0, angle=1, crop=crop,   # noqa: E731
                                                    size=(h, h), gt=gt, gt_range=(0.1, 0.9))
                print(json.dumps({"B": B, "N": N, "wrapper_us_per_call_u8_f32_transposing_labels": round(1000 * timed(wr, a.runs, a.iters)[0], 2)}), flush=True)
    print(json.dumps({"probe_copy_GBps": round(peak_b.value, 1), "runs": a.runs, "iters": a.iters,
                      "note": "C ABI calls with preallocated outputs on one stream; the *_wrapper_* lines time pipeline.augment_stack"}))


if __name__ == "__main__":
    main()
