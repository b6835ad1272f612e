#!/usr/bin/env python3
"""Rate of the GPU focal-stack simulator (dffw_sim_render): stacks per second at B=32, 10 x 224 x 352 (the reference's working
size and default slice count), timed with HIP events around repeated calls on one stream.  Prints one JSON line.

    python tools/sim_rate.py [--B 32] [--N 10] [--iters 20] [--focal 0.0046]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--N", type=int, default=10)
    ap.add_argument("--H", type=int, default=224)
    ap.add_argument("--W", type=int, default=352)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--focal", type=float, default=0.0046, help="focal length (m) of the camera; F-number 1.8")
    a = ap.parse_args()
    import sim_ref
    from dffinthewild_amd import engine, simulator
    image, depth = sim_ref.case_inputs(1, a.B, a.H, a.W)
    cam = simulator.Camera(a.focal, 1.8, -0.003, 0.012, beta_sigma=5.0, gamma_sigma=5.0, size_ratio=a.W / 4000)
    shifts = simulator.draw_shifts(cam, a.B, a.N, generator=torch.Generator().manual_seed(0))
    img, dep = torch.from_numpy(image).cuda(), torch.from_numpy(depth).cuda()
    args = (img, dep, cam, shifts, a.N, 61625.0, (0.1, 1.0), (0.1, 0.9), 2000)
    ws = torch.empty(engine.sim_workspace_bytes(a.B, a.N, a.H, a.W, 2000), dtype=torch.uint8, device="cuda")
    out = simulator.render(*args, workspace=ws)
    torch.cuda.synchronize()
    rmax = simulator.max_radius([cam], a.N, 61625.0, (0.1, 1.0), (0.1, 0.9), 2000)
    for _ in range(3):
        simulator.render(*args, workspace=ws)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(a.iters):
        simulator.render(*args, workspace=ws)
    t1.record()
    torch.cuda.synchronize()
    ms = t0.elapsed_time(t1) / a.iters
    print(json.dumps({"B": a.B, "N": a.N, "H": a.H, "W": a.W, "max_radius": rmax, "kernels": engine.op_kernels(),
                      "ms_per_call": round(ms, 4), "us_per_stack": round(1000 * ms / a.B, 2), "stacks_per_s": round(a.B * 1000 / ms, 1),
                      "discarded": int(out["status"].sum())}))


if __name__ == "__main__":
    main()
