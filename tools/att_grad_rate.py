#!/usr/bin/env python3
"""Rate of the attention tail's fused backward against the record-form chain it replaces, on the two heaviest tails:
C = 8 at B = 8, 10 x 256 x 256 and C = 32 at B = 8, 10 x 64 x 64, in the three arithmetics.

  A  dffw_att_tail_backward: one kernel + its finish kernel.
  B  the chain of section 15 on records: dffw_grad_combine (mask by t), dffw_conv_pw_wgrad k111 (+ finish), dffw_grad_combine (mask by a),
     dffw_conv_pw_wgrad k311 (+ finish), dffw_grad_combine (add the skip gradient).  The chain's two adjoint convs have no enqueue-only
     record form (they run inside dffw_op_conv3d, which stages, allocates and synchronises), so they are LEFT OUT of B: B's time here is a lower
     bound of the chain's, 13 of its 17 tensor passes.

Both are timed enqueue-only, HIP events around --iters calls; the runs alternate A B B A and the median of --runs is taken per candidate.
GB/s of A is against 4 reads + 1 write of the records.  One JSON line per row.

    python tools/att_grad_rate.py [--runs 7] [--iters 20] [--only C:precision]      (--only 8:bf16x3: one row, for a kernel trace)
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

ROWS = [(8, 8, 10, 256, 256), (8, 32, 10, 64, 64)]   # (B, C, N, H, W)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--only", default="", help="C:precision of the one row to run")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a rate is measured on the GPU"
    from dffinthewild_amd import engine
    lib, c_int, vp = engine.lib, ctypes.c_int, ctypes.c_void_p
    stream = engine._stream_ptr(0)
    k3, p3, k1, p1 = (c_int * 3)(3, 1, 1), (c_int * 3)(1, 0, 0), (c_int * 3)(1, 1, 1), (c_int * 3)(0, 0, 0)

    def once(call):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(a.iters):
            call()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) / a.iters

    for B, C, N, H, W in ROWS:
        for precision, prec in engine.PRECISIONS.items():
            if a.only and a.only != "%d:%s" % (C, precision):
                continue
            parts = 2 if precision == "bf16x3" else 1
            dt = torch.float16 if precision == "fp16" else torch.bfloat16
            M = B * N * H * W
            g = torch.Generator(device="cuda").manual_seed(0)
            # records of the shapes: any finite 16-bit data times alike; a and t half positive, half zero as behind a ReLU
            x, gy = ((torch.rand((M, parts, C), device="cuda", generator=g) - 0.5).to(dt) for _ in range(2))
            av, tv = (torch.relu(torch.rand((M, 1, C), device="cuda", generator=g) - 0.5).to(dt).repeat(1, parts, 1).contiguous() for _ in range(2))
            gt, ga, gx = (torch.empty_like(x) for _ in range(3))
            w3, w1 = torch.randn(C, C, 3, 1, 1, device="cuda") * 0.1, torch.randn(C, C, 1, 1, 1, device="cuda") * 0.1
            gw3, gw1 = torch.empty_like(w3), torch.empty_like(w1)
            rec_bytes = M * parts * C * 2
            nA = lib.dffw_att_tail_backward_workspace_bytes(B, C, N, H, W)
            n3 = lib.dffw_conv_pw_wgrad_workspace_bytes(B, C, N, H, W, C, k3, p3)
            n1 = lib.dffw_conv_pw_wgrad_workspace_bytes(B, C, N, H, W, C, k1, p1)
            ws = torch.empty(max(nA, n3, n1), dtype=torch.uint8, device="cuda")
            P = lambda t: vp(t.data_ptr())

            def fused():
                rc = lib.dffw_att_tail_backward(0, prec, P(x), P(av), P(tv), P(gy), B, C, N, H, W, P(w3), P(w1), P(gx), P(gw3), P(gw1), P(ws), nA, stream)
                assert rc == 0, lib.dffw_last_error()

            def chain():
                rcs = (lib.dffw_grad_combine(0, prec, P(gy), P(tv), None, B, C, N, H, W, P(gt), stream),
                       lib.dffw_conv_pw_wgrad(0, prec, P(av), B, C, N, H, W, P(gt), C, k1, p1, P(gw1), P(ws), n1, stream),
                       lib.dffw_grad_combine(0, prec, P(gt), P(av), None, B, C, N, H, W, P(ga), stream),      # (stands for the mask of the 1x1x1 adjoint's output)
                       lib.dffw_conv_pw_wgrad(0, prec, P(x), B, C, N, H, W, P(ga), C, k3, p3, P(gw3), P(ws), n3, stream),
                       lib.dffw_grad_combine(0, prec, P(ga), None, P(gy), B, C, N, H, W, P(gx), stream))      # (stands for the add behind the 3x1x1 adjoint)
                assert not any(rcs), lib.dffw_last_error()

            fused()
            names = ";".join(engine.op_kernels())
            once(fused), once(chain)      # warm-up
            ta, tb = [], []
            for i in range(a.runs):
                for cand in ("ABBA" if i % 2 == 0 else "BAAB"):
                    (ta if cand == "A" else tb).append(once(fused if cand == "A" else chain))
            ma, mb = statistics.median(ta), statistics.median(tb)
            print(json.dumps({"B": B, "C": C, "N": N, "H": H, "W": W, "precision": precision, "fused_ms": round(ma, 4),
                              "chain_without_adjoint_convs_ms": round(mb, 4), "fused_over_chain": round(ma / mb, 3),
                              "fused_GBps_4_reads_1_write": round(5 * rec_bytes / ma / 1e6, 1), "fused_min_ms": round(min(ta), 4),
                              "fused_max_ms": round(max(ta), 4), "workspace_MB": round(nA / 2 ** 20, 2), "kernels": names}), flush=True)


if __name__ == "__main__":
    main()
