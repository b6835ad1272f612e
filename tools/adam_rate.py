#!/usr/bin/env python3
"""Rate of the Adam step on the depth network's own parameter list -- every non-buffer entry of engine.param_table():
the conv weights and the BatchNorm gammas and betas, 8 to 192 * 128 * 27 floats -- for

    dffw_adam_step          the C call alone on a table built once: the launches and nothing else
    pipeline.Adam.step()    the optimizer as a training loop calls it (state lookup, argument checks, the ctypes table, the C call)
    torch.optim.Adam        foreach=True and fused=True, same lr, betas and eps

Enqueue-only, after a warm-up, --iters steps between two HIP events and a synchronise; median of --runs runs.  ``ms`` is the events' time per
step: the GPU's time where the GPU is the limit, the host's where the step is launch- or Python-bound; ``host_ms`` is the host clock around the
same loop before the synchronise, the time the training loop's thread spends enqueueing one step.  GB/s counts 28 bytes per parameter (p, g, m,
v read, p, m, v written), beside the HBM copy rate engine.probe_peaks() measures in the same run; the working set, 28 bytes per parameter
less the rewrites, stays in the 256 MB last-level cache from step to step, as it does in training.  One JSON line per variant.

    python tools/adam_rate.py [--runs 7] [--iters 50]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

BYTES_PER_PARAM = 28
LR, BETAS, EPS = 1e-4, (0.9, 0.99), 1e-8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a rate is measured on the GPU"
    torch.set_num_threads(min(16, torch.get_num_threads()))
    from dffinthewild_amd import engine, pipeline
    shapes = [shape for _, shape, flags in engine.param_table() if not flags & 1]
    numel = sum(torch.Size(s).numel() for s in shapes)
    gen = torch.Generator(device="cuda").manual_seed(0)
    _, hbm = engine.probe_peaks(0)

    def fresh():
        ps = [torch.nn.Parameter(torch.randn(s, device="cuda", generator=gen)) for s in shapes]
        for p in ps:
            p.grad = 0.1 * torch.randn(p.shape, device="cuda", generator=gen)
        return ps

    def timed(step):
        def run():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            h0 = time.perf_counter()
            t0.record()
            for _ in range(a.iters):
                step()
            t1.record()
            h1 = time.perf_counter()
            torch.cuda.synchronize()
            return t0.elapsed_time(t1) / a.iters, (h1 - h0) * 1e3 / a.iters
        run()
        runs = [run() for _ in range(a.runs)]
        return statistics.median(r[0] for r in runs), statistics.median(r[1] for r in runs)

    variants = []
    # the C call alone: the table is built once, the state lives in plain tensors
    ps = fresh()
    ms_, vs_ = [torch.zeros_like(p) for p in ps], [torch.zeros_like(p) for p in ps]
    table = (engine.AdamTensor * len(ps))()
    for e, p, m, v in zip(table, ps, ms_, vs_):
        e.param, e.grad, e.exp_avg, e.exp_avg_sq, e.numel = p.data_ptr(), p.grad.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel()
    stream, count = engine._stream_ptr(0), [0]

    def c_call():
        count[0] += 1
        rc = engine.lib.dffw_adam_step(0, table, len(ps), count[0], LR, BETAS[0], BETAS[1], EPS, stream)
        assert rc == 0, engine.lib.dffw_last_error()
    variants.append(("dffw_adam_step (table built once)", c_call))
    ours = pipeline.Adam(fresh(), lr=LR, betas=BETAS, eps=EPS)
    variants.append(("pipeline.Adam.step()", ours.step))
    for name, kw in (("torch.optim.Adam(foreach=True)", dict(foreach=True)), ("torch.optim.Adam(fused=True)", dict(fused=True))):
        variants.append((name, torch.optim.Adam(fresh(), lr=LR, betas=BETAS, eps=EPS, **kw).step))

    for name, step in variants:
        ms, host_ms = timed(step)
        launches = len(engine.op_kernels()) if name.startswith(("dffw", "pipeline")) else None
        print(json.dumps({"variant": name, "tensors": len(shapes), "parameters": numel, "ms": round(ms, 4), "host_ms": round(host_ms, 4),
                          "GBps_at_28B_per_parameter": round(numel * BYTES_PER_PARAM / ms / 1e6, 1), "hbm_copy_GBps": round(hbm, 1),
                          "MB_per_step": round(numel * BYTES_PER_PARAM / 2 ** 20, 1), "launches": launches}), flush=True)


if __name__ == "__main__":
    main()
