#!/usr/bin/env python3
"""From an in-place change of every parameter to the end of the next forward, at bench.py's shape (1 x 3 x 10 x 256 x 256,
split-bf16, the depth network), along the two paths Network._engine_on can take:

    rebuild   Network.invalidate() after the change: every entry copied to the host, BatchNorm folded and every layout packed there, a new
              engine uploaded (what every in-place change cost before Engine.update existed)
    update    nothing but the change: the cached engine repacks on the GPU (dffw::repack_fold_kernel, dffw::repack_gather_kernel)

The change is ``p.mul_(1.0)`` on every parameter and buffer: the values stay, the version counters move.  Two Networks with the same weights,
one per path, alternate in one process after a warm-up of both (one model would make every update the first one of a newly rebuilt engine, which
builds that engine's repack plan: that first update is timed once, on its own line); each sample is the time between two device events around
[change, forward], closed by a synchronise, and the host clock around the same (the rebuild is host work: the events measure it because the
stream waits for it).  Both paths must give the bits of the first forward.  Medians and quartiles go to stdout as one JSON line per path and, with --out, into a text file (profiles/repack_time.txt).

    python tools/repack_time.py [--runs 15] [--out profiles/repack_time.txt]
    python tools/repack_time.py --trace 5      # five updates and nothing else timed: the run to put under `rocprofv3 --kernel-trace --stats`
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

B, N, H, W = 1, 10, 256, 256


def quartiles(xs):
    q = statistics.quantiles(xs, n=4)
    return round(q[0], 3), round(statistics.median(xs), 3), round(q[2], 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", type=int, default=0, help="only this many update + forward rounds (for a kernel trace)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a time is measured on the GPU"
    torch.set_num_threads(min(16, torch.get_num_threads()))
    from dffinthewild_amd import graph, synth
    from dffinthewild_amd.Depth_Estimation_Network import Network

    entries = list(graph.param_entries(graph.dff_net_convs()))
    sd = {k: torch.from_numpy(v.copy()) for k, v in synth.state_dict_numpy(entries, seed=0).items()}

    def network():
        m = Network("bf16x3")
        m.load_state_dict(sd)
        return m.cuda().eval()
    models = {"rebuild": network(), "update": network()}
    FS = torch.from_numpy(synth.focal_stack(B, N, H, W, seed=78)).cuda()
    fd = torch.from_numpy(synth.focus_dists(B, N, 1, 1)).cuda()
    tensors = {p: [t for t in m.state_dict(keep_vars=True).values() if torch.is_floating_point(t)] for p, m in models.items()}
    idx = torch.cuda.current_device()

    def change(path):
        with torch.no_grad():
            torch._foreach_mul_(tensors[path], 1.0)

    def round_(path):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        h0 = time.perf_counter()
        model = models[path]
        e0.record()
        change(path)
        if path == "rebuild":
            model.invalidate()
        with torch.no_grad():
            out = model(FS, fd)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), (time.perf_counter() - h0) * 1e3, out

    with torch.no_grad():
        first = models["rebuild"](FS, fd)
        assert all(torch.equal(o, f) for o, f in zip(models["update"](FS, fd), first))
    torch.cuda.synchronize()
    engine0 = models["update"]._engines[idx][1]
    first_update = round_("update")[:2]   # builds the engine's repack plan
    if a.trace:
        for _ in range(a.trace):
            round_("update")
        assert models["update"]._engines[idx][1] is engine0
        print(json.dumps({"traced_update_rounds": a.trace + 1, **engine0.repack_stats()}))
        return
    for path in ("update", "rebuild", "update", "rebuild"):   # warm-up
        round_(path)
    samples = {"rebuild": [], "update": []}
    for _ in range(a.runs):
        for path in ("rebuild", "update"):
            before = models[path]._engines.get(idx, (None, None))[1]
            ms, host_ms, out = round_(path)
            same_engine = models[path]._engines[idx][1] is before
            assert same_engine == (path == "update"), path
            assert all(torch.equal(o, f) for o, f in zip(out, first)), "the %s path changed the forward's bits" % path
            samples[path].append((ms, host_ms))
    assert models["update"]._engines[idx][1] is engine0
    stats = engine0.repack_stats()
    lines = []
    for path in ("rebuild", "update"):
        q = quartiles([s[0] for s in samples[path]])
        hq = quartiles([s[1] for s in samples[path]])
        lines.append(json.dumps({"path": path, "shape": [B, 3, N, H, W], "precision": "bf16x3", "runs": a.runs, "event_ms_q1_median_q3": q,
                                 "host_ms_q1_median_q3": hq}))
    lines.append(json.dumps({"first_update_of_an_engine": {"event_ms": round(first_update[0], 3), "host_ms": round(first_update[1], 3)}}))
    lines.append(json.dumps({"repack_plan": stats}))
    med = {p: statistics.median(s[0] for s in samples[p]) for p in samples}
    lines.append(json.dumps({"rebuild_over_update": round(med["rebuild"] / med["update"], 2)}))
    print("\n".join(lines), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("tools/repack_time.py: in-place change of every parameter -> end of the next forward, %d alternating runs\n" % a.runs)
            f.write("\n".join(lines) + "\n")
    assert med["update"] <= med["rebuild"], "the update path is slower than the rebuild"


if __name__ == "__main__":
    main()
