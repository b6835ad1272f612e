"""What the conv dispatch decides, case by case: one line per kernel launch of one profiled forward (kernel name, layer label, flops, bytes,
in launch order, from Engine.profile_collect()), then dffw_workspace_bytes, then the sha256 of every output tensor (a shape the library refuses
shows as one `rejected` line with its message).  Weights and inputs are seeded,
and only the public engine API is used, so two builds of the library (DFFW_LIB_PATH) are compared with `diff`.

The lines hold what the roofline table and the kernel-name assertions see; the grid of a launch (zsplit, persistent workgroups, output-tile offset) is not in
them, so a knob that only moves those (DFFW_ROLL_ZSPLIT, DFFW_ROLL_WGS) shows in the full dump's output hashes alone.

usage: dispatch_dump.py FULL.txt             every case in full (compare two builds)
       dispatch_dump.py --pin FILE.json      the compact form that tests/test_gpu_dispatch.py holds the library to (tests/data/dispatch_pins.json):
                                             per case the launch count, the sha256 of its launch lines and the workspace size; the launch lines
                                             themselves for the default batch-1 and batch-32 cases; no output hashes (they depend on the torch build)
A pull request that retunes a threshold regenerates the pin file on purpose, and its diff shows which cases moved."""
import contextlib
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from dffinthewild_amd import engine, graph, synth  # noqa: E402

SWITCH_SETS = [{"DFFW_" + n: "1"} for n in (
    "NO_ROLL", "NO_ROLLT", "NO_ROLLK", "NO_ROLLX", "NO_SLICE32", "NO_ROLL_S2", "NO_ROLL_S2_WIDE", "NO_TILE", "NO_SPLIT", "NO_SPLITK", "NO_TEAMS",
    "NO_NARROW", "NO_SMALL", "NO_STEM_PAIR", "NO_STEM_PIPE", "NO_FUSED_EFD", "NO_FUSED_SRD", "NO_LEAN_TILE", "NO_LEAN_ROLL")] + [
    {"DFFW_ROLL_MIN_UNITS": "1"}, {"DFFW_ROLL_MIN_UNITS": "1000000"}, {"DFFW_ROLL_MIN_UNITS": "1000000", "DFFW_NO_ROLLT": "1"},
    {"DFFW_ROLLK_MERGE_BELOW": "1"}, {"DFFW_ROLL_ZSPLIT": "2"}, {"DFFW_ROLL_WGS": "8"}, {"DFFW_SMALL_MAX_UNITS": "256"}, {"DFFW_KSPLIT_TARGET": "256"}]
# ... and the ones that walk every form the alignment network chooses between (of_block(), of_first_block(), align_level() in dffw_align.cpp)
E2E_SWITCH_SETS = [{"DFFW_" + n: "1"} for n in (
    "NO_HEAD_SPLIT", "NO_HEAD_WARP", "NO_HEAD_SUMS", "NO_HEAD_SUMS_FUSED", "NO_FUSED_OF", "NO_OF_FIRST", "NO_TILE", "NO_SLICE32")] + [
    {"DFFW_ROLL_MIN_UNITS": "1"}, {"DFFW_ROLL_MIN_UNITS": "1000000"}]


def _tag(env):
    return "+".join(k[5:] + ("" if k[5:8] == "NO_" else "=" + v) for k, v in env.items())


def _cases():
    """(id, net, precision, (B, N, H, W), environment)"""
    out = []
    depth = [(b, 10, 256, 256) for b in (1, 2, 4, 8, 32)] + [(1, 5, 224, 224)]
    depth += [(1, 7, 96, 160), (2, 3, 192, 128), (5, 4, 64, 96), (3, 10, 160, 96), (1, 2, 288, 352), (7, 1, 64, 64)]   # test_oracle_parity_at_shapes_outside_the_fixtures
    # coarse grids that are not whole 8 x 8 columns (28 x 36 at 1/8 resolution = 4 x 5 columns, the last ones partial; H and W are multiples of 32, so the
    # 1/4 grids always are), at a batch that gives conv_rollk / conv_rollt their units there (320 columns): their predicated partial columns.  The
    # End_to_End cases at 480 x 640 (60 x 80 and 30 x 40 grids) have them too
    depth += [(16, 10, 224, 288)]
    for shp in depth:
        out.append(("depth-%dx%dx%dx%d" % shp, "depth", "bf16x3", shp, {}))
    for shp in [(1, 10, 480, 640), (8, 10, 480, 640), (2, 10, 64, 96)]:
        out.append(("e2e-%dx%dx%dx%d" % shp, "e2e", "bf16x3", shp, {}))
    for prec in ("fp16", "bf16"):
        for b in (1, 8):
            out.append(("depth-%dx10x256x256-%s" % (b, prec), "depth", prec, (b, 10, 256, 256), {}))
    for env in SWITCH_SETS:
        for b in (1, 8):
            out.append(("depth-%dx10x256x256-%s" % (b, _tag(env)), "depth", "bf16x3", (b, 10, 256, 256), env))
    # End_to_End: 33 x 10 planes are more than head_warp keeps (320) on 1584 columns, so the split head runs over a [cur | flow] volume; 96 x 160 misses every
    # streaming form (120 columns), once with 3 slices -- which the library rejects: the alignment heads are built for 10 -- and once with 10
    for shp in [(33, 10, 64, 96), (1, 3, 96, 160), (1, 10, 96, 160)]:
        out.append(("e2e-%dx%dx%dx%d" % shp, "e2e", "bf16x3", shp, {}))
    for env in E2E_SWITCH_SETS:
        for b in (1, 8):
            out.append(("e2e-%dx10x480x640-%s" % (b, _tag(env)), "e2e", "bf16x3", (b, 10, 480, 640), env))
    return out


CASES = _cases()
FULL_LINES = ("depth-1x10x256x256", "depth-32x10x256x256")   # the cases whose launch lines the pin file holds in full

_engines = {}


def _engine(net, prec):
    if (net, prec) not in _engines:
        convs = graph.e2e_convs() if net == "e2e" else graph.dff_net_convs()
        sd = {k: torch.from_numpy(v) for k, v in synth.state_dict_numpy(list(graph.param_entries(convs)), seed=0, profile="smooth").items()}
        _engines[(net, prec)] = engine.Engine(sd, "cuda:0", prec, engine.NET_E2E if net == "e2e" else engine.NET_DEPTH)
    return _engines[(net, prec)]


@contextlib.contextmanager
def _environment(env):
    """The library reads its DFFW_* switches from the process environment at the start of every forward."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def run_case(case):
    """-> (launch lines, workspace bytes, [sha256 of each output]); a shape the library refuses: (one line with its message, -1, [])"""
    try:
        return _run_case(case)
    except ValueError as e:   # (DFFW_EINVAL)
        return ["rejected\t%s" % e], -1, []


def _run_case(case):
    _, net, prec, (B, N, H, W), env = case
    eng = _engine(net, prec)
    dev = eng.device
    FS = torch.from_numpy(synth.focal_stack(B, N, H, W, seed=1000)).to(dev)
    fd = torch.from_numpy(synth.focus_dists(B, N, 1, 1)).to(dev)
    with _environment(env), torch.no_grad():
        eng.profile(True)
        try:
            if net == "e2e":
                fov = (1.0 + 0.06 * torch.arange(N - 1, -1, -1, dtype=torch.float32) / max(N - 1, 1)).repeat(B, 1).to(dev)
                outs = eng.forward_e2e(FS, fd, fov)
            else:
                outs = eng.forward(FS, fd)
            torch.cuda.synchronize(dev)
            rows = eng.profile_collect()
        finally:
            eng.profile(False)
        ws = eng.workspace_bytes(B, N, H, W)
    lines = ["%s\t%s\t%r\t%r" % (kernel, layer, flops, nbytes) for kernel, layer, flops, nbytes, _ in rows]
    return lines, ws, [hashlib.sha256(o.cpu().numpy().tobytes()).hexdigest() for o in outs]


def pin_of(case, lines, ws):
    pin = {"launches": len(lines), "sha256": hashlib.sha256("\n".join(lines).encode()).hexdigest(), "workspace_bytes": ws}
    if case[0] in FULL_LINES:
        pin["lines"] = lines
    return pin


def main(argv):
    pin = len(argv) == 3 and argv[1] == "--pin"
    if not pin and len(argv) != 2:
        sys.exit(__doc__)
    pins, text = {}, []
    for case in CASES:
        lines, ws, hashes = run_case(case)
        pins[case[0]] = pin_of(case, lines, ws)
        text += ["== " + case[0]] + lines + ["workspace_bytes %d" % ws] + ["output %d %s" % (i, h) for i, h in enumerate(hashes)]
        print(case[0], len(lines), "launches", flush=True)
    with open(argv[-1], "w") as f:
        if pin:
            json.dump(pins, f, indent=0, sort_keys=True)
            f.write("\n")
        else:
            f.write("\n".join(text) + "\n")


if __name__ == "__main__":
    main(sys.argv)
