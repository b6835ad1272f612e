"""Pins the refusals and the workspace sizes of the four weight-gradient ABIs (plain, pointwise, stem and score convs) of ONE build of the library.
usage: python tools/grad_abi_pins.py PATH/TO/libdffw.so tests/golden/grad_abi_pins.json

Written for a change that moves the host code of these entry points without changing what they answer: run it against the library of the commit
BEFORE the change, commit the file, and tests/test_grad_abi_pins.py replays every call on the library of the tree it runs in.  No call reaches the
GPU: each is refused first, sizes a workspace, or asks an op form for no output.  The file maps the name of a call of calls() below to what it
returned: rc (an int; the int64 of a *_workspace_bytes function), or [rc, dffw_last_error()] after a refusal (rc < 0).  An argument of a call is an
int (c_int), a list of three ints (const int[3]), None or {"ptr": address} (a pointer), {"i64": value} (int64_t)."""
import ctypes
import itertools
import json
import sys

P = {"ptr": 4096}   # stands for an operand: 16-byte aligned, never dereferenced
NULL = None
BIG = {"i64": 1 << 40}


def off(n):
    return {"ptr": 4096 + n}


def c_args(args):
    """(argtypes, values) of an entry's arguments"""
    types, vals = [], []
    for a in args:
        if isinstance(a, list):
            types.append(ctypes.POINTER(ctypes.c_int))
            vals.append((ctypes.c_int * 3)(*a))
        elif a is None or (isinstance(a, dict) and "ptr" in a):
            types.append(ctypes.c_void_p)
            vals.append(None if a is None else a["ptr"])
        elif isinstance(a, dict):
            types.append(ctypes.c_int64)
            vals.append(a["i64"])
        else:
            types.append(ctypes.c_int)
            vals.append(a)
    return types, vals


def replay(lib, fn, args):
    """(rc, error message or None) of one call"""
    f = getattr(lib, fn)
    f.argtypes, vals = c_args(args)
    f.restype = ctypes.c_int64 if fn.endswith("_workspace_bytes") else ctypes.c_int
    rc = f(*vals)
    lib.dffw_last_error.restype = ctypes.c_char_p
    return rc, lib.dffw_last_error().decode() if rc < 0 else None


# ---- the four families: geometry arguments, and the three forms of each as functions of (precision, shape, channels, geometry, pointers)
ONE = [1, 1, 1]
PLAIN = {"k333": ([3, 3, 3], ONE, ONE, 0), "k133": ([1, 3, 3], ONE, [0, 1, 1], 0), "k333s2": ([3, 3, 3], [1, 2, 2], ONE, 0), "k333t": ([3, 3, 3], [1, 2, 2], ONE, 1)}
PW = {"k311": ([3, 1, 1], [1, 0, 0]), "k111": (ONE, [0, 0, 0])}
SCORE = {"k111": (ONE, [0, 0, 0]), "k333": ([3, 3, 3], ONE)}


def plain(form, geom, shape=(1, 2, 8, 8), ch=(8, 8), prec=0, x=P, gy=P, gw=P, ws=P, wsb=BIG, w=P, gx=P):
    (B, N, H, W), (ci, co), g = shape, ch, list(geom)
    if form == "bytes":
        return "dffw_conv_wgrad_workspace_bytes", [B, ci, N, H, W, co] + g
    if form == "record":
        return "dffw_conv_wgrad", [0, prec, x, B, ci, N, H, W, gy, co] + g + [gw, ws, wsb, NULL]
    return "dffw_op_conv3d_backward", [0, prec, x, B, ci, N, H, W, w, co] + g + [gy, gx, gw, NULL]


def pw(form, geom, shape=(1, 2, 8, 8), ch=(8, 8), prec=0, x=P, gy=P, gw=P, ws=P, wsb=BIG, w=P, gx=P):
    (B, N, H, W), (ci, co), g = shape, ch, list(geom)
    if form == "bytes":
        return "dffw_conv_pw_wgrad_workspace_bytes", [B, ci, N, H, W, co] + g
    if form == "record":
        return "dffw_conv_pw_wgrad", [0, prec, x, B, ci, N, H, W, gy, co] + g + [gw, ws, wsb, NULL]
    return "dffw_op_conv_pw_backward", [0, prec, x, B, ci, N, H, W, w, co] + g + [gy, gx, gw, NULL]


def stem(form, geom=(), shape=(1, 2, 17, 19), ch=None, prec=0, x=P, gy=P, gw=P, ws=P, wsb=BIG, w=None, gx=None):
    B, N, H, W = shape
    if form == "bytes":
        return "dffw_stem_wgrad_workspace_bytes", [B, N, H, W]
    if form == "record":
        return "dffw_stem_wgrad", [0, prec, x, gy, B, N, H, W, gw, ws, wsb, NULL]
    return "dffw_op_stem_backward", [0, prec, x, gy, B, N, H, W, gw, NULL]


def score(form, geom, shape=(1, 2, 8, 8), ch=(8, 1), prec=0, x=P, gy=P, gw=P, ws=P, wsb=BIG, w=P, gx=P, b=NULL, out=P):
    (B, N, H, W), ci, g = shape, ch[0], list(geom)
    if form == "bytes":
        return "dffw_score_conv_wgrad_workspace_bytes", [B, ci, N, H, W] + g
    if form == "record":
        return "dffw_score_conv_wgrad", [0, prec, x, gy, B, ci, N, H, W] + g + [gw, ws, wsb, NULL]
    if form == "dgrad":
        return "dffw_score_conv_dgrad", [0, prec, gy, B, ci, N, H, W, w] + g + [b, out, NULL]
    return "dffw_op_score_conv_backward", [0, prec, x, B, ci, N, H, W, w] + g + [gy, b, gx, gw, NULL]


# (B, N, H, W): one pixel; one pixel past one 4 x 16 unit in each direction; the stem's 16 x 32 unit and one past it; the pointwise family's
# 128-pixel chunk and one past it
VALID_SHAPES = [(1, 1, 1, 1), (2, 3, 5, 18), (1, 5, 16, 32), (1, 5, 17, 33), (1, 2, 8, 16), (1, 2, 3, 43)]
CHANNELS = [(8, 8), (24, 40), (128, 128)]   # (24, 40): ragged over the 16- and 32-channel tiles
BAD_SHAPES = [(0, 2, 8, 8), (1, 0, 8, 8), (1, 2, 0, 8), (1, 2, 8, -2)]
BAD_PLAIN = [([3, 1, 1], ONE, [1, 0, 0], 0), ([3, 3, 3], ONE, [0, 0, 0], 0), ([1, 3, 3], ONE, ONE, 0), ([3, 3, 3], [2, 2, 2], ONE, 0), ([1, 3, 3], [1, 2, 2], [0, 1, 1], 0),
             ([3, 3, 3], ONE, ONE, 1), ([5, 5, 5], ONE, [2, 2, 2], 0)]
BAD_PW = [([3, 3, 3], ONE), ([3, 1, 1], [0, 0, 0]), (ONE, [1, 0, 0]), ([1, 3, 3], [0, 1, 1]), ([3, 1, 1], [1, 1, 1])]
# tests/test_score_grad.py's
BAD_SCORE = [([1, 3, 3], [0, 1, 1]), ([3, 1, 1], [1, 0, 0]), ([3, 3, 3], [0, 0, 0]), (ONE, ONE), ([3, 3, 3], [1, 1, 0]), ([5, 5, 5], [2, 2, 2]), ([3, 3, 1], [1, 1, 0]),
             ([0, 0, 0], [0, 0, 0])]
# 2^31 units of each family (the plain convs count 4 x 16 tiles, the pointwise convs chunks of 128 pixels per sample, the others pixels)
TOO_LARGE = {"plain": [(32768, 65536, 4, 16), (2, 2, 262144, 131072)], "pw": [(1 << 24, 1, 128, 128), (1, 1, 65536, 32768)],
             "stem": [(32768, 1, 256, 256), (1, 65536, 256, 128), (2, 2, 32768, 16384)], "score": [(32768, 1, 256, 256)]}
BELOW = {"plain": (32767, 65536, 4, 16), "pw": ((1 << 24) - 1, 1, 128, 128), "stem": (32767, 1, 256, 256), "score": (32767, 1, 256, 256)}


def calls():
    """[(name, fn, args, short)]: every pinned call; `short`, where the call sizes the workspace of a valid shape: (the record form's (fn, args) with a
    workspace of so many bytes, how many bytes short of the size it is to be called)"""
    out = []

    def add(name, call, short=None, by=8):
        out.append((name,) + call + (short and (short, by),))

    for fam, form_of, geoms, bad_geoms in (("plain", plain, PLAIN, BAD_PLAIN), ("pw", pw, PW, BAD_PW), ("stem", stem, {"stem": ()}, []), ("score", score, SCORE, BAD_SCORE)):
        forms = ("bytes", "record", "op") + (("dgrad",) if fam == "score" else ())
        g0 = next(iter(geoms.values()))
        # valid shapes: the workspace's size, the record form one double short of it, the op form asked for nothing
        for (gname, geom), shape, ch in itertools.product(geoms.items(), VALID_SHAPES, CHANNELS if fam in ("plain", "pw") else [(8, 1), (24, 1), (128, 1)] if fam == "score" else [None]):
            tag = "%s %s %s %s" % (fam, gname, "x".join(map(str, shape)), ch and "%dto%d" % ch)
            add(tag + " bytes", form_of("bytes", geom, shape=shape, ch=ch),
                short=lambda wsb, form_of=form_of, geom=geom, shape=shape, ch=ch: form_of("record", geom, shape=shape, ch=ch, wsb={"i64": wsb}))
            add(tag + " op without outputs", form_of("op", geom, shape=shape, ch=ch, gx=NULL, gw=NULL))
        for form in forms:
            for i, geom in enumerate(bad_geoms):
                add("%s %s wrong kernel or padding %d" % (fam, form, i), form_of(form, geom))
            if fam != "stem":
                add("%s %s null kernel" % (fam, form), form_of(form, [NULL] + list(g0)[1:]))
                for c in (0, 4, 12, 136, -8):
                    add("%s %s Cin %d" % (fam, form, c), form_of(form, g0, ch=(c, 8)))
                    if fam != "score":
                        add("%s %s Cout %d" % (fam, form, c), form_of(form, g0, ch=(8, c)))
            for shape in BAD_SHAPES:
                add("%s %s zero or negative dimension %s" % (fam, form, shape), form_of(form, g0, shape=shape))
            for shape in TOO_LARGE[fam]:
                if not (fam == "plain" and form == "op"):   # (the plain op form leaves this refusal to its record form: nothing to pin without a GPU)
                    add("%s %s too large %s" % (fam, form, shape), form_of(form, g0, shape=shape))
            if form != "bytes":
                for prec in (-1, 3):
                    add("%s %s precision %d" % (fam, form, prec), form_of(form, g0, prec=prec))
        add("%s bytes just below the limit" % fam, form_of("bytes", g0, shape=BELOW[fam]))
        # null and misaligned operands
        for what in ("x", "gy", "gw", "ws"):
            add("%s record null %s" % (fam, what), form_of("record", g0, **{what: NULL}))
        for what in ("x", "gy") + (("w",) if fam not in ("stem",) else ()):
            add("%s op null %s" % (fam, what), form_of("op", g0, **{what: NULL}))
        if fam == "stem":
            add("stem op null gw", stem("op", gw=NULL))
        add("%s record workspace of 0 bytes" % fam, form_of("record", g0, wsb={"i64": 0}))
    add("plain s2 odd H", plain("bytes", PLAIN["k333s2"], shape=(1, 2, 7, 8)))
    add("plain s2 odd W record", plain("record", PLAIN["k333s2"], shape=(1, 2, 8, 9)))
    add("plain s2 odd H op", plain("op", PLAIN["k333s2"], shape=(1, 2, 7, 8)))
    # alignment.  The plain record form is called with no workspace bytes: a build that does not check its alignment answers DFFW_ENOMEM, never a launch
    for what, n in (("x", 8), ("gy", 8), ("ws", 4)):
        add("plain record misaligned %s" % what, plain("record", PLAIN["k333"], wsb={"i64": 0}, **{what: off(n)}))
        add("pw record misaligned %s" % what, pw("record", PW["k311"], **{what: off(n)}))
    for what, n in (("x", 2), ("gy", 8), ("ws", 4)):
        add("stem record misaligned %s" % what, stem("record", **{what: off(n)}))
    for what, n in (("x", 8), ("ws", 4), ("gy", 2), ("gw", 2)):
        add("score record misaligned %s" % what, score("record", SCORE["k111"], **{what: off(n)}))
    for what, n in (("out", 8), ("b", 8), ("gy", 2), ("w", 2)):
        add("score dgrad misaligned %s" % what, score("dgrad", SCORE["k111"], **{what: off(n)}))
    for what in ("gy", "w", "out"):
        add("score dgrad null %s" % what, score("dgrad", SCORE["k111"], **{what: NULL}))
    add("score op b without grad_x", score("op", SCORE["k111"], b=P, gx=NULL))
    add("score op grad_w without x", score("op", SCORE["k111"], x=NULL))
    # the cases of tests/test_score_grad.py and tests/test_stem_grad.py that the lists above do not hold: their workspace sizes (the score test calls
    # one byte short), the stem's shape (1, 2, 17, 19) with a dimension zeroed, the score op asked for nothing at the test's shape
    for (gname, geom), (shape, c) in itertools.product(SCORE.items(), (((1, 2, 8, 8), 8), ((2, 3, 16, 24), 40), ((8, 10, 256, 256), 8), ((32, 10, 32, 32), 32))):
        add("score %s %s C %d bytes" % (gname, shape, c), score("bytes", geom, shape=shape, ch=(c, 1)), by=1,
            short=lambda wsb, geom=geom, shape=shape, c=c: score("record", geom, shape=shape, ch=(c, 1), wsb={"i64": wsb}))
    add("score op without outputs at 1x2x8x8", score("op", SCORE["k111"], gx=NULL, gw=NULL))
    add("stem 4x10x224x224 bytes", stem("bytes", shape=(4, 10, 224, 224)))
    add("stem 1x2x17x19 bytes", stem("bytes"), short=lambda wsb: stem("record", wsb={"i64": wsb}))
    for shape in ((0, 2, 17, 19), (1, 0, 17, 19), (1, 2, 0, 19), (1, 2, 17, -3)):
        for form in ("bytes", "record", "op"):
            add("stem %s zero or negative dimension %s" % (form, shape), stem(form, shape=shape))
    assert len({c[0] for c in out}) == len(out), "names are unique"
    return out


def walk(run):
    """run(name, fn, args) -> rc for every pinned call, in order; the record forms called short of a workspace size take the size from run's answer"""
    for name, fn, args, short in calls():
        rc = run(name, fn, args)
        if short and rc > 0:   # DFFW_ENOMEM, before any launch
            run(name[:-len("bytes")] + "record %d bytes short" % short[1], *short[0](rc - short[1]))


def main():
    lib = ctypes.CDLL(sys.argv[1])
    pinned = {}

    def run(name, fn, args):
        rc, err = replay(lib, fn, args)
        pinned[name] = rc if err is None else [rc, err]
        return rc
    walk(run)
    with open(sys.argv[2], "w") as f:
        f.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(v)) for k, v in pinned.items()) + "\n}\n")
    print("%d calls pinned from %s" % (len(pinned), sys.argv[1]))


if __name__ == "__main__":
    main()
