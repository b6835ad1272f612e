"""The refusals and the workspace sizes of the four weight-gradient ABIs (plain, pointwise, stem, score convs), pinned against the library of the
commit before their host code was merged into one file (tests/golden/grad_abi_pins.json, written by tools/grad_abi_pins.py from THAT library):
every call returns what it returned there.  No call reaches the GPU."""
import ctypes
import importlib.util
import json
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("grad_abi_pins", os.path.join(ROOT, "tools", "grad_abi_pins.py"))
pins = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(pins)

# Changed on purpose, by name: {entry: (the new return code, words its message must hold)}.  There are no other exceptions.
#  - the plain convs' record form now refuses a misaligned x, grad_y or workspace (DFFW_EINVAL) as the other three families do; the pinned build
#    did not look, and answered DFFW_ENOMEM for the empty workspace these calls pass;
#  - the stem's alignment refusal says which pointer needs which alignment (the pinned build: "records must be 16-byte aligned" for all three).
STEM_WORDS = ("grad_y", "16-byte", "x (fp32) 4-byte", "workspace 8-byte")
CHANGED = {
    "plain record misaligned x": (-1, ("16-byte",)), "plain record misaligned gy": (-1, ("16-byte",)), "plain record misaligned ws": (-1, ("aligned",)),
    "stem record misaligned x": (-1, STEM_WORDS), "stem record misaligned gy": (-1, STEM_WORDS), "stem record misaligned ws": (-1, STEM_WORDS),
}


def integers(message):
    return set(re.findall(r"-?\d+", message))


@pytest.fixture(scope="module")
def pinned(golden_dir):
    with open(os.path.join(golden_dir, "grad_abi_pins.json")) as f:
        return {k: (v if isinstance(v, list) else [v, None]) for k, v in json.load(f).items()}


def test_the_fixture_holds_the_tools_calls(pinned):
    """The committed fixture is the tool's list, no call dropped from either; and it holds what the pinned build answered where the head
    answers otherwise on purpose."""
    names = []

    def run(name, fn, args):
        names.append(name)
        return pinned[name][0]
    pins.walk(run)
    assert names == list(pinned)
    for name in CHANGED:
        assert pinned[name] == ([-3, pinned[name][1]] if name.startswith("plain") else [-1, "records must be 16-byte aligned"]), name


def test_every_call_answers_as_pinned(lib_built, pinned):
    lib = ctypes.CDLL(lib_built)
    failures = []

    def run(name, fn, args):
        want, want_err = pinned[name]
        rc, err = pins.replay(lib, fn, args)
        if name in CHANGED:
            new_rc, words = CHANGED[name]
            if rc != new_rc or not all(w in err for w in words):
                failures.append((name, "changed on purpose", new_rc, words, rc, err))
        elif rc != want:   # return codes and byte counts: identical
            failures.append((name, "rc", want, rc, err))
        elif rc < 0 and not (err and integers(want_err) <= integers(err)):   # a message, with every integer the pinned one held
            failures.append((name, "message", want_err, err))
        return want   # (the calls short of a workspace size are short of the PINNED size)
    pins.walk(run)
    assert not failures, "%d of %d calls differ, the first: %s" % (len(failures), len(pinned), failures[:5])
