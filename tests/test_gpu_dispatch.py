"""The kernel choice is pinned: for every case of tools/dispatch_dump.py (shapes, precisions, switches) a profiled forward launches the kernels
that tests/data/dispatch_pins.json records -- same names, layer labels, flops, bytes and order, same workspace size.  (A launch's grid -- zsplit,
persistent workgroups, filter offset -- is not part of a line: cases that differ only there pin the same hash as the default.)  A change that moves a
layer to another kernel on purpose regenerates the file (`python tools/dispatch_dump.py --pin tests/data/dispatch_pins.json`) and shows the move in its diff."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "data", "dispatch_pins.json")) as _f:
    PINS = json.load(_f)


def _tool():
    spec = importlib.util.spec_from_file_location("dispatch_dump", os.path.join(ROOT, "tools", "dispatch_dump.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def tool(lib_built):
    return _tool()


def test_the_pin_file_covers_the_tools_cases(tool):
    assert sorted(PINS) == sorted(c[0] for c in tool.CASES)
    for name in tool.FULL_LINES:
        assert len(PINS[name]["lines"]) == PINS[name]["launches"]


@pytest.mark.gpu
@pytest.mark.parametrize("case_id", sorted(PINS))
def test_dispatch_is_the_pinned_one(tool, case_id):
    case = next(c for c in tool.CASES if c[0] == case_id)
    lines, ws, _ = tool.run_case(case)
    live = tool.pin_of(case, lines, ws)
    if live != PINS[case_id]:
        print("live launches of %s (workspace %d bytes):" % (case_id, ws))
        print("\n".join(lines))
    assert live == PINS[case_id]
