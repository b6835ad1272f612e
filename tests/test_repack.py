"""Repacking the weights on the GPU, the part that needs no GPU: the three entry points are exported and declared, they
refuse a null engine before any device is touched, and Engine.update refuses tensors it would have to copy."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("dffw_engine_update", "dffw_engine_repack_stats", "dffw_engine_packed_bytes", "dffw_engine_packed_read")


@pytest.fixture(scope="module")
def eng(lib_built):
    from dffinthewild_amd import engine
    return engine


def test_symbols_are_exported_and_declared(eng):
    header = open(os.path.join(ROOT, "include", "dffw.h")).read()
    declared = set(re.findall(r"\b(dffw_[a-z0-9_]+)\s*\(", header))
    for name in SYMBOLS:
        assert name in declared, name
        assert name in eng.ABI_SYMBOLS, name
        assert getattr(eng.lib, name) is not None


def test_null_engine_is_refused_without_a_device(eng):
    lib = eng.lib
    assert lib.dffw_engine_update(None, None, 0, None) == -1 and b"null engine" in lib.dffw_last_error()
    t = (eng._Tensor * 1)(eng._Tensor(b"x", None, 0))
    assert lib.dffw_engine_update(None, t, 1, None) == -1 and b"null engine" in lib.dffw_last_error()
    assert lib.dffw_engine_packed_bytes(None) == -1 and b"null engine" in lib.dffw_last_error()
    assert lib.dffw_engine_repack_stats(None, (ctypes.c_int64 * 4)()) == -1 and b"null" in lib.dffw_last_error()
    buf = ctypes.create_string_buffer(16)
    assert lib.dffw_engine_packed_read(None, buf, 16, None) == -1 and b"null" in lib.dffw_last_error()


def test_update_refuses_cpu_tensors_by_message(eng):
    """The check runs before the library is called, so an Engine shell without a handle shows it."""
    assert callable(eng.Engine.update) and callable(eng.Engine.packed_bytes)
    shell = object.__new__(eng.Engine)
    shell.index = 0
    with pytest.raises(ValueError, match=r"'w' is on cpu.*cuda:0"):
        shell.update({"w": torch.zeros(4)})
    with pytest.raises(ValueError, match="not a tensor"):
        shell.update({"w": 3.0})
