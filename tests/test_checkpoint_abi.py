"""CPU tier: the surface of checkpoint and resume (include/lmc_abi.h lmc_checkpoint_*) -- the five declarations, the five exports, the Python
bindings, the dpt_amd flags, and the one call that needs no GPU: lmc_checkpoint_info on files that are no checkpoints.  Saving and loading need a
context, and a context needs a GPU: tests/test_gpu_checkpoint.py."""
import ctypes
import os
import re

import pytest

from tests import gpu_checks as gc

NAMES = ("lmc_checkpoint_save", "lmc_checkpoint_load", "lmc_group_checkpoint_save", "lmc_group_checkpoint_load", "lmc_checkpoint_info")


def _product_lib():
    p = gc.pkg()
    if not os.path.exists(p.LIB_PATH):
        pytest.skip("liblmc_hip.so not built (run `python __graft_entry__.py`)")
    return ctypes.CDLL(p.LIB_PATH)


def test_the_five_calls_are_declared():
    hdr = open(os.path.join(gc.ROOT, "include", "lmc_abi.h")).read()
    for pat in (r"int\s+lmc_checkpoint_save\s*\(\s*lmc_ctx\s*\*\s*ctx\s*,\s*const char\s*\*\s*path\s*\)\s*;",
                r"int\s+lmc_checkpoint_load\s*\(\s*lmc_ctx\s*\*\s*ctx\s*,\s*const char\s*\*\s*path\s*\)\s*;",
                r"int\s+lmc_group_checkpoint_save\s*\(\s*lmc_ctx\s*\*\*\s*ctxs\s*,\s*int\s+n\s*,\s*const char\s*\*\s*path\s*\)\s*;",
                r"int\s+lmc_group_checkpoint_load\s*\(\s*lmc_ctx\s*\*\*\s*ctxs\s*,\s*int\s+n\s*,\s*const char\s*\*\s*path\s*\)\s*;",
                r"long long\s+lmc_checkpoint_info\s*\(\s*const char\s*\*\s*path\s*,\s*char\s*\*\s*json\s*,\s*long long\s+cap\s*\)\s*;"):
        assert re.search(pat, hdr), pat


def test_the_five_calls_are_exported():
    L = _product_lib()
    for name in NAMES:
        assert hasattr(L, name), name


def test_python_bindings():
    p = gc.pkg()
    for cls in (p.Renderer, p.Group):
        assert callable(getattr(cls, "save_checkpoint", None)) and callable(getattr(cls, "load_checkpoint", None))
    assert callable(getattr(p, "checkpoint_info", None))
    _product_lib()
    assert p.lib().lmc_checkpoint_info.restype is ctypes.c_longlong


def test_dpt_amd_has_the_flags():
    src = open(os.path.join(gc.ROOT, "tools", "dpt_amd.cpp")).read()
    for flag in ('"--checkpoint"', '"--checkpoint-every"', '"--max-steps"', '"--resume"'):
        assert flag in src, flag
    assert "lmc_group_checkpoint_save" in src and "lmc_group_checkpoint_load" in src


def test_checkpoint_info_refuses_what_is_no_checkpoint(tmp_path):
    p = gc.pkg()
    _product_lib()
    L = p.lib()
    buf = ctypes.create_string_buffer(256)
    garbage = tmp_path / "garbage.ckpt"
    garbage.write_bytes(bytes(range(256)) * 8)
    assert L.lmc_checkpoint_info(os.fsencode(str(garbage)), buf, len(buf)) == -1
    assert "magic" in L.lmc_last_error().decode()
    short = tmp_path / "short.ckpt"
    short.write_bytes(b"LMC")
    assert L.lmc_checkpoint_info(os.fsencode(str(short)), buf, len(buf)) == -1
    assert "shorter than a checkpoint header" in L.lmc_last_error().decode()
    assert L.lmc_checkpoint_info(os.fsencode(str(tmp_path / "missing.ckpt")), buf, len(buf)) == -1
    assert "cannot open" in L.lmc_last_error().decode() and "missing.ckpt" in L.lmc_last_error().decode()
    with pytest.raises(RuntimeError, match="cannot open"):
        p.checkpoint_info(str(tmp_path / "missing.ckpt"))
