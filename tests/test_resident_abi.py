"""CPU tier: the resident schedule's surface (include/lmc_abi.h lmc_resident_stats, lmc_set_option "resident_steps") -- the export, its
declaration, and the Python bindings.  Setting the option needs a context, and a context needs a GPU: the option's behaviour, the refusal of an
unknown name beside it and the refusal on H2MC contexts are checked in tests/test_gpu_resident.py."""
import ctypes
import os
import re

import pytest

from tests import gpu_checks as gc


def _product_lib():
    p = gc.pkg()
    if not os.path.exists(p.LIB_PATH):
        pytest.skip("liblmc_hip.so not built (run `python __graft_entry__.py`)")
    return ctypes.CDLL(p.LIB_PATH)


def test_lmc_resident_stats_is_declared_and_exported():
    hdr = open(os.path.join(gc.ROOT, "include", "lmc_abi.h")).read()
    m = re.search(r"int\s+lmc_resident_stats\s*\(\s*lmc_ctx\s*\*\s*ctx\s*,\s*long long\s*\*\s*out4\s*,\s*double\s*\*\s*kernel_ms\s*\)\s*;", hdr)
    assert m, "lmc_resident_stats(lmc_ctx *ctx, long long *out4, double *kernel_ms) not declared"
    assert '"resident_steps"' in hdr
    assert hasattr(_product_lib(), "lmc_resident_stats")


def test_python_bindings():
    p = gc.pkg()
    assert callable(getattr(p.Renderer, "resident_stats", None))
    assert callable(getattr(p.Group, "resident_stats", None))
    assert p.lib().lmc_resident_stats.argtypes is not None


def test_dpt_amd_documents_the_flag():
    src = open(os.path.join(gc.ROOT, "tools", "dpt_amd.cpp")).read()
    assert '"--resident"' in src and '"resident_steps"' in src
