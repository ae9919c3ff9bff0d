"""CPU tier: the host side of liblmc_hip.so as several units (csrc/host/: context.cpp for init, the cache transition and the step path; ckpt.cpp,
mcrender.cpp, probes.cpp and plugin_abi.cpp for the cold parts of the ABI; context.h between them).  Every declared call still resolves in the one
library, every moved call is defined where the Makefile and the documents say, and none of the new units holds a kernel."""
import ctypes
import os
import re

from tests import gpu_checks as gc
from tests.test_host import plugin_techniques

HOST = os.path.join(gc.ROOT, "langevin-mcmc_amd", "csrc", "host")
NEW_UNITS = ("ckpt", "mcrender", "probes", "plugin_abi")


def _src(unit):
    return open(os.path.join(HOST, unit + ".cpp")).read()


def test_every_declared_call_resolves_in_the_library():
    L = ctypes.CDLL(gc.pkg().LIB_PATH)
    hdr = open(os.path.join(gc.ROOT, "include", "lmc_abi.h")).read()
    names = set(m[:-1].rstrip() for m in re.findall(r"\blmc_\w+\s*\(", hdr))
    names.discard("lmc_ctx")
    assert len(names) >= 90  # 95 today: a pattern that stopped matching must not pass for "nothing is missing"
    for n in sorted(names):
        assert hasattr(L, n), "missing export " + n
    table = plugin_techniques()
    assert len(table) == 42
    for c, l in table:
        for name in ("evaluate_path_bidir_mala_%d_%d_static", "evaluate_path_bidir_mala_%d_%d_static_derv", "evaluate_path_bidir_%d_%d_static", "evaluate_path_bidir_%d_%d_static_derv"):
            assert hasattr(L, name % (c, l)), "missing export " + name % (c, l)


def test_the_cold_calls_live_in_their_own_host_units():
    mk = open(os.path.join(gc.ROOT, "langevin-mcmc_amd", "csrc", "Makefile")).read()
    for unit in NEW_UNITS + ("context",):
        assert re.search(r"^HOST_HIP\s*:=.*\b%s\b" % unit, mk, re.M), unit
    core = _src("context")
    for definition, unit in (("lmc_checkpoint_save(", "ckpt"), ("lmc_mc_render(", "mcrender"), ("lmc_trace(", "probes"), ("evaluate_path_bidir_", "plugin_abi")):
        assert definition in _src(unit), (definition, unit)
        assert definition not in core, definition
        for other in NEW_UNITS:
            if other != unit:
                assert not re.search(r"^\w[\w \*]*\b" + re.escape(definition), _src(other), re.M), (definition, other)  # defined once (a call from another unit is fine)


def test_the_new_host_units_hold_no_kernels():
    for unit in NEW_UNITS:
        src = _src(unit)
        assert "__global__" not in src and "hipLaunchKernelGGL" not in src, unit  # host code only: the launch functions are device/kernels.h's
