"""CPU tier: the "mc" integrator's surface (include/lmc_abi.h lmc_mc_render / lmc_mc_read / lmc_mc_stats, the Python bindings, dpt_amd's
dispatch on <string integrator>) and its CPU oracle, tests/helpers/mc_oracle.cpp: the product's stream layout restated over the oracle's
generators, pinned to the reference's own PathTrace loop (pathtrace.cpp:37-69).  The device side is checked against it in
tests/test_gpu_mc.py."""
import ctypes
import os
import re
import subprocess

import numpy as np

from tests import gpu_checks as gc
from tests._orc import P

HELPER_SRC = os.path.join(gc.ROOT, "tests", "helpers", "mc_oracle.cpp")
HELPER_SO = os.path.join(gc.ROOT, "tests", "helpers", "libmc_oracle.so")


def mc_oracle():
    """tests/helpers/mc_oracle.cpp built against oracle/liblmc_oracle.so with the oracle's flags (oracle/Makefile: no contraction, -mfma)"""
    gc.oracle_lib()  # builds the oracle if needed
    deps = [HELPER_SRC, gc.ORACLE_SO]
    if not os.path.exists(HELPER_SO) or os.path.getmtime(HELPER_SO) < max(os.path.getmtime(f) for f in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-mfma",
                               "-I" + os.path.join("langevin-mcmc_amd", "csrc", "host"), HELPER_SRC, "-o", HELPER_SO,
                               "-L" + os.path.join(gc.ROOT, "oracle"), "-llmc_oracle", "-Wl,-rpath,$ORIGIN/../../oracle"], cwd=gc.ROOT)
    L = ctypes.CDLL(HELPER_SO)
    L.mc_oracle_render.restype = ctypes.c_int
    L.mc_oracle_render.argtypes = [ctypes.c_char_p] + [ctypes.c_int] * 8 + [ctypes.c_longlong, ctypes.c_longlong, ctypes.c_int, ctypes.c_void_p,
                                                                              ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int]
    return L


def oracle_mc(xml, spp, force_diffuse=1, max_depth=6, width=64, height=48, seed_offset=0, min_depth=-1, bidir=True, streams=None, literal=False):
    """(film [H, W, 3] weighted by 1 / spp, paths traced, contributions splatted) of the oracle's mc integrator"""
    L = mc_oracle()
    begin, end = (0, -1) if streams is None else streams
    out = np.zeros((height, width, 3), np.float32)
    counts = np.zeros(2, np.int64)
    err = ctypes.create_string_buffer(512)
    rc = L.mc_oracle_render(xml.encode(), force_diffuse, max_depth, width, height, seed_offset, min_depth, int(bidir), spp, begin, end, int(literal),
                            P(out), P(counts), err, 512)
    assert rc == 0, err.value.decode()
    return out, int(counts[0]), int(counts[1])


def test_mc_entry_points_are_declared_and_exported():
    hdr = open(os.path.join(gc.ROOT, "include", "lmc_abi.h")).read()
    assert re.search(r"int\s+lmc_mc_render\s*\(\s*lmc_ctx\s*\*\s*ctx\s*,\s*int\s+spp\s*,\s*long long\s+stream_begin\s*,\s*long long\s+stream_end\s*\)\s*;", hdr)
    assert re.search(r"int\s+lmc_mc_read\s*\(\s*lmc_ctx\s*\*\s*ctx\s*,\s*float\s*\*\s*rgb\s*\)\s*;", hdr)
    assert re.search(r"int\s+lmc_mc_stats\s*\(\s*lmc_ctx\s*\*\s*ctx\s*,\s*long long\s*\*\s*out2\s*\)\s*;", hdr)
    L = ctypes.CDLL(gc.pkg().LIB_PATH)
    for fn in ("lmc_mc_render", "lmc_mc_read", "lmc_mc_stats"):
        assert hasattr(L, fn), fn


def test_python_bindings():
    p = gc.pkg()
    assert callable(getattr(p.Renderer, "mc_render", None)) and callable(getattr(p.Renderer, "mc_stats", None))
    L = p.lib()
    assert L.lmc_mc_render.argtypes is not None and L.lmc_mc_read.argtypes is not None and L.lmc_mc_stats.argtypes is not None


def test_dpt_amd_dispatches_on_the_integrator():
    src = open(os.path.join(gc.ROOT, "tools", "dpt_amd.cpp")).read()
    assert '"integrator_mc"' in src and "lmc_mc_render" in src


def test_helper_stream_layout_is_the_reference_loop_at_one_sample():
    """spp = 1, seedoffset 0: stream t of the layout is RNG(t), the reference's tile stream -- the same film, float for float, and the same
    number of contributions, on the Lambertian torus at 64 x 48 (both generators)"""
    for bidir in (True, False):
        a, pa, na = oracle_mc(gc.TORUS, 1, bidir=bidir)
        b, pb, nb = oracle_mc(gc.TORUS, 1, bidir=bidir, literal=True)
        assert pa == pb == 64 * 48 and na == nb and na > 0, (bidir, pa, pb, na, nb)
        assert np.array_equal(a, b) and a.sum() > 0, bidir


def test_helper_stream_ranges_partition_the_render():
    """two stream ranges sum to the whole render (the CPU adds in a different order, hence the float-sum bar)"""
    nTiles = 4 * 3
    full, p0, n0 = oracle_mc(gc.TORUS, 2, seed_offset=7)
    a, pa, na = oracle_mc(gc.TORUS, 2, seed_offset=7, streams=(0, 9))
    b, pb, nb = oracle_mc(gc.TORUS, 2, seed_offset=7, streams=(9, 2 * nTiles))
    assert pa + pb == p0 == 2 * 64 * 48 and na + nb == n0
    assert np.allclose(a + b, full, rtol=1e-5, atol=1e-7 * full.max())
