"""CPU tier: the layered mc film's surface (include/lmc_abi.h "Layered mc film": lmc_set_option "mc_layers", lmc_mc_layer_info / _read_layer /
_read_layer_fixed, the Python bindings) and the layered fixed-point CPU oracle tests/helpers/mc_oracle_layers_fx.cpp, pinned to the unlayered one of
tests/test_mc_exact_abi.py and shown to fill the layers the GPU tier (tests/test_gpu_mc_layers.py) compares."""
import ctypes
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from tests import gpu_checks as gc
from tests._orc import P
from tests.test_mc_exact_abi import oracle_mc_fx

HELPER_SRC = os.path.join(gc.ROOT, "tests", "helpers", "mc_oracle_layers_fx.cpp")
HELPER_SO = os.path.join(gc.ROOT, "tests", "helpers", "libmc_oracle_layers_fx.so")
VEACH = os.path.join(gc.ROOT, "scenes", "veachdoor", "lmc.xml")

NEW_SYMBOLS = ("lmc_mc_layer_info", "lmc_mc_read_layer", "lmc_mc_read_layer_fixed")
LENGTH, TECHNIQUE = 1, 2

# tests/test_gpu_mc.py::SCENES with the maxdepth the context ends with (veach-door's own is 8): (scene, force_diffuse, max_depth override, width, height, D)
SCENES = {
    "torus_lambert": (gc.TORUS, 1, 6, 64, 48, 6),
    "torus_materials": (gc.TORUS, 0, 8, 64, 48, 8),
    "veachdoor": (VEACH, 0, 0, 80, 45, 8),
}
SAMPLES = ((0, 2), (7, 3))  # (seed offset, spp)


def layer_count(mode, D):
    return D if mode == LENGTH else D * (D + 3) // 2


def layer_table(mode, D):
    """the (L, -1) / (c, l) of every layer, in layer order, from the numbering rule of the header"""
    if mode == LENGTH:
        return [(L, -1) for L in range(1, D + 1)]
    return [(L + 1 - l, l) for L in range(1, D + 1) for l in range(L + 1)]


def mc_oracle_layers_fx():
    """tests/helpers/mc_oracle_layers_fx.cpp built like tests/test_mc_exact_abi.py builds its helper (the oracle's flags: no contraction, -mfma)"""
    gc.oracle_lib()  # builds the oracle if needed
    deps = [HELPER_SRC, gc.ORACLE_SO]
    if not os.path.exists(HELPER_SO) or os.path.getmtime(HELPER_SO) < max(os.path.getmtime(f) for f in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-mfma",
                               "-I" + os.path.join("langevin-mcmc_amd", "csrc", "host"), HELPER_SRC, "-o", HELPER_SO,
                               "-L" + os.path.join(gc.ROOT, "oracle"), "-llmc_oracle", "-Wl,-rpath,$ORIGIN/../../oracle"], cwd=gc.ROOT)
    L = ctypes.CDLL(HELPER_SO)
    L.mc_oracle_layers_fx_render.restype = ctypes.c_int
    L.mc_oracle_layers_fx_render.argtypes = [ctypes.c_char_p] + [ctypes.c_int] * 8 + [ctypes.c_longlong, ctypes.c_longlong, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                                                                       ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int]
    return L


@functools.lru_cache(maxsize=None)
def _oracle_mc_layers_fx(xml, spp, mode, D, force_diffuse, max_depth, width, height, seed_offset, min_depth, bidir, streams):
    L = mc_oracle_layers_fx()
    begin, end = (0, -1) if streams is None else streams
    n = layer_count(mode, D)
    out = np.zeros((n, height, width, 3), np.int64)
    counts = np.zeros(4, np.int64)
    err = ctypes.create_string_buffer(512)
    rc = L.mc_oracle_layers_fx_render(xml.encode(), force_diffuse, max_depth, width, height, seed_offset, min_depth, int(bidir), spp, begin, end, mode, n,
                                      P(out), P(counts), err, 512)
    assert rc == n, (rc, n, err.value.decode())
    out.setflags(write=False)
    return out, int(counts[0]), int(counts[1]), int(counts[2]), int(counts[3])


def oracle_mc_layers_fx(xml, spp, mode, D, force_diffuse=1, max_depth=6, width=64, height=48, seed_offset=0, min_depth=-1, bidir=True, streams=None):
    """(words int64 [n, H, W, 3]; paths traced; contributions counted; dropped by the range rule; outside the table) of the layered fixed-point oracle;
    D is the maxdepth the scene ends with (the helper refuses another layer count).  Computed once per argument set and shared (read-only)."""
    return _oracle_mc_layers_fx(xml, int(spp), int(mode), int(D), int(force_diffuse), int(max_depth), int(width), int(height), int(seed_offset), int(min_depth), bool(bidir),
                                None if streams is None else (int(streams[0]), int(streams[1])))


def scene_oracle(name, mode, spp, seed_offset, bidir, min_depth=-1, width=None, height=None, xml=None, streams=None):
    sxml, fd, md, W, H, D = SCENES[name]
    return oracle_mc_layers_fx(xml or sxml, spp, mode, D, force_diffuse=fd, max_depth=md, width=width or W, height=height or H, seed_offset=seed_offset, min_depth=min_depth,
                               bidir=bidir, streams=streams)


# ---------------------------------------------------------------------------------------------- surface
def test_layered_mc_entry_points_are_declared_exported_and_bound():
    hdr = open(os.path.join(gc.ROOT, "include", "lmc_abi.h")).read()
    assert re.search(r"int\s+lmc_mc_layer_info\s*\(\s*lmc_ctx\s*\*\s*ctx\s*,\s*int\s*\*\s*mode\s*,\s*int\s*\*\s*n_layers\s*,\s*int\s*\*\s*cl\s*,\s*int\s+cap\s*\)\s*;", hdr)
    assert re.search(r"int\s+lmc_mc_read_layer\s*\(\s*lmc_ctx\s*\*\s*ctx\s*,\s*int\s+layer\s*,\s*float\s*\*\s*rgb\s*\)\s*;", hdr)
    assert re.search(r"int\s+lmc_mc_read_layer_fixed\s*\(\s*lmc_ctx\s*\*\s*ctx\s*,\s*int\s+layer\s*,\s*long long\s*\*\s*words\s*\)\s*;", hdr)
    assert '"mc_layers"' in hdr and "Layered mc film" in hdr
    p = gc.pkg()
    L = ctypes.CDLL(p.LIB_PATH)
    for fn in NEW_SYMBOLS:
        assert hasattr(L, fn), fn
        assert getattr(p.lib(), fn).argtypes is not None, fn
    for m in ("mc_layer_info", "mc_layer", "mc_layer_fixed", "mc_layers", "mc_layers_fixed"):
        assert callable(getattr(p.Renderer, m, None)), m
    src = open(os.path.join(gc.ROOT, "tools", "dpt_amd.cpp")).read()
    for s in ('"--mc-layers"', '"mc_layers"', "lmc_mc_layer_info", "lmc_mc_read_layer"):
        assert s in src, s
    for doc, what in (("INTEGRATION.md", "## Layered mc film"), ("DESIGN.md", "mc_layers"), ("README.md", "mc_layers")):
        assert what in open(os.path.join(gc.ROOT, doc)).read(), doc


def test_layer_numbering_rule():
    assert [layer_count(TECHNIQUE, D) for D in (6, 8, 12)] == [27, 44, 90] and [layer_count(LENGTH, D) for D in (6, 8, 12)] == [6, 8, 12]
    for D in (1, 6, 12):
        t = layer_table(TECHNIQUE, D)
        assert len(t) == len(set(t)) == layer_count(TECHNIQUE, D)
        for k, (c, l) in enumerate(t):
            L = c + l - 1
            assert c >= 1 and 0 <= l <= L <= D and k == (L - 1) * (L + 2) // 2 + l


# ---------------------------------------------------------------------------------------------- the layered oracle
@pytest.mark.parametrize("name", list(SCENES))
@pytest.mark.parametrize("bidir", [True, False])
def test_layered_oracle_sums_to_the_fixed_point_oracle(name, bidir):
    """either mode: the sum of the layers is oracle_mc_fx's film word for word, with its counts, and nothing falls outside the table"""
    sxml, fd, md, W, H, D = SCENES[name]
    for seed_offset, spp in SAMPLES:
        whole = oracle_mc_fx(sxml, spp, force_diffuse=fd, max_depth=md, width=W, height=H, seed_offset=seed_offset, bidir=bidir)
        for mode in (LENGTH, TECHNIQUE):
            layers, paths, counted, dropped, outside = scene_oracle(name, mode, spp, seed_offset, bidir)
            assert layers.shape == (layer_count(mode, D), H, W, 3)
            assert (paths, counted, dropped) == whole[1:] and outside == 0, (paths, counted, dropped, outside, whole[1:])
            assert np.array_equal(layers.sum(0), whole[0])


def _contributions_per_layer(layers):
    """a lower bound of the contributions a layer received: its non-zero pixels"""
    return [int(l.any(-1).sum()) for l in layers]


@pytest.mark.parametrize("name", list(SCENES))
@pytest.mark.parametrize("bidir", [True, False])
def test_the_inputs_exercise_the_layers(name, bidir):
    """on the oracle alone, so that a later change of scene cannot hollow the GPU tests out: every length 2 .. maxdepth is filled and length 1 is not;
    the veach-door bidirectional runs fill at least 35 technique layers (37 and 38 when this was written), light tracing (1, l >= 3) and connections
    (c >= 2, l >= 2) among them; the unidirectional generator only fills (c, 0) and (c, 1)"""
    D = SCENES[name][5]
    for seed_offset, spp in SAMPLES:
        by_len = scene_oracle(name, LENGTH, spp, seed_offset, bidir)[0]
        filled = _contributions_per_layer(by_len)
        assert filled[0] == 0 and all(n >= 1 for n in filled[1:]), (name, bidir, seed_offset, filled)
        by_tech = scene_oracle(name, TECHNIQUE, spp, seed_offset, bidir)[0]
        table = layer_table(TECHNIQUE, D)
        non_empty = [cl for cl, l in zip(table, by_tech) if l.any()]
        print(name, bidir, seed_offset, spp, "lengths", filled, "techniques", len(non_empty), non_empty)
        if name == "veachdoor" and bidir:
            assert len(non_empty) >= 35, len(non_empty)
            assert any(c == 1 and l >= 3 for c, l in non_empty), non_empty
            assert any(c >= 2 and l >= 2 for c, l in non_empty), non_empty
        assert non_empty
        if not bidir:
            assert all(l in (0, 1) for c, l in non_empty), non_empty
