"""CPU tier: the layered MLT film's surface (include/lmc_abi.h "Layered MLT film": lmc_set_option "film_layers", lmc_film_layer_info / _read_layer /
_read_layer_fixed, lmc_chain_splats, lmc_film_layer_splat_probe, the Python bindings, dpt_amd --film-layers) as far as it runs without a device: the
numbering, the validation that comes before any device call, the wrappers' argument checks.  The GPU tier is tests/test_gpu_film_layers.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests import gpu_checks as gc

NEW_SYMBOLS = ("lmc_film_layer_info", "lmc_film_read_layer", "lmc_film_read_layer_fixed", "lmc_chain_splats", "lmc_film_layer_splat_probe")
LENGTH, TECHNIQUE = 1, 2
CLI = os.path.join(gc.ROOT, "langevin-mcmc_amd", "dpt_amd")


def test_entry_points_are_declared_exported_and_bound():
    hdr = open(os.path.join(gc.ROOT, "include", "lmc_abi.h")).read()
    assert re.search(r"int\s+lmc_film_layer_info\s*\(\s*lmc_ctx\s*\*\s*ctx\s*,\s*int\s*\*\s*mode\s*,\s*int\s*\*\s*n_layers\s*,\s*int\s*\*\s*cl\s*,\s*int\s+cap\s*\)\s*;", hdr)
    assert re.search(r"int\s+lmc_film_read_layer\s*\(\s*lmc_ctx\s*\*\s*ctx\s*,\s*int\s+layer\s*,\s*float\s*\*\s*rgb\s*\)\s*;", hdr)
    assert re.search(r"int\s+lmc_film_read_layer_fixed\s*\(\s*lmc_ctx\s*\*\s*ctx\s*,\s*int\s+layer\s*,\s*long long\s*\*\s*words\s*\)\s*;", hdr)
    assert re.search(r"int\s+lmc_chain_splats\s*\(\s*lmc_ctx\s*\*\s*ctx\s*,\s*const int\s*\*\s*chain_ids\s*,\s*int\s+n\s*,\s*int\s+cap\s*,\s*float\s*\*\s*out\s*,\s*int\s*\*\s*counts\s*\)\s*;", hdr)
    assert re.search(r"int\s+lmc_film_layer_splat_probe\s*\(\s*int\s+W\s*,\s*int\s+H\s*,\s*int\s+mode\s*,\s*int\s+D\s*,\s*int\s+n\s*,", hdr)
    assert '"film_layers"' in hdr and "Layered MLT film" in hdr
    p = gc.pkg()
    L = ctypes.CDLL(p.LIB_PATH)
    for fn in NEW_SYMBOLS:
        assert hasattr(L, fn), fn
        assert getattr(p.lib(), fn).argtypes is not None, fn
    for m in ("film_layer_info", "film_layer", "film_layer_fixed", "film_layers_fixed", "chain_splats"):
        assert callable(getattr(p.Renderer, m, None)), m
    assert (p.SPLAT_WORDS, p.SPLAT_MAX_ENTRIES) == tuple(int(re.search(r"#define\s+%s\s+(\d+)" % k, hdr).group(1)) for k in ("LMC_SPLAT_WORDS", "LMC_SPLAT_MAX_ENTRIES"))
    src = open(os.path.join(gc.ROOT, "tools", "dpt_amd.cpp")).read()
    for s in ('"--film-layers"', '"film_layers"', "lmc_film_layer_info", "lmc_film_read_layer"):
        assert s in src, s
    for doc, what in (("INTEGRATION.md", "## Layered MLT film"), ("DESIGN.md", "film_layers"), ("README.md", "film_layers")):
        assert what in open(os.path.join(gc.ROOT, doc)).read(), doc


def test_the_existing_units_do_not_instantiate_the_layered_film():
    """the third film type lives in units of its own: DispatchFilm and the launch functions of the float and exact films never name it"""
    dev = os.path.join(gc.ROOT, "langevin-mcmc_amd", "csrc", "device")
    chain = open(os.path.join(dev, "dchain.h")).read()
    dispatch = chain[chain.index("void DispatchFilm("):chain.index("// image.h:66-77")]
    assert "ChainFilmLayers" not in dispatch
    makefile = open(os.path.join(gc.ROOT, "langevin-mcmc_amd", "csrc", "Makefile")).read()
    for unit in ("step_large", "step_large_mux", "step_large_cache", "step_small_plain", "step_small_leangrad", "step_small_grad"):
        assert unit + "_layers" in makefile
        layered = open(os.path.join(dev, unit + "_layers.hip")).read()
        assert "#define LMC_FILM_LAYERS_TU" in layered and '#include "%s.hip"' % unit in layered
        src = open(os.path.join(dev, unit + ".hip")).read()
        head, _, tail = src.partition("LMC_FILM_LAYERS_TU")
        assert "ChainFilmLayers" not in head and tail, unit  # only behind the guard
    assert "step_mala_finish_layers" in makefile


def test_layer_numbering():
    """the numbering of "mc_layers": length mode D layers, layer L - 1; technique mode D (D + 3) / 2 layers, layer (L - 1)(L + 2) / 2 + l"""
    p = gc.pkg()
    assert [p.film_layer_count(TECHNIQUE, D) for D in (4, 6, 8, 12)] == [14, 27, 44, 90]
    assert [p.film_layer_count(LENGTH, D) for D in (4, 6, 12)] == [4, 6, 12] and p.film_layer_count(0, 6) == 0
    for D in (1, 4, 6, 12):
        table = [(L + 1 - l, l) for L in range(1, D + 1) for l in range(L + 1)]
        assert len(table) == len(set(table)) == p.film_layer_count(TECHNIQUE, D)
        for k, (c, l) in enumerate(table):
            assert p.film_layer_of(TECHNIQUE, c, l) == k and p.film_layer_of(LENGTH, c, l) == c + l - 2
        assert p.film_layer_of(TECHNIQUE, D + 1, 1) >= p.film_layer_count(TECHNIQUE, D) and p.film_layer_of(LENGTH, 1, D + 1) >= D  # L = D + 1: outside the table
    for c, l in ((0, 3), (-2, 5), (3, -1), (1, 0)):  # c < 1, l < 0, L < 1: no such technique
        assert p.film_layer_of(LENGTH, c, l) == p.film_layer_of(TECHNIQUE, c, l) == -1
    # the label of a pending entry: c * 16 + l in one byte, for every technique of the largest table
    assert max(c * 16 + l for L in range(1, 13) for l in range(L + 1) for c in [L + 1 - l]) <= 255
    for bad in (3, -1):
        with pytest.raises(ValueError):
            p.film_layer_count(bad, 6)
        with pytest.raises(ValueError):
            p.film_layer_of(bad, 2, 1)


def test_probe_validation_comes_before_any_device_call():
    """option-style validation of the probe: mode, D, the film size and missing arrays are refused with -1 and a message, without a device"""
    p = gc.pkg()
    L = p.lib()
    xy, v, cl = np.zeros((1, 2), np.float32), np.ones((1, 3), np.float32), np.array([[2, 1]], np.int32)
    for args, what in (((4, 3, 3, 6), "mode"), ((4, 3, 0, 6), "mode"), ((4, 3, 1, 0), "D is"), ((4, 3, 2, 13), "D is"), ((0, 3, 1, 6), "film size"), ((4, -1, 1, 6), "film size")):
        assert L.lmc_film_layer_splat_probe(*args, 1, p.P(xy), p.P(v), p.P(cl), None, None, None) == -1
        assert "lmc_film_layer_splat_probe" in p._err() and what in p._err(), (args, p._err())
    assert L.lmc_film_layer_splat_probe(4, 3, 1, 6, 1, None, p.P(v), p.P(cl), None, None, None) == -1 and "NULL" in p._err()
    with pytest.raises(ValueError):
        p.film_layer_splat_probe(4, 3, 3, 6, xy, v, cl)
    with pytest.raises(ValueError, match="differ in length"):
        p.film_layer_splat_probe(4, 3, 1, 6, xy, v, np.zeros((2, 2), np.int32))


def test_wrapper_argument_checks():
    """the Renderer methods refuse bad arguments before they reach the library (no context needed)"""
    p = gc.pkg()
    ren = object.__new__(p.Renderer)
    ren.h, ren.width, ren.height = None, 4, 3
    with pytest.raises(ValueError, match="at least one chain id"):
        ren.chain_splats([])
    for cap in (0, -1, p.SPLAT_MAX_ENTRIES + 1):
        with pytest.raises(ValueError, match="cap is 1"):
            ren.chain_splats([0], cap=cap)
    for k in (0.5, "1"):
        with pytest.raises((TypeError, ValueError)):
            ren.film_layer(k)
        with pytest.raises((TypeError, ValueError)):
            ren.film_layer_fixed(k)


def test_dpt_amd_flag_parsing():
    assert os.path.exists(CLI), "dpt_amd not built"
    h = subprocess.run([CLI, "--help"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert "--film-layers length|technique" in h.stdout
    r = subprocess.run([CLI, "--film-layers", "depth", "x.xml"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert r.returncode == 2 and "--film-layers: length or technique expected" in r.stdout
