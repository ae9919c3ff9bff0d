"""CPU tier: the surface of the exact film (include/lmc_abi.h "Exact film") -- the declarations, the exports, the Python bindings, the dpt_amd flag, and
what needs no GPU: lmc_checkpoint_info's film format on header fixtures built here.  Everything that splats needs a GPU: tests/test_gpu_film_exact.py."""
import ctypes
import os
import re
import struct

import pytest

from tests import gpu_checks as gc

NAMES = ("lmc_film_read_fixed", "lmc_film_overflow", "lmc_film_splat_probe")


def test_the_calls_are_declared_with_the_contract():
    hdr = open(os.path.join(gc.ROOT, "include", "lmc_abi.h")).read()
    for pat in (r"int\s+lmc_film_read_fixed\s*\(\s*lmc_ctx\s*\*\s*ctx\s*,\s*long long\s*\*\s*out\s*\)\s*;",
                r"int\s+lmc_film_overflow\s*\(\s*lmc_ctx\s*\*\s*ctx\s*,\s*long long\s*\*\s*n\s*\)\s*;",
                r"int\s+lmc_film_splat_probe\s*\(\s*int\s+W\s*,\s*int\s+H\s*,\s*int\s+n\s*,\s*const float\s*\*\s*screen_xy\s*,\s*const float\s*\*\s*rgb\s*,\s*int\s+exact\s*,"
                r"\s*long long\s*\*\s*out_fixed\s*,\s*float\s*\*\s*out_float\s*,\s*long long\s*\*\s*overflow\s*\)\s*;"):
        assert re.search(pat, hdr), pat
    for word in ('"film_exact"', "LMC_FILM_EXACT", "llrint((double)v * 4294967296.0)", "2^30", "ELEMENT TYPE FOLLOWS THE MODE", "ncclInt64"):
        assert word in hdr, word


def test_the_calls_are_exported():
    L = ctypes.CDLL(gc.pkg().LIB_PATH)
    for name in NAMES:
        assert hasattr(L, name), name


def test_python_bindings_and_the_cli_flag():
    p = gc.pkg()
    assert callable(getattr(p.Renderer, "film_fixed", None)) and callable(getattr(p.Renderer, "film_overflow", None))
    assert callable(getattr(p.Group, "film_overflow", None)) and callable(getattr(p, "film_splat_probe", None))
    assert p.lib().lmc_film_splat_probe.argtypes is not None and len(p.lib().lmc_film_splat_probe.argtypes) == 9
    src = open(os.path.join(gc.ROOT, "tools", "dpt_amd.cpp")).read()
    assert '"--exact-film"' in src and '"film_exact"' in src


def _header(version, film_format, film_words=12):
    """a checkpoint header as the library lays it out (176 bytes, little endian) for a one-chain file with an empty job-wide section and a one-word record"""
    h = struct.pack("<8sIIQ", b"LMCCKPT\n", version, 176, 0x1234)
    h += struct.pack("<8i", 1, 2, 2, 6, 0, 0, 1, 8)  # force_diffuse, width, height, maxdepth, mindepth, seedoffset, use_gradient, max-derivatives-depth
    h += struct.pack("<6i", 1, 0, 0, 0, 0, film_format)  # mala, h2mc, samplecache, uselightcoordinatesampling, largestepmultiplexed, film format
    h += struct.pack("<6f", 0.3, 1.0, 0.01, 1.0, 0.01, 0.2)
    h += struct.pack("<2i4qd", 1, 64, 100, 0, 1000, 7, 1.5)  # chains, init threads, samples per chain, chains that need one more, init samples, steps done, seconds
    h += struct.pack("<2I2Q", 1, film_words, 0, 176 + 4)  # record words, film words, job bytes, total bytes
    assert len(h) == 176
    return h + b"\0" * 4


def test_checkpoint_info_reports_the_film_format(tmp_path):
    p = gc.pkg()
    f = tmp_path / "float.ckpt"
    f.write_bytes(_header(1, 0))
    info = p.checkpoint_info(str(f))
    assert info["film_format"] == "float32" and info["version"] == 1 and info["steps_done"] == 7 and info["n_chains_total"] == 1
    e = tmp_path / "exact.ckpt"
    e.write_bytes(_header(2, 1))
    info = p.checkpoint_info(str(e))
    assert info["film_format"] == "fixed64" and info["version"] == 2
    for version, fmt in ((1, 1), (2, 0)):  # the version and the format word go together
        bad = tmp_path / "bad.ckpt"
        bad.write_bytes(_header(version, fmt))
        with pytest.raises(RuntimeError, match="film format"):
            p.checkpoint_info(str(bad))
    old = tmp_path / "v3.ckpt"
    old.write_bytes(_header(3, 0))
    with pytest.raises(RuntimeError, match="format version 3"):
        p.checkpoint_info(str(old))
