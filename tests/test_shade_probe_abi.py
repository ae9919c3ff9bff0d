"""CPU tier: the surface of the shading probe (include/lmc_abi.h lmc_shade_probe) -- the declaration, the export, the Python binding, and every refusal:
bad arguments are turned away on the host, before the first device call, with the argument named in lmc_last_error.  What the probe computes needs a
GPU: tests/test_gpu_shade.py."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import gpu_checks as gc
from tests import shade_cases as sc
from tests import shade_ref as sr

ARGS = ("int op, int glossy, int n_mat, const float *materials, int n_bitmaps, const int *bitmap_wh, const float *bitmap_gamma, const float *texels, long long n_texels, "
        "int n, int n_rows, const int *case_ints, const float *case_in, int *out_ok, float *out")


def test_the_call_is_declared_exported_and_bound():
    hdr = open(os.path.join(gc.ROOT, "include", "lmc_abi.h")).read()
    body = r"\s*,\s*".join(r"\s*".join(re.escape(tok) for tok in re.findall(r"\w+|\*", a)) for a in ARGS.split(","))
    assert re.search(r"int\s+lmc_shade_probe\s*\(\s*" + body + r"\s*\)\s*;", hdr)
    assert hdr.index("probes used by the parity tests") < hdr.index("lmc_shade_probe(")
    p = gc.pkg()
    for define, value in (("LMC_SHADE_MAT_WORDS", p.SHADE_MAT_WORDS), ("LMC_SHADE_INT_WORDS", p.SHADE_INT_WORDS), ("LMC_SHADE_IN_WORDS", p.SHADE_IN_WORDS),
                          ("LMC_SHADE_OUT_WORDS", p.SHADE_OUT_WORDS)):
        assert re.search(r"#define\s+%s\s+%d\s" % (define, value), hdr), define
    assert re.search(r"#define\s+LMC_SHADE_UNTOUCHED_BITS\s+0x%xu\s" % p.PROBE_UNTOUCHED_BITS, hdr)
    assert sc.SENTINEL == p.PROBE_SENTINEL and sc.UNTOUCHED_BITS == p.PROBE_UNTOUCHED_BITS
    assert (sr.OP_TEX, sr.OP_EVALUATE, sr.OP_SAMPLE) == tuple(p.SHADE_OPS.index(x) for x in ("tex", "evaluate", "sample"))
    assert sc.MATERIALS.shape[1] == p.SHADE_MAT_WORDS
    for word in ("EvalTex", "BsdfEvaluate", "BsdfSample", "before any device", "n_rows >= n"):
        assert word in hdr, word
    assert hasattr(ctypes.CDLL(p.LIB_PATH), "lmc_shade_probe")
    L = p.lib()
    assert len(L.lmc_shade_probe.argtypes) == len(ARGS.split(",")) and L.lmc_shade_probe.argtypes[8] is ctypes.c_longlong
    assert callable(p.shade_probe)


def test_the_probe_is_a_device_unit_of_its_own_built_strictly_and_shares_the_scene_packing():
    csrc = os.path.join(gc.ROOT, "langevin-mcmc_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"^DEVICE_TUS\s*:=.*\bshade_probe\b", mk, re.M) and re.search(r"^HOST_HIP\s*:=.*\bshade_probes\b", mk, re.M)
    assert not re.search(r"shade_probe\w*\.o\s*:\s*CXXFLAGS", mk) and "-ffp-contract=off" in mk  # no flags of its own: the common, strict ones
    host = open(os.path.join(csrc, "host", "shade_probes.cpp")).read()
    assert "__global__" not in host and "hipLaunchKernelGGL" not in host and "PackMaterials(" in host
    ctx = open(os.path.join(csrc, "host", "context.cpp")).read()
    upload = ctx[ctx.index("static void UploadScene"):]
    assert "PackMaterials(" in upload and "LMC_TEX_INLINE" not in upload  # one packing, called by both
    dev = open(os.path.join(csrc, "device", "shade_probe.hip")).read()
    assert "k_shade_probe<true>" in dev and "k_shade_probe<false>" in dev and "__launch_bounds__(64)" in dev
    twin = open(os.path.join(gc.ROOT, "tests", "helpers", "dshade_host.cpp")).read()
    assert "shade_probe.h" in twin  # the lines a lane runs are the lines the host build runs


def _call(**kw):
    """the raw C call on a small good argument set, any argument replaced by keyword: (return value, message)"""
    p = gc.pkg()
    L, P = p.lib(), p.P
    op, ints, cin = sc.family("edge_textures")
    m, wh, ga, tx, ci, cc = p.shade_probe_args(sc.MATERIALS, sc.BITMAP_WH, sc.BITMAP_GAMMA, sc.TEXELS, ints[:8], cin[:8])
    a = dict(op=op, glossy=1, n_mat=len(m), materials=m, n_bitmaps=len(wh), bitmap_wh=wh, bitmap_gamma=ga, texels=tx, n_texels=len(tx), n=8, n_rows=8, case_ints=ci, case_in=cc,
             out_ok=np.zeros(8, np.int32), out=np.zeros((8, 9), np.float32))
    a.update(kw)
    ptr = lambda x: None if x is None else P(np.ascontiguousarray(x))  # noqa: E731
    keep = {k: (np.ascontiguousarray(v) if isinstance(v, np.ndarray) else v) for k, v in a.items()}
    r = L.lmc_shade_probe(keep["op"], keep["glossy"], keep["n_mat"], ptr(keep["materials"]), keep["n_bitmaps"], ptr(keep["bitmap_wh"]), ptr(keep["bitmap_gamma"]), ptr(keep["texels"]),
                          keep["n_texels"], keep["n"], keep["n_rows"], ptr(keep["case_ints"]), ptr(keep["case_in"]), ptr(keep["out_ok"]), ptr(keep["out"]))
    return r, (L.lmc_last_error() or b"").decode()


def _bad_arguments():
    """(what, replaced arguments, what the message must name) for every refusal of include/lmc_abi.h"""
    out = [("unknown op", dict(op=3), "op = 3"), ("negative op", dict(op=-1), "op = -1"), ("no material", dict(n_mat=0), "n_mat"), ("no case", dict(n=0), "n = 0"),
           ("rows short", dict(n_rows=7), "n_rows"), ("texels short", dict(n_texels=len(sc.TEXELS) - 1), "n_texels")]
    for name in ("materials", "bitmap_wh", "bitmap_gamma", "texels", "case_ints", "case_in", "out_ok", "out"):
        out.append(("null " + name, {name: None}, name + " is null"))
    m = sc.MATERIALS.copy()
    m.view(np.int32)[3, 0] = 3
    out.append(("type 3", dict(materials=m), "materials[3]: type = 3"))
    m = sc.MATERIALS.copy()
    m.view(np.int32)[2, 0] = -1
    out.append(("type -1", dict(materials=m), "materials[2]: type = -1"))
    m = sc.MATERIALS.copy()
    m.view(np.int32)[1, 2 + 6 * 1] = len(sc.BITMAP_WH)
    out.append(("bitmap index = n_bitmaps", dict(materials=m), "materials[1]: Ks.bitmap"))
    m = sc.MATERIALS.copy()
    m.view(np.int32)[0, 2 + 6 * 3] = -2
    out.append(("bitmap index -2", dict(materials=m), "materials[0]: expOrAlpha.bitmap = -2"))
    op, ints, cin = sc.family("edge_textures")
    ci = ints[:8].copy()
    ci[5, 0] = len(sc.MATERIALS)
    out.append(("material index = n_mat", dict(case_ints=ci), "case_ints[5]: material"))
    ci = ints[:8].copy()
    ci[6, 0] = -1
    out.append(("material index -1", dict(case_ints=ci), "case_ints[6]: material = -1"))
    ci = ints[:8].copy()
    ci[2, 2] = 4
    out.append(("texture slot 4", dict(case_ints=ci), "case_ints[2]: texture slot = 4"))
    for k, (w, h) in enumerate(((0, 4), (4, 0), (-1, 3))):
        wh = sc.BITMAP_WH.copy()
        wh[k] = (w, h)
        out.append(("bitmap %d x %d" % (w, h), dict(bitmap_wh=wh), "bitmap_wh[%d]" % k))
    return out


def test_the_probe_refuses_bad_arguments_before_any_device_call():
    """(this tier has no device: a probe that got as far as the device would fail with another message)"""
    for what, kw, needle in _bad_arguments():
        r, msg = _call(**kw)
        assert r != 0 and msg.startswith("lmc_shade_probe: ") and needle in msg and "HIP" not in msg and "device" not in msg, (what, msg)
    with pytest.raises(RuntimeError, match="op = 7"):
        op, ints, cin = sc.family("edge_textures")
        gc.pkg().shade_probe(7, 1, sc.MATERIALS, sc.BITMAP_WH, sc.BITMAP_GAMMA, sc.TEXELS, ints[:4], cin[:4])


def test_the_host_build_refuses_what_the_probe_refuses():
    """(the test helper indexes the same arrays: it must not be the weaker of the two)"""
    p = gc.pkg()
    L = sc._host()
    op, ints, cin = sc.family("edge_textures")
    for what, kw, _ in _bad_arguments():
        if what.startswith("null"):
            continue
        m, wh, ga, tx, ci, cc = p.shade_probe_args(kw.get("materials", sc.MATERIALS), kw.get("bitmap_wh", sc.BITMAP_WH), sc.BITMAP_GAMMA, sc.TEXELS, kw.get("case_ints", ints[:8]), cin[:8])
        ok, out = np.zeros(8, np.int32), np.zeros((8, 9), np.float32)
        r = L.lmc_test_shade_host(kw.get("op", op), 1, kw.get("n_mat", len(m)), p.P(m), len(wh), p.P(wh), p.P(ga), p.P(tx), kw.get("n_texels", len(tx)), kw.get("n", 8), kw.get("n_rows", 8),
                                  p.P(ci), p.P(cc), p.P(ok), p.P(out))
        assert r != 0, what
