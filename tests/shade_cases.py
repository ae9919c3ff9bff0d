"""The cases of the shading probe (include/lmc_abi.h lmc_shade_probe), the host build of the same source (tests/helpers/dshade_host.cpp) and the
comparisons tests/test_shade_cases.py (CPU) and tests/test_gpu_shade.py (device) share.

One material table and one bitmap list serve every family.  A family is (op, case_ints [n, 3], case_in [n, 20]) of at most 4096 cases; directions are
built in float64 and rounded to float32 once -- device, host build and reference all read the rounded words.  Two sets:
  edge_*   the thresholds, the special normals, the extreme parameters.  Asserted by bit equality (device = host build) and by decision agreement.
  cond_*   constructed so that the formulas are well-conditioned (every cosine at least 0.05 from its threshold, normal.z > -0.9, micro-normals with
           tan / alpha <= 2, Phong R.wo >= 0.5 and exponents <= 200, gamma-1 bitmaps at |st| < 64), drawn at random from those constructions and kept
           where the float64 reference is decisive: these also get the tolerance bars of tests/shade_ref.py.
`python -m tests.shade_cases --measure` prints shade_ref.MEASURED (reference float32 against reference float64; nothing of the product runs)."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np

from tests import shade_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -0x5A5A5A5B
UNTOUCHED_BITS = 0x7FC0BEEF
MAX_FAMILY = 4096
EPS = np.float32(1e-4)
F32 = np.float32
ONE_M = np.nextafter(F32(1), F32(0))  # 1 - ulp


# ------------------------------------------------------------------------------------------------ the host build
def host_shade_lib():
    """device/dshade.h through device/shade_probe.h compiled for the host with the product's arithmetic contract (no contraction; -mfma so that the
    EXPLICIT fused multiply-adds of dtrans.h / dtrig.h are the instruction), built on demand like gpu_checks.host_trans_lib"""
    so = os.path.join(ROOT, "tests", "helpers", "libdshade_host.so")
    src = os.path.join(ROOT, "tests", "helpers", "dshade_host.cpp")
    dev = os.path.join(ROOT, "langevin-mcmc_amd", "csrc", "device")
    hdrs = [os.path.join(dev, h) for h in ("shade_probe.h", "dshade.h", "dscene.h", "dmath.h", "dtrans.h", "dtrig.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in [src] + hdrs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-mfma", src, "-o", so], cwd=ROOT)
    return so


@functools.lru_cache(None)
def _host():
    L = ctypes.CDLL(host_shade_lib())
    vp, ci = ctypes.c_void_p, ctypes.c_int
    L.lmc_test_shade_host.argtypes = [ci, ci, ci, vp, ci, vp, vp, vp, ctypes.c_longlong, ci, ci, vp, vp, vp, vp]
    return L


def _pkg():
    import importlib

    return importlib.import_module("langevin-mcmc_amd")


def host_shade(op, glossy, ints, cin, n=None, n_rows=None, materials=None):
    """the host build on the first n cases: (ok [n_rows], out [n_rows, 9]), pre-filled like the device probe's outputs"""
    p = _pkg()
    m, wh, ga, tx, ci, cc = p.shade_probe_args(MATERIALS if materials is None else materials, BITMAP_WH, BITMAP_GAMMA, TEXELS, ints, cin)
    n = len(cc) if n is None else n
    n_rows = n if n_rows is None else n_rows
    ok = np.full(n_rows, SENTINEL, np.int32)
    out = np.full((n_rows, 9), UNTOUCHED_BITS, np.uint32).view(np.float32)
    r = _host().lmc_test_shade_host(op, glossy, len(m), p.P(m), len(wh), p.P(wh), p.P(ga), p.P(tx), len(tx), n, n_rows, p.P(ci), p.P(cc), p.P(ok), p.P(out))
    assert r == 0, "the host build refused the cases"
    return ok, out


def device_shade(op, glossy, ints, cin, n=None, n_rows=None, materials=None):
    return _pkg().shade_probe(op, glossy, MATERIALS if materials is None else materials, BITMAP_WH, BITMAP_GAMMA, TEXELS, ints, cin, n=n, n_rows=n_rows)


def reference(op, glossy, ints, cin, dtype=np.float64):
    return sr.run(op, glossy, MATERIALS, BITMAP_WH, BITMAP_GAMMA, TEXELS, ints, cin, dtype=dtype)


# ------------------------------------------------------------------------------------------------ bitmaps and materials
def _bitmaps():
    rng = np.random.default_rng(11)
    spec = [  # (W, H, gamma, lo, hi)
        (4, 4, 2.2, 0.05, 1.0),   # 0 colour map, gamma 2.2
        (1, 5, 1.0, 0.05, 1.0),   # 1 one texel wide
        (7, 1, 1.0, 0.05, 1.0),   # 2 one texel high
        (5, 3, 1.0, 0.05, 1.0),   # 3 non-square; gets a negative texel below
        (8, 2, 2.2, 0.05, 4.0),   # 4 non-square, gamma 2.2, values above 1
        (3, 3, 1.0, 5.0, 150.0),  # 5 Phong exponents (channel 0)
        (2, 2, 1.0, 0.1, 0.6),    # 6 dielectric alphas (channel 0)
        (6, 5, 1.0, 0.05, 1.0),   # 7 gamma-1 colour map
    ]
    wh, gamma, tex = [], [], []
    for W, H, g, lo, hi in spec:
        wh.append((W, H)), gamma.append(g)
        tex.append(rng.uniform(lo, hi, (H, W, 3)).astype(F32))
    tex[3][1, 2, :] = (-0.25, 0.5, -1.0)
    return np.array(wh, np.int32), np.array(gamma, F32), np.concatenate([t.ravel() for t in tex])


BITMAP_WH, BITMAP_GAMMA, TEXELS = _bitmaps()
GAMMA1_BITMAPS = (1, 2, 7)  # positive texels, gamma 1: the conditioned texture family
MATERIAL_INDEX = {}


def _tex(bitmap=-1, value=(0.0, 0.0, 0.0), s=1.0, t=1.0):
    return (bitmap, value, s, t)


def _row(type_, two_sided, Kd=_tex(), Ks=_tex(), Kt=_tex(), ea=_tex(), eta=1.0, ks_weight=0.0):
    r = np.zeros(29, F32)
    ri = r.view(np.int32)
    ri[0], ri[1] = type_, two_sided
    for j, (b, v, s, t) in enumerate((Kd, Ks, Kt, ea)):
        o = 2 + 6 * j
        ri[o] = b
        r[o + 1 : o + 4] = v
        r[o + 4], r[o + 5] = s, t
    r[26] = eta
    r[27] = F32(1) / F32(eta)
    r[28] = ks_weight
    return r


def _materials():
    rows = []

    def add(name, row):
        MATERIAL_INDEX[name] = len(rows)
        rows.append(row)

    kd, ks = (0.7, 0.5, 0.3), (0.4, 0.6, 0.8)
    for two in (0, 1):
        add("lam%d" % two, _row(sr.LAMBERTIAN, two, Kd=_tex(value=kd)))
        add("lam%d_tex" % two, _row(sr.LAMBERTIAN, two, Kd=_tex(0, s=2.0, t=-1.5)))
    for two in (0, 1):
        for kw in (0.0, 0.3, 1.0):
            for e in (0.0, 1.0, 30.0, 200.0, 1e4, "tex"):
                ea = _tex(5, s=1.0, t=2.0) if e == "tex" else _tex(value=(e, 0, 0))
                add("phong%d_%g_%s" % (two, kw, e if e == "tex" else "%g" % e), _row(sr.PHONG, two, Kd=_tex(value=kd) if e != 1.0 else _tex(7), Ks=_tex(value=ks) if e != 30.0 else _tex(0), ea=ea, ks_weight=kw))
    for v in (1e-13, 3e-10):  # colours that put MaxCoeff(contrib) below / about its 1e-10 threshold
        add("phong_dim_%g" % v, _row(sr.PHONG, 1, Kd=_tex(value=(v, v, v)), Ks=_tex(value=(v, v, v)), ea=_tex(value=(30.0, 0, 0)), ks_weight=0.3))
    for eta in (1.5, 1 / 1.5, 1.0001):
        for a in (1e-3, 0.03, 0.3, 1.0, "tex"):
            ea = _tex(6, s=3.0, t=1.0) if a == "tex" else _tex(value=(a, 0, 0))
            add("diel_%.4f_%s" % (eta, a if a == "tex" else "%g" % a), _row(sr.ROUGHDIELECTRIC, 0, Ks=_tex(value=(0.9, 0.95, 1.0)) if a != 0.3 else _tex(7, s=0.5), Kt=_tex(value=(1.0, 0.9, 0.8)), ea=ea, eta=eta))
    # texture carriers: the four references of a record name different bitmaps and scales
    add("tex_a", _row(sr.LAMBERTIAN, 1, Kd=_tex(0), Ks=_tex(1, s=1.0, t=3.0), Kt=_tex(2, s=-2.0, t=1.0), ea=_tex(3, s=1.0, t=1.0)))
    add("tex_b", _row(sr.LAMBERTIAN, 1, Kd=_tex(4, s=-0.5, t=0.25), Ks=_tex(5), Kt=_tex(6, s=7.0, t=-7.0), ea=_tex(7, s=1.0, t=1.0)))
    add("tex_c", _row(sr.LAMBERTIAN, 1, Kd=_tex(1, s=1.0, t=1.0), Ks=_tex(2, s=1.0, t=1.0), Kt=_tex(7, s=-3.0, t=0.5), ea=_tex(value=(0.25, 0.5, 0.75))))
    # eta and 1 / eta both exact in float32: Sample's Snell refraction and Evaluate's generalised half vector then agree to float64 rounding (the
    # reference's own identities, tests/test_shade_cases.py); no family uses them
    for eta in (2.0, 0.5):
        for a in (0.03, 0.3, 1.0, "tex"):
            ea = _tex(6, s=3.0, t=1.0) if a == "tex" else _tex(value=(a, 0, 0))
            add("exact_%g_%s" % (eta, a if a == "tex" else "%g" % a), _row(sr.ROUGHDIELECTRIC, 0, Ks=_tex(value=(0.9, 0.95, 1.0)), Kt=_tex(7), ea=ea, eta=eta))
    return np.array(rows, F32)


MATERIALS = _materials()
M = MATERIAL_INDEX


def mats_like(prefix):
    return np.array([i for name, i in MATERIAL_INDEX.items() if name.startswith(prefix)], np.int64)


# ------------------------------------------------------------------------------------------------ building blocks
INIT = dict(pdf=0.125, rev=0.375, cos=-0.625, con=(0.0625, 0.1875, 0.3125))  # what the in / out words hold going in: recognisable bits


def unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def rand_unit(rng, n):
    return unit(rng.normal(size=(n, 3)))


def frame(n):
    """any orthonormal pair perpendicular to the unit vectors n (float64)"""
    helper = np.where((np.abs(n[:, 0:1]) < 0.9), np.array([[1.0, 0, 0]]), np.array([[0, 1.0, 0]]))
    t1 = unit(np.cross(n, helper))
    return t1, np.cross(n, t1)


def with_cos(n, c, phi):
    """unit vectors at cosine c to n, azimuth phi"""
    t1, t2 = frame(n)
    s = np.sqrt(np.maximum(1 - c * c, 0))
    return c[:, None] * n + (s * np.cos(phi))[:, None] * t1 + (s * np.sin(phi))[:, None] * t2


def block(mat, wi, nrm, wo=None, st=None, rnd=None, u=None, adjoint=0, slot=0):
    n = len(wi)
    ints = np.zeros((n, 3), np.int32)
    ints[:, 0], ints[:, 1], ints[:, 2] = mat, adjoint, slot
    cin = np.zeros((n, 20), F32)
    cin[:, sr.IN_WI], cin[:, sr.IN_N] = wi, nrm
    cin[:, sr.IN_WO] = (0.6, 0.0, 0.8) if wo is None else wo
    cin[:, sr.IN_ST] = (0.3, 0.7) if st is None else st
    cin[:, sr.IN_RND] = (0.4, 0.6) if rnd is None else rnd
    cin[:, sr.IN_U] = 0.5 if u is None else u
    cin[:, sr.IN_PDF], cin[:, sr.IN_REV], cin[:, sr.IN_COS], cin[:, sr.IN_CON] = INIT["pdf"], INIT["rev"], INIT["cos"], INIT["con"]
    return ints, cin


def join(blocks):
    ints, cin = np.concatenate([b[0] for b in blocks]), np.concatenate([b[1] for b in blocks])
    assert len(cin) <= MAX_FAMILY and np.isfinite(cin).all()
    return np.ascontiguousarray(ints), np.ascontiguousarray(cin)


def special_normals():
    """(0, 0, -1), n.z a few ulps either side of the frame's switch at -1 + 1e-6, and the axes"""
    out = [(0, 0, 1.0), (0, 0, -1.0), (1.0, 0, 0), (0, -1.0, 0)]
    flip = F32(-1.0 + 1e-6)
    for z in (flip, np.nextafter(flip, F32(0)), np.nextafter(flip, F32(-2)), F32(-1.0 + 3e-6), F32(-1.0 + 1e-4)):
        z = float(z)
        out.append((np.sqrt(1 - z * z), 0.0, z))
    return np.array(out, np.float64)


def normal_pool(rng, n, special_share=0.3):
    nrm = rand_unit(rng, n)
    nrm[:, 2] = np.where(nrm[:, 2] < -0.9, -nrm[:, 2], nrm[:, 2])
    sp = special_normals()
    k = rng.random(n) < special_share
    nrm[k] = sp[rng.integers(0, len(sp), k.sum())]
    return nrm


def side_cos(rng, n, lo=0.02):
    return rng.uniform(lo, 1.0, n) * rng.choice([-1.0, 1.0], n)


def threshold_values():
    """|cos| at c_CosEpsilon, one and three ulps either side, exactly 0, and a little further out (float32 values, both signs)"""
    e = EPS
    v = [F32(0), e, np.nextafter(e, F32(1)), np.nextafter(e, F32(0)), e + 3 * np.spacing(e), e - 3 * np.spacing(e), F32(5e-4), F32(2e-5)]
    return np.array([float(x) for x in v] + [-float(x) for x in v[1:]], np.float64)


def axis_dirs(z):
    """unit vectors whose z component is exactly the float32 value z (|z| small): the dot product with (0, 0, +-1) is then exact in any precision"""
    z = np.asarray(z, np.float64)
    return np.stack([np.sqrt(1 - z * z), np.zeros_like(z), z], 1)


def uniforms(rng, n, edge_share=0.1):
    """float32 uniforms in [0, 1) with some components at 0 and at 1 - ulp"""
    r = rng.random((n, 2)).astype(F32)
    r = np.minimum(r, ONE_M)
    k = rng.random((n, 2)) < edge_share
    r[k] = rng.choice(np.array([0.0, float(ONE_M)], F32), k.sum())
    return r


# ------------------------------------------------------------------------------------------------ edge set
def edge_lambert_evaluate():
    rng = np.random.default_rng(101)
    n = 2600
    lam = mats_like("lam")
    nrm = normal_pool(rng, n)
    b = [block(rng.choice(lam, n), with_cos(nrm, side_cos(rng, n), rng.uniform(0, 7, n)), nrm, with_cos(nrm, side_cos(rng, n), rng.uniform(0, 7, n)), st=rng.uniform(-2, 2, (n, 2)))]
    th = threshold_values()
    for sign in (1.0, -1.0):
        up = np.tile([[0, 0, sign]], (len(th), 1))
        for m in ("lam0", "lam1", "lam1_tex"):
            b.append(block(M[m], axis_dirs(th), up, unit([0.3, 0.4, 0.866 * sign])[None, :].repeat(len(th), 0)))
            b.append(block(M[m], unit([0.3, 0.4, 0.866 * sign])[None, :].repeat(len(th), 0), up, axis_dirs(th)))
    return sr.OP_EVALUATE, *join(b)


def edge_lambert_sample():
    rng = np.random.default_rng(102)
    n = 2600
    lam = mats_like("lam")
    nrm = normal_pool(rng, n)
    b = [block(rng.choice(lam, n), with_cos(nrm, side_cos(rng, n), rng.uniform(0, 7, n)), nrm, rnd=uniforms(rng, n), st=rng.uniform(-2, 2, (n, 2)))]
    b[0][1][:, 12] = np.maximum(b[0][1][:, 12], F32(1e-4))  # (rnd.y = 0, the grazing sample, is a threshold case below)
    th = threshold_values()
    for sign in (1.0, -1.0):
        up = np.tile([[0, 0, sign]], (len(th), 1))
        for m in ("lam0", "lam1"):
            b.append(block(M[m], axis_dirs(th), up, rnd=(0.25, 0.5)))
    # cosWo = sqrt(rnd.y): 0 and the neighbourhood of c_CosEpsilon^2
    ys = np.array([0.0, 1e-8, 0.99e-8, 1.01e-8, 1e-7, 1e-9, float(np.nextafter(F32(0), F32(1)))], F32)
    for x in (0.0, 0.3, float(ONE_M)):
        b.append(block(M["lam1"], np.tile(unit([0.2, -0.5, 0.7]), (len(ys), 1)), np.tile(unit([0.1, 0.2, 0.9]), (len(ys), 1)), rnd=np.stack([np.full(len(ys), x, F32), ys], 1)))
    return sr.OP_SAMPLE, *join(b)


def _around(axis, rng, n, lo):
    """directions whose cosine to `axis` is uniform in [lo, 1]"""
    return with_cos(axis, rng.uniform(lo, 1.0, n), rng.uniform(0, 7, n))


def edge_phong_evaluate():
    rng = np.random.default_rng(103)
    n = 3000
    ph = mats_like("phong")
    nrm = normal_pool(rng, n)
    wi = with_cos(nrm, side_cos(rng, n, 0.05), rng.uniform(0, 7, n))
    facing = nrm * np.sign(np.sum(wi * nrm, 1))[:, None]
    R = 2 * np.sum(wi * facing, 1)[:, None] * facing - wi
    wo = np.where((rng.random(n) < 0.6)[:, None], _around(R, rng, n, 0.9), rand_unit(rng, n))  # inside the lobe, or anywhere (below the surface included)
    b = [block(rng.choice(ph, n), wi, nrm, wo, st=rng.uniform(-2, 2, (n, 2)))]
    # narrow lobes: exponent 1e4 keeps a weight above 1e-10 within 4 degrees of R only
    k = 300
    nn = normal_pool(rng, k, 0.0)
    w2 = with_cos(nn, rng.uniform(0.3, 1.0, k), rng.uniform(0, 7, k))
    R2 = 2 * np.sum(w2 * nn, 1)[:, None] * nn - w2
    b.append(block(rng.choice(mats_like("phong0_0.3_10000"), k), w2, nn, with_cos(R2, np.cos(rng.uniform(0, 0.12, k)), rng.uniform(0, 7, k))))
    # weight about 1e-10: exponent 30 at R.wo = (2 pi 1e-10)^(1/30) = 0.4935
    c30 = (2 * np.pi * 1e-10) ** (1 / 30.0)
    cs = c30 * np.array([0.9, 0.97, 0.999, 1.0, 1.001, 1.03, 1.1])
    up = np.tile([[0, 0, 1.0]], (len(cs), 1))
    wi3 = np.tile(unit([0.0, 0.05, 1.0]), (len(cs), 1))
    R3 = 2 * np.sum(wi3 * up, 1)[:, None] * up - wi3
    b.append(block(M["phong0_1_30"], wi3, up, with_cos(R3, cs, np.full(len(cs), 0.3))))
    th = threshold_values()
    up = np.tile([[0, 0, 1.0]], (len(th), 1))
    steady = np.tile(unit([0.3, 0.4, 0.866]), (len(th), 1))
    for m in ("phong0_0.3_30", "phong1_0.3_30", "phong1_0_1", "phong0_1_200"):
        b.append(block(M[m], axis_dirs(th), up, steady))
        b.append(block(M[m], steady, up, axis_dirs(th)))
    for m in ("phong_dim_1e-13", "phong_dim_3e-10"):
        k = 40
        nn = normal_pool(rng, k, 0.0)
        w4 = with_cos(nn, rng.uniform(0.2, 1.0, k), rng.uniform(0, 7, k))
        b.append(block(M[m], w4, nn, _around(2 * np.sum(w4 * nn, 1)[:, None] * nn - w4, rng, k, 0.8)))
    return sr.OP_EVALUATE, *join(b)


def edge_phong_sample():
    rng = np.random.default_rng(104)
    n = 3200
    ph = mats_like("phong")
    nrm = normal_pool(rng, n)
    mat = rng.choice(ph, n)
    rnd = uniforms(rng, n)
    rnd[:, 1] = np.where(rng.random(n) < 0.05, F32(1.0), rnd[:, 1])  # rnd.y = 1: the lobe's axis itself
    kw = MATERIALS[mat, 28]
    hit = rng.random(n) < 0.15
    rnd[hit, 0] = np.minimum(kw[hit], ONE_M)  # rnd.x == KsWeight exactly: the lobe choice's own edge
    wi = with_cos(nrm, side_cos(rng, n, 0.05), rng.uniform(0, 7, n))
    graze = rng.random(n) < 0.15  # grazing wi: the specular lobe then reaches below the surface
    wi[graze] = with_cos(nrm[graze], rng.uniform(0.02, 0.2, graze.sum()), rng.uniform(0, 7, graze.sum()))
    b = [block(mat, wi, nrm, rnd=rnd, st=rng.uniform(-2, 2, (n, 2)))]
    th = threshold_values()
    up = np.tile([[0, 0, 1.0]], (len(th), 1))
    for m in ("phong0_0.3_30", "phong1_0.3_30", "phong1_0_1"):
        b.append(block(M[m], axis_dirs(th), up, rnd=(0.25, 0.5)))
    for m in ("phong_dim_1e-13", "phong_dim_3e-10"):
        k = 40
        nn = normal_pool(rng, k, 0.0)
        b.append(block(M[m], with_cos(nn, rng.uniform(0.2, 1.0, k), rng.uniform(0, 7, k)), nn, rnd=uniforms(rng, k, 0.0)))
    return sr.OP_SAMPLE, *join(b)


def _micro_pairs(rng, n, mat, tmax, cos_lo, nrm):
    """(wi, wo, ok) built from a micro-normal: H at tan / alpha <= tmax around nrm, wi with |cos| >= cos_lo to nrm and to H on one side, wo the mirror
    image of wi about H or its refraction through H (Snell with the material's eta, from wi's side), in float64"""
    ea = MATERIALS[mat, 21].astype(np.float64)
    alpha = np.where(MATERIALS[mat].view(np.int32)[:, 20] >= 0, 0.3, ea)
    eta = MATERIALS[mat, 26].astype(np.float64)
    H = with_cos(nrm, 1 / np.sqrt(1 + (alpha * rng.uniform(0, tmax, n)) ** 2), rng.uniform(0, 7, n))
    wi = with_cos(H, side_cos(rng, n, cos_lo), rng.uniform(0, 7, n))
    ci = np.sum(wi * H, 1)
    refl = rng.random(n) < 0.5
    e = np.where(ci > 0, 1 / eta, eta)  # sin_t = e sin_i
    ct2 = 1 - (1 - ci * ci) * e * e
    ct = np.sqrt(np.maximum(ct2, 0))
    wo_t = -e[:, None] * wi + (e * ci - np.sign(ci) * ct)[:, None] * H
    wo = np.where(refl[:, None], 2 * ci[:, None] * H - wi, wo_t)
    ok = (refl | (ct2 > 0.01)) & (np.sum(wi * nrm, 1) * ci > 0) & (np.abs(np.sum(wi * nrm, 1)) >= cos_lo) & (np.abs(np.sum(wo * nrm, 1)) >= cos_lo)
    return wi, unit(wo), ok


def edge_dielectric_evaluate():
    rng = np.random.default_rng(105)
    di = mats_like("diel")
    n = 3000
    mat = rng.choice(di, n)
    nrm = normal_pool(rng, n)
    wi, wo, ok = _micro_pairs(rng, n, mat, 4.0, 0.04, nrm)
    ok |= rng.random(n) < 0.3  # mostly pairs that reach the end of the function; some that graze, or whose refraction does not exist
    b = [block(mat[ok], wi[ok], nrm[ok], wo[ok], st=rng.uniform(-2, 2, (int(ok.sum()), 2)), adjoint=rng.integers(0, 2, int(ok.sum())))]
    k = 450  # anywhere: most of these leave at a sign test, a vanishing D or prob
    mat = rng.choice(di, k)
    nrm = normal_pool(rng, k)
    b.append(block(mat, rand_unit(rng, k), nrm, rand_unit(rng, k), adjoint=rng.integers(0, 2, k)))
    k = 200  # D underflowing: micro-normals at tan / alpha of 11 .. 30
    mat = rng.choice(np.concatenate([mats_like("diel_1.5000_0.03"), mats_like("diel_1.5000_0.001"), mats_like("diel_0.6667_0.03")]), k)
    nrm = normal_pool(rng, k, 0.0)
    ea = MATERIALS[mat, 21].astype(np.float64)
    H = with_cos(nrm, 1 / np.sqrt(1 + (ea * rng.uniform(11, 30, k)) ** 2), rng.uniform(0, 7, k))
    w5 = with_cos(H, rng.uniform(0.3, 0.9, k) * rng.choice([-1, 1], k), rng.uniform(0, 7, k))
    b.append(block(mat, w5, nrm, 2 * np.sum(w5 * H, 1)[:, None] * H - w5))
    k = 120  # wo = Reflect(wi, n) exactly (H = n), and wi = n (tan = 0 in G1)
    mat = rng.choice(di, k)
    nrm = normal_pool(rng, k, 0.5)
    w6 = with_cos(nrm, side_cos(rng, k, 0.05), rng.uniform(0, 7, k))
    n32, w32 = nrm.astype(F32), w6.astype(F32)
    mirror = (F32(2) * np.sum(w32 * n32, 1, dtype=F32))[:, None] * n32 - w32  # in float32, as the device's Reflect rounds it
    b.append(block(mat, w6, nrm, mirror))
    b.append(block(mat, nrm, nrm, nrm))
    th = threshold_values()
    up = np.tile([[0, 0, 1.0]], (len(th), 1))
    steady = np.tile(unit([0.3, 0.4, 0.866]), (len(th), 1))
    for m in ("diel_1.5000_0.3", "diel_0.6667_1"):
        b.append(block(M[m], axis_dirs(th), up, steady))
        b.append(block(M[m], steady, up, axis_dirs(th)))
    return sr.OP_EVALUATE, *join(b)


def edge_dielectric_sample():
    rng = np.random.default_rng(106)
    di = mats_like("diel")
    n = 3300
    mat = rng.choice(di, n)
    nrm = normal_pool(rng, n)
    wi = with_cos(nrm, side_cos(rng, n, 0.04), rng.uniform(0, 7, n))
    rnd = uniforms(rng, n)
    close = rng.random(n) < 0.08  # rnd.x so close to 1 that the 1e-6 clamp inside the logarithm acts
    rnd[close, 0] = (1 - rng.choice([3e-7, 6e-8, 1e-6, 2e-6], close.sum())).astype(F32)
    u = np.minimum(rng.random(n).astype(F32), ONE_M)
    k = rng.random(n) < 0.07
    u[k] = rng.choice(np.array([0.0, float(ONE_M)], F32), k.sum())
    ints, cin = block(mat, wi, nrm, rnd=rnd, u=u, st=rng.uniform(-2, 2, (n, 2)), adjoint=rng.integers(0, 2, n))
    # uDiscrete at F itself: the float32 Fresnel value of the case as the host build's reference in float32 computes it
    F = _fresnel_of_sample(ints, cin)
    at = rng.random(n) < 0.02
    cin[at, sr.IN_U] = np.minimum(F[at], ONE_M)
    b = [(ints, cin)]
    k = 300  # total internal reflection: from inside (the side where the relative index is below 1), grazing
    nn = normal_pool(rng, k, 0.0)
    inside = rng.choice(np.concatenate([mats_like("diel_1.5000"), mats_like("diel_0.6667")]), k)
    sgn = np.where(MATERIALS[inside, 26] > 1, -1.0, 1.0)
    b.append(block(inside, with_cos(nn, sgn * rng.uniform(0.05, 0.7, k), rng.uniform(0, 7, k)), nn, rnd=uniforms(rng, k), u=np.minimum(rng.random(k).astype(F32), ONE_M)))
    th = threshold_values()
    up = np.tile([[0, 0, 1.0]], (len(th), 1))
    for m in ("diel_1.5000_0.3", "diel_0.6667_1"):
        b.append(block(M[m], axis_dirs(th), up, rnd=(0.25, 0.5), u=0.01))
    return sr.OP_SAMPLE, *join(b)


def _fresnel_of_sample(ints, cin):
    """F of RoughDielectricSample's micro-normal for the cases, from the reference in float32 (a construction aid: puts uDiscrete next to F)"""
    T = np.float32
    C = sr._Case(MATERIALS, sr.Textures(BITMAP_WH, BITMAP_GAMMA, TEXELS), np.asarray(ints, np.int64), cin, T)
    k = C.K.k
    cos_wi = sr.dot(C.wi, C.nrm)
    alp = C.texture("expOrAlpha")[:, 0]
    local_h, _ = sr.sample_micronormal(C.rnd, alp * (k(1.2) - k(0.2) * np.sqrt(np.abs(cos_wi))), C.K)
    b0, b1, _ = sr.coordinate_system(C.nrm, C.K)
    F, _, _ = sr.fresnel(sr.dot(C.wi, sr.to_world(local_h, b0, b1, C.nrm)), C.eta, C.invEta, C.K)
    return np.nan_to_num(F.astype(F32), nan=0.5)


def _tex_block(mat, slot, st):
    n = len(st)
    z = np.tile([[0, 0, 1.0]], (n, 1))
    return block(mat, z, z, st=st, slot=slot)


def edge_textures():
    rng = np.random.default_rng(107)
    carriers = [M["tex_a"], M["tex_b"], M["tex_c"]]
    b = []
    n = 1500
    b.append(_tex_block(rng.choice(carriers, n), rng.integers(0, 4, n), rng.uniform(-5, 5, (n, 2))))
    for mat in carriers:
        for slot in range(4):
            o = 2 + 6 * slot
            bm = int(MATERIALS[mat].view(np.int32)[o])
            if bm < 0:
                b.append(_tex_block(mat, slot, rng.uniform(-5, 5, (4, 2))))
                continue
            W, H = (int(x) for x in BITMAP_WH[bm])
            s, t = float(MATERIALS[mat, o + 4]), float(MATERIALS[mat, o + 5])
            # texel centres and the wrap seam, over three periods either side of 0
            xs = np.concatenate([(np.arange(-3 * W, 3 * W) + 0.5) / (W * s), np.arange(-3, 4) / s])
            ys = np.concatenate([(np.arange(-3 * H, 3 * H) + 0.5) / (H * t), np.arange(-3, 4) / t])
            g = np.stack(np.meshgrid(xs, ys, indexing="ij"), -1).reshape(-1, 2)
            b.append(_tex_block(mat, slot, g[rng.choice(len(g), min(len(g), 60), replace=False)]))
            # |s st W| about 2^30 (where the 32-bit remainder hands over to the 64-bit one) and far beyond, up to 2^61
            big = np.concatenate([2.0**30 * np.array([1 - 3e-7, 1 - 1e-7, 1.0, 1 + 1e-7, 1 + 3e-7, 0.5, 2.0]), 2.0 ** np.array([31.0, 33.5, 40.0, 52.0, 61.0])])
            for sign in (1.0, -1.0):
                b.append(_tex_block(mat, slot, np.stack([sign * big / (abs(s) * W), np.full(len(big), 0.37)], 1)))
                b.append(_tex_block(mat, slot, np.stack([np.full(len(big), -0.61), sign * big / (abs(t) * H)], 1)))
    return sr.OP_TEX, *join(b)


# ------------------------------------------------------------------------------------------------ conditioned set
def _keep_decisive(op, ints, cin, n, want=None):
    """the first n candidates on which the float64 reference is decisive (and, for most, does something: `want`)"""
    res = reference(op, 1, ints, cin)
    keep = sr.decisive(res, cos_margin=0.05)
    if want is not None:
        keep &= want(res)
    idx = np.flatnonzero(keep)[:n]
    assert len(idx) == n, "the construction yields %d decisive cases of the %d asked for" % (len(idx), n)
    return op, np.ascontiguousarray(ints[idx]), np.ascontiguousarray(cin[idx])


def _cond_normals(rng, n):
    nrm = rand_unit(rng, n)
    nrm[:, 2] = np.where(nrm[:, 2] < -0.85, -nrm[:, 2], nrm[:, 2])
    return nrm


def _cond_phong_mats():
    return np.array([i for name, i in MATERIAL_INDEX.items() if name.startswith("phong") and not name.startswith("phong_dim") and not name.endswith("10000")], np.int64)


def cond_lambert_evaluate():
    rng = np.random.default_rng(201)
    n = 3000
    nrm = _cond_normals(rng, n)
    ints, cin = block(rng.choice(mats_like("lam"), n), with_cos(nrm, side_cos(rng, n, 0.06), rng.uniform(0, 7, n)), nrm, with_cos(nrm, side_cos(rng, n, 0.06), rng.uniform(0, 7, n)),
                      st=rng.uniform(-3, 3, (n, 2)))
    return _keep_decisive(sr.OP_EVALUATE, ints, cin, 2048)


def cond_lambert_sample():
    rng = np.random.default_rng(202)
    n = 3000
    nrm = _cond_normals(rng, n)
    rnd = rng.random((n, 2)).astype(F32)
    rnd[:, 1] = np.maximum(rnd[:, 1], F32(0.004))  # cosWo = sqrt(rnd.y) >= 0.06
    ints, cin = block(rng.choice(mats_like("lam"), n), with_cos(nrm, side_cos(rng, n, 0.06), rng.uniform(0, 7, n)), nrm, rnd=rnd, st=rng.uniform(-3, 3, (n, 2)))
    return _keep_decisive(sr.OP_SAMPLE, ints, cin, 2048)


def cond_phong_evaluate():
    rng = np.random.default_rng(203)
    n = 6000
    nrm = _cond_normals(rng, n)
    wi = with_cos(nrm, side_cos(rng, n, 0.06), rng.uniform(0, 7, n))
    facing = nrm * np.sign(np.sum(wi * nrm, 1))[:, None]
    wo = _around(2 * np.sum(wi * facing, 1)[:, None] * facing - wi, rng, n, 0.5)
    ints, cin = block(rng.choice(_cond_phong_mats(), n), wi, nrm, wo, st=rng.uniform(-3, 3, (n, 2)))
    return _keep_decisive(sr.OP_EVALUATE, ints, cin, 3072)


def cond_phong_sample():
    rng = np.random.default_rng(204)
    n = 6000
    nrm = _cond_normals(rng, n)
    mat = rng.choice(_cond_phong_mats(), n)
    rnd = rng.random((n, 2)).astype(F32)
    rnd[:, 1] = np.maximum(rnd[:, 1], F32(0.004))
    hit = rng.random(n) < 0.1
    rnd[hit, 0] = np.minimum(MATERIALS[mat, 28][hit], ONE_M)  # rnd.x == KsWeight: the lobe choice must fall the same way
    ints, cin = block(mat, with_cos(nrm, side_cos(rng, n, 0.06), rng.uniform(0, 7, n)), nrm, rnd=rnd, st=rng.uniform(-3, 3, (n, 2)))
    res = reference(sr.OP_SAMPLE, 1, ints, cin)
    C = sr._Case(MATERIALS, sr.Textures(BITMAP_WH, BITMAP_GAMMA, TEXELS), ints.astype(np.int64), cin, np.float64)
    facing = C.nrm * np.sign(sr.dot(C.wi, C.nrm))[:, None]
    lobe = sr.dot(sr.reflect(C.wi, facing), res["out"][:, 0:3]) >= 0.5  # R.wo >= 0.5 for the sampled direction
    return _keep_decisive(sr.OP_SAMPLE, ints, cin, 3072, want=lambda r: lobe | ~r["ok"])


def _cond_diel_mats():
    """alpha 0.03, 0.3, 1 and textured at eta 1.5 and 1 / 1.5.  Left to the edge set: alpha 1e-3 (the micro-normal's tangent components are differences of
    nearly equal numbers) and eta 1.0001 (the generalised half vector wi + eta wo and the denominator wi.h + eta wo.h cancel to 1e-4 of their terms)"""
    return np.array([i for name, i in MATERIAL_INDEX.items() if name.startswith("diel") and not name.endswith("_0.001") and not name.startswith("diel_1.0001")], np.int64)


def cond_dielectric_evaluate():
    rng = np.random.default_rng(205)
    n = 12000
    mat = rng.choice(_cond_diel_mats(), n)
    nrm = _cond_normals(rng, n)
    wi, wo, ok = _micro_pairs(rng, n, mat, 2.0, 0.06, nrm)
    ints, cin = block(mat[ok], wi[ok], nrm[ok], wo[ok], st=rng.uniform(-3, 3, (int(ok.sum()), 2)), adjoint=rng.integers(0, 2, int(ok.sum())))
    return _keep_decisive(sr.OP_EVALUATE, ints, cin, 3072, want=lambda r: r["out"][:, 7] > 0)


def cond_dielectric_sample():
    rng = np.random.default_rng(206)
    n = 12000
    mat = rng.choice(_cond_diel_mats(), n)
    nrm = _cond_normals(rng, n)
    rnd = rng.random((n, 2)).astype(F32)
    rnd[:, 0] *= F32(1 - np.exp(-4.0))  # tan^2 / alpha^2 = -log(1 - rnd.x) <= 4
    ints, cin = block(mat, with_cos(nrm, side_cos(rng, n, 0.06), rng.uniform(0, 7, n)), nrm, rnd=rnd, u=np.minimum(rng.random(n).astype(F32), ONE_M),
                      st=rng.uniform(-3, 3, (n, 2)), adjoint=rng.integers(0, 2, n))
    return _keep_decisive(sr.OP_SAMPLE, ints, cin, 3072, want=lambda r: r["ok"] | (np.arange(n) % 8 == 0))


def cond_textures():
    rng = np.random.default_rng(207)
    rows = [(mat, slot) for mat in (M["tex_a"], M["tex_b"], M["tex_c"]) for slot in range(4) if int(MATERIALS[mat].view(np.int32)[2 + 6 * slot]) in GAMMA1_BITMAPS]
    n = 2048
    pick = rng.integers(0, len(rows), n)
    st = rng.uniform(-1, 1, (n, 2)) * 64
    for i, (mat, slot) in enumerate(rows):  # |st| < 64 is the bound on the look-up's own coordinate: scale it out
        o = 2 + 6 * slot
        st[pick == i] /= np.abs(MATERIALS[mat, o + 4 : o + 6]).astype(np.float64)
    return sr.OP_TEX, *_tex_block(np.array([rows[i][0] for i in pick]), np.array([rows[i][1] for i in pick]), st)


EDGE = dict(edge_lambert_evaluate=edge_lambert_evaluate, edge_lambert_sample=edge_lambert_sample, edge_phong_evaluate=edge_phong_evaluate, edge_phong_sample=edge_phong_sample,
            edge_dielectric_evaluate=edge_dielectric_evaluate, edge_dielectric_sample=edge_dielectric_sample, edge_textures=edge_textures)
COND = dict(cond_lambert_evaluate=cond_lambert_evaluate, cond_lambert_sample=cond_lambert_sample, cond_phong_evaluate=cond_phong_evaluate, cond_phong_sample=cond_phong_sample,
            cond_dielectric_evaluate=cond_dielectric_evaluate, cond_dielectric_sample=cond_dielectric_sample, cond_textures=cond_textures)
FAMILIES = tuple(EDGE) + tuple(COND)
MAX_LEFT_OUT = 0.05  # of an edge family; a conditioned family leaves out none


@functools.lru_cache(None)
def family(name):
    """(op, case_ints, case_in), built once"""
    op, ints, cin = (EDGE.get(name) or COND[name])()
    ints.setflags(write=False), cin.setflags(write=False)
    return op, ints, cin


@functools.lru_cache(None)
def family_reference(name, glossy=1):
    """the float64 reference of a family, computed once and shared"""
    op, ints, cin = family(name)
    return reference(op, glossy, ints, cin)


# ------------------------------------------------------------------------------------------------ comparisons
def pattern(ok, out):
    """what the decisions of a function show of themselves: the boolean and which of contrib / pdf / revPdf are zero"""
    return np.concatenate([np.asarray(ok).astype(bool)[:, None], np.asarray(out)[:, 3:6] != 0, np.asarray(out)[:, 7:9] != 0], 1)


def check_decisions(name, ok, out, ref=None):
    """Where the reference is decisive the implementation returns its boolean and its zero / non-zero pattern.  -> share of cases left out"""
    ref = ref or family_reference(name)
    dec = sr.decisive(ref)
    left_out = 1.0 - dec.mean()
    assert left_out <= (MAX_LEFT_OUT if name.startswith("edge") else 0.0), "%s: %.1f %% of the cases are too close to a threshold to be asserted" % (name, 100 * left_out)
    same = (pattern(ok, out) == pattern(ref["ok"], ref["out"])).all(1)
    bad = np.flatnonzero(dec & ~same)
    assert len(bad) == 0, "%s: %d decisive cases fall the other way, first %d: got %s %s, reference %s %s" % (
        name, len(bad), bad[0], ok[bad[0]], out[bad[0]], ref["ok"][bad[0]], ref["out"][bad[0]])
    return left_out


def check_untouched(name, out, cin, ref=None):
    """Where the reference is decisive, a word the operation does not write keeps the bits that went in"""
    ref = ref or family_reference(name)
    dec = sr.decisive(ref)
    went_in = np.concatenate([cin[:, sr.IN_WO], cin[:, sr.IN_CON], cin[:, [sr.IN_COS, sr.IN_PDF, sr.IN_REV]]], 1)
    keep = dec[:, None] & ~ref["written"]
    assert keep.any() or family(name)[0] == sr.OP_TEX or "evaluate" in name
    bad = keep & (np.ascontiguousarray(out).view(np.uint32) != np.ascontiguousarray(went_in).view(np.uint32))
    assert not bad.any(), "%s: case %d: a word the operation leaves alone changed: %s -> %s" % (name, np.argwhere(bad)[0][0], went_in[np.argwhere(bad)[0][0]], out[np.argwhere(bad)[0][0]])
    return int(keep.sum())


def deviations(name, ok, out, ref=None):
    """largest rel_dev per quantity over the cases both sides take the same way (same boolean; on a false return only what both wrote)"""
    ref = ref or family_reference(name)
    same = (pattern(ok, out) == pattern(ref["ok"], ref["out"])).all(1)
    masked = np.where(ref["written"], out, ref["out"])
    d = sr.rel_dev(masked, ref["out"])
    return {q: float(d[same, j].max()) for j, q in enumerate(sr.QUANTITIES)}, float(same.mean())


def check_bars(name, ok, out):
    dev, same = deviations(name, ok, out)
    assert same == 1.0, "%s: %.2f %% of the conditioned cases fall another way than the reference" % (name, 100 * (1 - same))
    bars = sr.bars(name)
    print("%s: deviation from the float64 reference %s" % (name, {q: "%.2e (bar %.2e)" % (dev[q], bars[q]) for q in dev}))
    for q in dev:
        assert dev[q] <= bars[q], "%s: %s deviates from the float64 reference by %.3e, bar %.3e" % (name, q, dev[q], bars[q])
    return dev


def measure():
    table = {}
    for name in COND:
        op, ints, cin = family(name)
        r32 = reference(op, 1, ints, cin, dtype=np.float32)
        dev, same = deviations(name, r32["ok"], r32["out"].astype(np.float32))
        table[name] = dev
        print("    %r: {%s},  # same way %.4f" % (name, ", ".join("%r: %.2e" % (q, v) for q, v in dev.items()), same), file=sys.stderr if same < 1 else sys.stdout)
    return table


if __name__ == "__main__":
    if "--measure" in sys.argv:
        measure()
    else:
        for name in FAMILIES:
            op, ints, cin = family(name)
            print(name, op, len(cin), "left out %.3f" % (1 - sr.decisive(family_reference(name)).mean()))
