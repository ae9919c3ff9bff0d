"""CPU tier of the shading tests: the float64 reference of the BSDFs and the texture look-up (tests/shade_ref.py) shown sound on its own, and the host
build of the device's source (tests/helpers/dshade_host.cpp: device/dshade.h compiled by g++ with the product's arithmetic contract) held against it on
the cases of tests/shade_cases.py -- tolerance bars on the conditioned set, decision agreement and untouched words on both sets.  The device runs the
same cases in tests/test_gpu_shade.py, where it must give the host build's bits."""
import numpy as np
import pytest

from tests import shade_cases as sc
from tests import shade_ref as sr

PROPERTY_BAR = 1e-9  # float64 rounding through a few dozen operations and one exponential whose argument is below 40


def _exact(name):
    """a conditioned family with wi and the normal re-normalised in float64 and nothing in the in / out words: the identities below hold for unit vectors"""
    op, ints, cin = sc.family(name)
    c = cin.astype(np.float64)
    c[:, sr.IN_WI], c[:, sr.IN_N], c[:, sr.IN_WO] = sc.unit(c[:, sr.IN_WI]), sc.unit(c[:, sr.IN_N]), sc.unit(c[:, sr.IN_WO])
    c[:, 14:20] = 0
    if "dielectric" in name:  # ... and for a boundary whose two relative indices are exact reciprocals
        ints = ints.copy()
        ints[:, 0] = np.random.default_rng(5).choice(sc.mats_like("exact_"), len(ints))
    return op, ints, c


def _close(a, b, what):
    d = sr.rel_dev(a, b).max(0)
    assert (d <= PROPERTY_BAR).all(), (what, dict(zip(sr.QUANTITIES, d)))


@pytest.mark.parametrize("bsdf", ["lambert", "phong", "dielectric"])
def test_reference_sample_is_evaluate_at_the_sampled_direction(bsdf):
    """contrib * pdf of Sample is Evaluate's contrib at the sampled wo; pdf, revPdf and cosWo are Evaluate's"""
    _, ints, c = _exact("cond_%s_sample" % bsdf)
    s = sc.reference(sr.OP_SAMPLE, 1, ints, c)
    ok = s["ok"]
    assert ok.mean() > 0.5
    c2 = c.copy()
    c2[:, sr.IN_WO] = s["out"][:, 0:3]
    e = sc.reference(sr.OP_EVALUATE, 1, ints, c2)
    got = s["out"].copy()
    got[:, 3:6] *= got[:, 7:8]
    _close(got[ok], e["out"][ok], bsdf)
    assert (e["out"][ok, 7] > 0).all()


@pytest.mark.parametrize("bsdf", ["lambert", "phong", "dielectric"])
def test_reference_reverse_pdf_is_the_pdf_of_the_reversed_pair(bsdf):
    _, ints, c = _exact("cond_%s_evaluate" % bsdf)
    fwd = sc.reference(sr.OP_EVALUATE, 1, ints, c)
    c2 = c.copy()
    c2[:, sr.IN_WI], c2[:, sr.IN_WO] = c[:, sr.IN_WO], c[:, sr.IN_WI]
    rev = sc.reference(sr.OP_EVALUATE, 1, ints, c2)
    assert (fwd["out"][:, 7] > 0).mean() > 0.25  # (the rest: wi or wo behind a one-sided surface, zero both ways)
    # Evaluate gives up on a direction pair when ITS sampling density underflows (prob < 1e-20), which the reversed pair need not: compared where both are live
    live = (fwd["out"][:, 7] > 0) & (rev["out"][:, 7] > 0)
    assert live.mean() > 0.25
    for a, b in ((fwd, rev), (rev, fwd)):
        d = np.abs(a["out"][live, 8] - b["out"][live, 7]) / np.abs(b["out"][live, 7])
        assert (d <= PROPERTY_BAR).all(), (bsdf, d.max())
    dead = ~live & ((fwd["out"][:, 7] > 0) | (rev["out"][:, 7] > 0))
    assert dead.mean() < 0.02 and max(fwd["out"][dead, 7].max(initial=0), rev["out"][dead, 7].max(initial=0)) < 1e-12


@pytest.mark.parametrize("material", ["lam1", "phong1_0.3_30", "phong0_1_1", "phong0_0_0", "phong1_1_30", "diel_1.5000_0.3", "diel_0.6667_0.3", "diel_1.5000_1", "diel_0.6667_1", "diel_1.5000_tex"])
def test_reference_pdf_integrates_to_at_most_one(material):
    """midpoint quadrature of Evaluate's pdf over the sphere of wo, on parameters rough enough to integrate (alpha >= 0.2, exponent <= 50); what a
    sampler loses below the surface or to a masked micro-normal makes the integral smaller than 1, nothing may make it larger"""
    nt, nphi = 600, 600
    th = (np.arange(nt) + 0.5) * np.pi / nt
    ph = (np.arange(nphi) + 0.5) * 2 * np.pi / nphi
    T, P = np.meshgrid(th, ph, indexing="ij")
    wo = np.stack([np.sin(T) * np.cos(P), np.sin(T) * np.sin(P), np.cos(T)], -1).reshape(-1, 3)
    w = (np.sin(T) * (np.pi / nt) * (2 * np.pi / nphi)).ravel()
    nrm = sc.unit([0.2, -0.3, 0.9])
    for cos_wi in (0.9, 0.35, -0.6):
        wi = sc.with_cos(nrm[None, :], np.array([cos_wi]), np.array([1.0]))[0]
        ints, cin = sc.block(sc.M[material], np.tile(wi, (len(wo), 1)), np.tile(nrm, (len(wo), 1)), wo, st=(0.3, 0.7))
        c = cin.astype(np.float64)
        c[:, sr.IN_WI], c[:, sr.IN_N], c[:, sr.IN_WO] = wi, nrm, wo
        c[:, 14:20] = 0  # (the Lambertian early-out leaves the caller's pdf in place)
        r = sc.reference(sr.OP_EVALUATE, 1, ints, c)
        total = float(np.sum(r["out"][:, 7] * w))
        assert total <= 1 + 1e-3, (material, cos_wi, total)
        if cos_wi > 0 or material == "lam1" or material.startswith("phong1") or material.startswith("diel"):
            assert total > 0.3, (material, cos_wi, total)  # (and it is a density, not a stray zero)


def test_reference_constants_are_the_measurement():
    """shade_ref.MEASURED is what the reference's float32 evaluation deviates from its float64 evaluation by on the committed conditioned cases
    (within a factor of 2: numpy's float32 transcendentals differ by an ulp or two between builds)"""
    table = sc.measure()
    assert set(table) == set(sr.MEASURED) == set(sc.COND)
    for name, row in table.items():
        for q, v in row.items():
            m = sr.MEASURED[name][q]
            assert (v == 0) == (m == 0) and m / 2 <= v <= m * 2, (name, q, v, m)


@pytest.mark.parametrize("name", list(sc.COND))
def test_host_build_against_the_reference_on_the_conditioned_set(name):
    op, ints, cin = sc.family(name)
    ok, out = sc.host_shade(op, 1, ints, cin)
    assert sc.check_decisions(name, ok, out) == 0.0
    sc.check_bars(name, ok, out)


@pytest.mark.parametrize("name", list(sc.FAMILIES))
def test_host_build_decides_as_the_reference_and_leaves_alone_what_it_does(name):
    op, ints, cin = sc.family(name)
    assert 0 < len(cin) <= sc.MAX_FAMILY
    ok, out = sc.host_shade(op, 1, ints, cin)
    sc.check_decisions(name, ok, out)
    kept = sc.check_untouched(name, out, cin)
    if "sample" in name:
        assert kept > 0
    if name == "edge_lambert_evaluate":  # the early-out leaves pdf and revPdf alone
        ref = sc.family_reference(name)
        assert (~ref["written"][:, 7] & sr.decisive(ref)).sum() > 100
    if name == "edge_phong_sample":  # KsWeight == 0: the diffuse lobe's reverse density is added onto what the caller passed in
        kw0 = sc.MATERIALS[ints[:, 0], 28] == 0
        ref = sc.family_reference(name)
        sel = kw0 & ref["ok"] & sr.decisive(ref)
        assert sel.sum() > 50 and (out[sel, 8] > sc.INIT["rev"]).all()
        assert np.abs(out[sel, 8] - ref["out"][sel, 8]).max() < 1e-5


def test_the_sets_are_small_and_finite():
    total = 0
    for name in sc.FAMILIES:
        op, ints, cin = sc.family(name)
        total += len(cin)
        assert np.isfinite(cin).all() and len(cin) <= sc.MAX_FAMILY
    assert total < 100000


def test_lambertian_only_instantiation_on_the_host_build():
    """G = 0 runs the Lambertian functions on any record: the bits of G = 1 on the same records with the type word set to Lambertian"""
    as_lambert = sc.MATERIALS.copy()
    as_lambert.view(np.int32)[:, 0] = sr.LAMBERTIAN
    for name in ("edge_lambert_evaluate", "edge_lambert_sample", "edge_phong_evaluate", "edge_phong_sample", "edge_dielectric_evaluate", "edge_dielectric_sample"):
        op, ints, cin = sc.family(name)
        ok0, out0 = sc.host_shade(op, 0, ints, cin)
        ok1, out1 = sc.host_shade(op, 1, ints, cin, materials=as_lambert)
        assert np.array_equal(ok0, ok1) and np.array_equal(out0.view(np.uint32), out1.view(np.uint32)), name
        if "lambert" in name:
            ok, out = sc.host_shade(op, 1, ints, cin)
            assert np.array_equal(ok0, ok) and np.array_equal(out0.view(np.uint32), out.view(np.uint32)), name
        else:
            sc.check_decisions(name, ok0, out0, ref=sc.reference(op, 0, ints, cin))
