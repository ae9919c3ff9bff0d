"""GPU tier: the device's texture look-up and BSDFs (lmc_shade_probe: device/dshade.h in a small kernel of its own, one case per lane) on the cases of
tests/shade_cases.py.
  * against the host build of the same source (tests/helpers/dshade_host.cpp): EVERY output word of every case of both sets bit-equal (NaN = NaN, as
    in the trigonometry test).  This is the contract the chain-parity tests rely on, stated per function and over the whole parameter space.
  * against the float64 reference (tests/shade_ref.py): the bars and the decision rule of the CPU tier (tests/test_shade_cases.py), so this file stands alone.
  * the Lambertian-only instantiation, the launch shapes, the sentinels beyond n, repeatability.
The probe runs the source in a small kernel; code generation inside the large step kernels stays the chain-parity tests' business."""
import numpy as np
import pytest

from tests import shade_cases as sc
from tests import shade_ref as sr

pytestmark = pytest.mark.gpu


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def _assert_same(name, dev, host, cin=None):
    (dok, dout), (hok, hout) = dev, host
    same = _same_bits(dout, hout).all(1) & (dok == hok)
    if not same.all():
        i = int(np.flatnonzero(~same)[0])
        raise AssertionError("%s: %d of %d cases differ from the host build, first %d: device %s %s, host %s %s%s" % (
            name, int((~same).sum()), len(same), i, dok[i], dout[i], hok[i], hout[i], "" if cin is None else ", inputs %s" % (cin[i],)))


@pytest.mark.parametrize("name", list(sc.FAMILIES))
def test_device_gives_the_bits_of_the_host_build(name):
    op, ints, cin = sc.family(name)
    _assert_same(name, sc.device_shade(op, 1, ints, cin), sc.host_shade(op, 1, ints, cin), cin)


@pytest.mark.parametrize("name", list(sc.FAMILIES))
def test_device_against_the_reference(name):
    op, ints, cin = sc.family(name)
    ok, out = sc.device_shade(op, 1, ints, cin)
    left_out = sc.check_decisions(name, ok, out)
    sc.check_untouched(name, out, cin)
    if name in sc.COND:
        assert left_out == 0.0
        sc.check_bars(name, ok, out)


def test_lambertian_only_instantiation():
    """G = 0: bit-equal to G = 1 on Lambertian records; on Phong and dielectric records bit-equal to the Lambertian functions on the same Kd and twoSided"""
    as_lambert = sc.MATERIALS.copy()
    as_lambert.view(np.int32)[:, 0] = sr.LAMBERTIAN
    for name in ("edge_lambert_evaluate", "edge_lambert_sample", "edge_phong_evaluate", "edge_phong_sample", "edge_dielectric_evaluate", "edge_dielectric_sample", "edge_textures"):
        op, ints, cin = sc.family(name)
        g0 = sc.device_shade(op, 0, ints, cin)
        _assert_same(name + " (G = 0 against G = 1 on Lambertian copies of the records)", g0, sc.device_shade(op, 1, ints, cin, materials=as_lambert))
        _assert_same(name + " (G = 0)", g0, sc.host_shade(op, 0, ints, cin))
        if "lambert" in name or "textures" in name:
            _assert_same(name + " (G = 0 against G = 1)", g0, sc.device_shade(op, 1, ints, cin))


def _mixed(op, n):
    """n cases of one operation drawn from every family that has it, interleaved (so that a wave holds all three BSDFs)"""
    fams = [sc.family(name) for name in sc.FAMILIES if sc.family(name)[0] == op]
    ints, cin = np.concatenate([f[1] for f in fams]), np.concatenate([f[2] for f in fams])
    pick = np.random.default_rng(31 + op).permutation(len(cin))[:n]
    assert len(pick) == n
    return np.ascontiguousarray(ints[pick]), np.ascontiguousarray(cin[pick])


@pytest.mark.parametrize("op", [sr.OP_TEX, sr.OP_EVALUATE, sr.OP_SAMPLE])
def test_launch_shapes_sentinels_and_repeatability(op):
    ints, cin = _mixed(op, 4096)
    full = sc.device_shade(op, 1, ints, cin)
    _assert_same("mixed, n = 4096", full, sc.host_shade(op, 1, ints, cin), cin)
    again = sc.device_shade(op, 1, ints, cin)
    assert np.array_equal(full[0], again[0]) and np.array_equal(full[1].view(np.uint32), again[1].view(np.uint32)), "a second call gives other bits"
    for n in (1, 63, 64, 65):
        rows = n + 70  # the grid's idle lanes (up to the next multiple of 64) and a block beyond them
        ok, out = sc.device_shade(op, 1, ints, cin, n=n, n_rows=rows)
        assert np.array_equal(ok[:n], full[0][:n]) and np.array_equal(out[:n].view(np.uint32), full[1][:n].view(np.uint32)), n
        assert (ok[n:] == sc.SENTINEL).all() and (out[n:].view(np.uint32) == sc.UNTOUCHED_BITS).all(), "n = %d: a lane beyond n wrote" % n
        written = out[:n].view(np.uint32) != sc.UNTOUCHED_BITS
        assert written.all() and (ok[:n] != sc.SENTINEL).all(), "n = %d: a lane below n left a word unwritten" % n
