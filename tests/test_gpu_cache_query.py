"""The lean small step's cache look-up (dsmall.h PrepareGaussianLean + GaussianDim, through lmc_lean_query_probe) on the device, against the oracle's
cache-ready branch of InitGaussianFor (orc_cache_gaussian) on the clouds of tests/cache_cases.py.  Every comparison is bit for bit: both sides use
the same + - * / sqrt without contraction."""
import ctypes

import numpy as np
import pytest

from tests import cache_cases as cc
from tests import gpu_checks as gc
from tests._orc import P

pytestmark = pytest.mark.gpu

FIELDS = ("ints", "w", "chain", "gauss", "generic")
DEFAULT = (4, 1, 1)  # the renderer's configuration: grid rank min(4, dim), the coordinates it would choose, the grid built on the device
_memo = {}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def probe(c, m, chosen, device):
    """lmc_lean_query_probe on a case -> ints nq x 10, w nq x 5, chain nq x 3 x dim, gauss nq x (3 dim + 1), generic nq x 2 x dim (run once per process)"""
    key = (c.name, c.dim, m, chosen, device)
    if key not in _memo:
        lib = gc.pkg().lib()
        nq, dim = c.q.shape
        out = dict(ints=np.full((nq, 10), -7, np.int32), w=np.zeros((nq, 5), np.float32), chain=np.zeros((nq, 3, dim), np.float32),
                   gauss=np.zeros((nq, 3 * dim + 1), np.float32), generic=np.zeros((nq, 2, dim), np.float32))
        r = lib.lmc_lean_query_probe(dim, len(c.pts), P(c.pts), P(c.v1), P(c.v2), ctypes.c_float(cc.MALA_STEPSIZE), ctypes.c_float(cc.MALA_STDDEV), m, chosen,
                                     device, nq, P(c.q), P(c.queried), P(c.last_pss), P(c.ch_v1), P(c.ch_v2), P(c.ss), P(out["ints"]), P(out["w"]),
                                     P(out["chain"]), P(out["gauss"]), P(out["generic"]))
        assert r == 0, lib.lmc_last_error().decode()
        _memo[key] = out
    return _memo[key]


def oracle(c):
    key = (c.name, c.dim, "oracle")
    if key not in _memo:
        _memo[key] = cc.oracle_gaussian(gc.oracle_lib(), c)
    return _memo[key]


# What every case is there to reach, per dimension at least this often (cache_cases.branch_counts; the generator gives, over the four dimensions, at
# least: bulk 52 / 97 / 2636 / 374 / 179 / 166, boundary 1455 / 475 / 0 / 84 / 1068 / 200, lattice3 56 / 266 / 967 / 0 / 1431 / 141, lattice4 131 / 410 /
# 968 / 0 / 1423 / 149, cell_edges 611 / 727 / 1064 / 0 / 411 / 157, one_cell 74 / 89 / 2071 / 0 / 108 / 144)
MIN_COUNTS = {
    "bulk": dict(one=40, few=80, many=2500, empty_cell=300, none_within=150, reuse=140),
    "boundary": dict(one=1400, few=450, empty_cell=70, none_within=1000, reuse=200),
    "lattice3": dict(one=50, few=250, many=900, none_within=1400, reuse=130),
    "lattice4": dict(one=120, few=400, many=900, none_within=1400, reuse=130),
    "cell_edges": dict(one=600, few=700, many=1000, none_within=400, reuse=140),
    "one_cell": dict(one=70, few=80, many=2000, none_within=100, reuse=130),
}


@pytest.mark.parametrize("dim", cc.DIMS)
def test_lean_query_matches_the_oracle_bit_for_bit(dim):
    """Default configuration.  Equal on every query of every cloud: the branch taken, the number of matches, their rows in search order, the blend
    weights, both counters, chain v1 / v2 / last_pss afterwards, the Gaussian of every dimension and logDet.  No case passes vacuously: each
    reaches the branches it was built for."""
    for name, c in cc.cases(dim).items():
        ints, w, chain, gauss = oracle(c)
        got = probe(c, *DEFAULT)
        counts = cc.branch_counts(c, ints)
        for branch, least in MIN_COUNTS.get(name, {}).items():
            assert counts[branch] >= least, (name, branch, counts)
        if name.startswith("small"):
            assert (ints[:, 0] == cc.BRANCH_BLEND).sum() >= 1, name
        assert np.array_equal(got["ints"][:, :9], ints), (name, np.nonzero((got["ints"][:, :9] != ints).any(1))[0][:10])
        assert np.array_equal(bits(got["w"]), bits(w)), name
        assert np.array_equal(bits(got["chain"]), bits(chain)), name
        assert np.array_equal(bits(got["gauss"]), bits(gauss)), name


@pytest.mark.parametrize("dim", cc.DIMS)
def test_every_grid_configuration_gives_the_same_answers(dim):
    """Grid built on the host or on the device, over the leading or the chosen coordinates, rank 3 or 4: all outputs identical to the default's.
    (The device's grid build on clouds no render produces; the existence test's exactness as a device claim.)"""
    for name, c in cc.cases(dim).items():
        ref = probe(c, *DEFAULT)
        for m in (3, 4):
            for chosen in (0, 1):
                for device in (0, 1):
                    got = probe(c, m, chosen, device)
                    for f in FIELDS:
                        assert np.array_equal(bits(got[f]), bits(ref[f])), (name, m, chosen, device, f)


@pytest.mark.parametrize("dim", cc.DIMS)
def test_lean_and_generic_query_agree(dim):
    """The generic kernel's CacheQuery (dchain.h) on the same point: its v1 / v2 equal what the lean blend wrote, and -- for a chain that has not
    queried before -- it hits exactly where the lean look-up blends."""
    hits = 0
    for name, c in cc.cases(dim).items():
        got = probe(c, *DEFAULT)
        mode, hit = got["ints"][:, 0], got["ints"][:, 9] == 1
        fresh = c.queried == 0
        assert np.array_equal(hit[fresh], mode[fresh] == cc.BRANCH_BLEND), name
        blend = mode == cc.BRANCH_BLEND
        assert hit[blend].all(), name
        assert np.array_equal(bits(got["generic"][blend]), bits(got["chain"][blend][:, :2])), name
        assert not got["generic"][~hit].any(), name
        hits += int(blend.sum())
    assert hits > 5000


@pytest.mark.parametrize("dim", cc.DIMS)
def test_reuse_exactly_where_the_oracle_reuses(dim):
    """The chains of the boundary case whose last_pss was bisected to the re-use radius around their query (F_QUERIED set): VS_REUSE exactly where the
    oracle re-uses, and a re-using chain keeps its v1 / v2 / last_pss and both counters."""
    c = cc.cases(dim)["boundary"]
    ints = oracle(c)[0]
    got = probe(c, *DEFAULT)
    tail = np.arange(len(c.q)) >= len(c.q) - 400  # 200 chains just inside the re-use radius, then the same 200 queries just outside it
    assert c.queried[tail].all()
    reuse = ints[:, 0] == cc.BRANCH_REUSE
    assert reuse[tail][:200].all() and not reuse[tail][200:].any()
    assert np.array_equal(got["ints"][:, 0] == cc.BRANCH_REUSE, reuse)
    before = np.stack([c.ch_v1, c.ch_v2, c.last_pss], 1)
    assert np.array_equal(bits(got["chain"][reuse]), bits(before[reuse]))
    assert not got["ints"][reuse, 7:9].any()
    assert (got["ints"][~reuse, 7] == 1).all()
