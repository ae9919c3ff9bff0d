"""Seeded point clouds, queries and chain states for the tests of the global-cache look-up (the oracle's CacheReadyGaussian / orc_kd_query on the
CPU, the lean kernel's PrepareGaussianLean + GaussianDim through lmc_lean_query_probe on the GPU).  The CPU and the GPU tests use the same arrays.

Every case is a `Case`: cache rows (pts, v1, v2: npts x dim), queries q (nq x dim) and one chain state per query (queried bit, last_pss, stored
v1 / v2, ssScore).  All coordinates lie in [0, 1]; 0 and 1.0 themselves occur.  The float32 helpers restate the arithmetic of the leaf scan of the
search (and of the lean kernel's candidate loop): differences, squares and the running sum each rounded to float32, summed in coordinate order."""
import collections
import ctypes

import numpy as np

F = np.float32
DIMS = (6, 8, 10, 12)
MALA_STEPSIZE = F(0.005)
MALA_STDDEV = F(0.005)
ONE_BELOW = np.nextafter(F(1), F(0))
BRANCH_ISOTROPIC, BRANCH_REUSE, BRANCH_BLEND = 0, 1, 2

Case = collections.namedtuple("Case", "name dim pts v1 v2 q queried last_pss ch_v1 ch_v2 ss")


def radius_sq(dim):
    """dim * (PSS_QUERY_DIST * PSS_QUERY_DIST) as the float expression evaluates (global_cache.h:99)"""
    return F(dim) * (F(0.01) * F(0.01))


def reuse_radius_sq(dim):
    """dim * (PSS_REUSE_DIST * PSS_REUSE_DIST), mutation_mala.h:139"""
    return F(dim) * (F(0.10) * F(0.10))


def grid_g(dim):
    """cells per axis of the existence grid (dchain.h CacheGridG)"""
    g = int(F(1) / (np.sqrt(F(dim)) * F(0.01)))
    return max(1, min(64, g))


def grid_cell(x, G):
    """dchain.h CacheGridCell"""
    return np.clip((np.asarray(x, F) * F(G)).astype(np.int64), 0, G - 1)


def dist32(a, b):
    """squared distance of the rows of a and b (broadcast) in the leaf scan's arithmetic"""
    a, b = np.asarray(a, F), np.asarray(b, F)
    d = np.zeros(np.broadcast_shapes(a.shape[:-1], b.shape[:-1]), F)
    diff = np.empty_like(d)
    for k in range(a.shape[-1]):
        np.subtract(a[..., k], b[..., k], out=diff)
        np.multiply(diff, diff, out=diff)
        np.add(d, diff, out=d)
    return d


def count32(pts, q, r2, chunk=512):
    """number of rows within the radius of every query (strict), float32 brute force, no tree"""
    out = np.zeros(len(q), np.int64)
    for s in range(0, len(q), chunk):
        out[s : s + chunk] = (dist32(q[s : s + chunk, None, :], pts[None, :, :]) < r2).sum(1)
    return out


def dist64(pts, q, chunk=512):
    """squared distances in float64: (nq, npts)"""
    p64, q64 = pts.astype(np.float64), q.astype(np.float64)
    return np.concatenate([((q64[s : s + chunk, None, :] - p64[None, :, :]) ** 2).sum(2) for s in range(0, len(q), chunk)])


def has_candidates(pts, q, dim, m=4):
    """does the query's own cell of the existence grid over the leading m coordinates list any row (a row lies in the 3^m cells around its own)?"""
    G = grid_g(dim)
    rc, qc = grid_cell(pts[:, :m], G), grid_cell(q[:, :m], G)
    occupied = set()
    for o in range(3**m):
        c, t, key = rc.copy(), o, np.zeros(len(pts), np.int64)
        for k in range(m):
            c[:, k] += t % 3 - 1
            t //= 3
        ok = ((c >= 0) & (c < G)).all(1)
        for k in range(m):
            key = key * G + c[:, k]
        occupied.update(key[ok].tolist())
    key = np.zeros(len(q), np.int64)
    for k in range(m):
        key = key * G + qc[:, k]
    return np.array([int(x) in occupied for x in key])


def _moments(rng, n, dim):
    """v1 normal, v2 positive over eleven decades: M = 1 / (1e-3 + sqrt(v2)) reaches both PCD_MAX (v2 < 8e-5) and PCD_MIN (v2 > 1e4)"""
    return rng.normal(0, 2.0, (n, dim)).astype(F), (10.0 ** rng.uniform(-5.5, 5.5, (n, dim))).astype(F)


def _scores(rng, n):
    """ssScore: 0 and values either side of the 1e-10 threshold among ordinary ones"""
    ss = (10.0 ** rng.uniform(-3, 1, n)).astype(F)
    special = np.array([0.0, 5e-11, np.nextafter(F(1e-10), F(0)), F(1e-10), np.nextafter(F(1e-10), F(1)), 2e-10], F)
    where = rng.random(n) < 0.2
    ss[where] = special[rng.integers(0, len(special), where.sum())]
    return ss


def _finish(name, dim, rng, pts, q, queried=None, last_pss=None):
    pts, q = np.ascontiguousarray(pts, F), np.ascontiguousarray(q, F)
    assert pts.min() >= 0 and pts.max() <= 1 and q.min() >= 0 and q.max() <= 1
    nq = len(q)
    v1, v2 = _moments(rng, len(pts), dim)
    ch_v1, ch_v2 = _moments(rng, nq, dim)
    if queried is None:  # half the chains have queried before, far away or (a few) within the re-use radius
        queried = (rng.random(nq) < 0.5).astype(np.int32)
        last_pss = rng.random((nq, dim)).astype(F)
        near = rng.random(nq) < 0.1
        last_pss[near] = np.clip(q[near] + rng.normal(0, 0.05, (near.sum(), dim)), 0, 1).astype(F)
    return Case(name, dim, pts, v1, v2, q, np.ascontiguousarray(queried, np.int32), np.ascontiguousarray(last_pss, F), ch_v1, ch_v2, _scores(rng, nq))


def _directions(rng, base, n_active):
    """unit directions with n_active[i] non-zero coordinates each, every component pointing to the side of `base` that has room inside [0, 1]"""
    n, dim = base.shape
    u = rng.normal(0, 1, (n, dim))
    u[np.abs(u) < 0.05] = 0.05
    rank = np.argsort(rng.random((n, dim)), 1)
    u[rank >= n_active[:, None]] = 0
    sign = np.where(rng.random((n, dim)) < 0.5, -1.0, 1.0)
    sign = np.where(base > 0.6, -1.0, np.where(base < 0.4, 1.0, sign))
    u = np.abs(u) * sign
    return u / np.sqrt((u * u).sum(1, keepdims=True))


def bisect_to_radius(fixed, base, u, r2, t_max, moving_first=True):
    """The two points base + t u (float32, clipped to [0, 1]) either side of the radius r2 around `fixed`: the first has the largest float32
    distance below r2 that bisection over t finds, the second the smallest at or above it.  moving_first: the distance is summed as
    (moving - fixed), the query minus the row; else as (fixed - moving), pss minus last_pss."""
    base64, lo, hi = base.astype(np.float64), np.zeros(len(base)), np.full(len(base), float(t_max))

    def point(t):
        return np.clip(base64 + t[:, None] * u, 0, 1).astype(F)

    def d(t):
        return dist32(point(t), fixed) if moving_first else dist32(fixed, point(t))

    assert (d(lo) < r2).all() and (d(hi) >= r2).all()
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        inside = d(mid) < r2
        lo, hi = np.where(inside, mid, lo), np.where(inside, hi, mid)
    dist = (lambda p: dist32(p, fixed)) if moving_first else (lambda p: dist32(fixed, p))
    p_in, p_out = point(lo), point(hi)
    # single coordinates one float further: away from `base` while the point stays inside the radius, towards it while it stays outside
    for p, away, keep in ((p_in, True, lambda x: dist(x) < r2), (p_out, False, lambda x: dist(x) >= r2)):
        for _ in range(3):
            for k in range(p.shape[1]):
                t = p.copy()
                target = np.where((u[:, k] > 0) == away, F(2), F(-1)).astype(F)
                t[:, k] = np.nextafter(p[:, k], target)
                ok = (u[:, k] != 0) & (t[:, k] >= 0) & (t[:, k] <= 1) & keep(t)
                p[ok, k] = t[ok, k]
    assert (dist(p_in) < r2).all() and (dist(p_out) >= r2).all()
    return p_in, p_out


def exact_radius_offsets(r2, base_d=F(0)):
    """every float32 x near sqrt(r2 - base_d) with fl(base_d + fl(x * x)) == r2: a coordinate difference that puts a distance ON the radius"""
    x0 = F(np.sqrt(np.float64(r2) - np.float64(base_d)))
    xs = (x0.view(np.uint32) + np.arange(-512, 513)).astype(np.uint32).view(F)
    return xs[(F(base_d) + xs * xs) == r2]


def _with_bounds(rng, a, frac=0.02):
    """a few coordinates moved onto the bounds 0, 1.0 and the float below 1"""
    a = a.copy()
    pick = rng.random(a.shape) < frac
    a[pick] = rng.choice(np.array([0, 1, ONE_BELOW], F), pick.sum())
    return a


def bulk(dim, seed=0):
    """the kd_case clusters (tests/test_oracle_pins.py), queries near the clusters at several spreads and uniform ones"""
    from tests.test_oracle_pins import kd_case

    rng = np.random.default_rng(1000 + 10 * dim + seed)
    pts, q0, _ = kd_case(dim)
    centers = np.random.default_rng(dim).random((40, dim)).astype(F)  # kd_case's first draw
    parts = [q0]
    for sigma, n in ((0.004, 500), (0.008, 700), (0.0095, 900), (0.011, 600)):
        parts.append(centers[rng.integers(0, 40, n)] + rng.normal(0, sigma, (n, dim)))
    parts.append(rng.random((300, dim)))
    return _finish("bulk", dim, rng, np.clip(pts, 0, 1), np.clip(np.concatenate(parts), 0, 1))


def boundary(dim, seed=0, npts=3000, nitems=1500, nre=200):
    """Uniform rows, a third of them in tight groups of two to four.  Queries bisected to the query radius around a row along directions that are
    non-zero in 1, 2, 3 or all coordinates; queries whose distance to a row EQUALS the radius (a miss: the comparison is strict); and chains whose
    last_pss is bisected to the re-use radius around their query."""
    rng = np.random.default_rng(2000 + 10 * dim + 1000 * seed)
    r2, rr2 = radius_sq(dim), reuse_radius_sq(dim)
    pts = _with_bounds(rng, rng.random((npts, dim)).astype(F))
    ngroup = npts // 3
    src = rng.integers(ngroup, npts, ngroup)
    pts[:ngroup] = np.clip(pts[src] + rng.normal(0, 0.002, (ngroup, dim)), 0, 1).astype(F)
    # rows with a coordinate at 0 whose neighbour at an exact offset lies ON the radius, in one and in two active coordinates
    exact_q = []
    row = 0
    for y in (F(0), F(0.0125), F(0.01), F(0.015), F(0.0175), F(0.02), F(0.0075)):  # y = 0: one active coordinate; else two, fl(y * y) summed first
        for x in exact_radius_offsets(r2, y * y)[:2]:
            for k in (1, dim // 2, dim - 1):
                p = pts[npts - 1 - row]  # (a view: the row itself is edited)
                p[k - 1], p[k] = F(0), F(0)
                qq = p.copy()
                qq[k - 1], qq[k] = y, x
                assert dist32(qq, p) == r2
                exact_q.append(qq)
                row += 1
    n_active = rng.choice([1, 2, 3, dim], nitems)
    rows = pts[rng.integers(0, npts - row, nitems)]
    q_in, q_out = bisect_to_radius(rows, rows, _directions(rng, rows, n_active), r2, 3 * np.sqrt(float(r2)))
    # re-use boundary: the query near a row (so that a chain that does not re-use goes on to a hit) or anywhere, last_pss bisected around it
    qr = np.clip(pts[rng.integers(0, npts, nre)] + rng.normal(0, 0.004, (nre, dim)), 0, 1).astype(F)
    qr[nre // 2 :] = rng.random((nre - nre // 2, dim)).astype(F)
    l_in, l_out = bisect_to_radius(qr, qr, _directions(rng, qr, rng.choice([1, 2, 3, dim], nre)), rr2, 3 * np.sqrt(float(rr2)), moving_first=False)
    exact_q = np.array(exact_q, F).reshape(-1, dim)
    q = np.concatenate([q_in, q_out, exact_q, qr, qr])
    n_plain = 2 * nitems + len(exact_q)
    queried = np.concatenate([(rng.random(n_plain) < 0.3).astype(np.int32), np.ones(2 * nre, np.int32)])
    last_pss = np.concatenate([rng.random((n_plain, dim)).astype(F), l_in, l_out])
    return _finish("boundary", dim, rng, pts, q, queried, last_pss)


def lattice(dim, LV, seed=0, npts=3000, nitems=1500, n_on=300):
    """Rows on the lattice (j + 1/2) / LV + c: the tree's split planes pass through row coordinates, and many rows are duplicates (distance 0, weight
    1e6, their order is the tree's).  Queries ON rows and bisected to the radius around a row."""
    rng = np.random.default_rng(3000 + 100 * LV + 10 * dim + 1000 * seed)
    r2 = radius_sq(dim)
    c = F(1.0 / 64) if seed % 2 else F(0)
    nsites = npts // 4
    sites = ((rng.integers(0, LV, (nsites, dim)).astype(F) + F(0.5)) / F(LV) + c).astype(F)
    mult = rng.choice([1, 1, 1, 2, 3, 4, 7, 12], nsites)
    pts = np.repeat(sites, mult, 0)[:npts]
    pts = pts[rng.permutation(len(pts))]
    rows = pts[rng.integers(0, len(pts), nitems)]
    q_in, q_out = bisect_to_radius(rows, rows, _directions(rng, rows, rng.choice([1, 2, 3, dim], nitems)), r2, 3 * np.sqrt(float(r2)))
    on = pts[rng.integers(0, len(pts), n_on)]
    return _finish("lattice%d" % LV, dim, rng, pts, np.concatenate([q_in, q_out, on]))


def _edge_values(rng, j, G, shape):
    """j / G, one of its two float neighbours, or a point up to 0.02 beside it; j = G gives 1.0 or the float below it"""
    e = (j.astype(F) / F(G)).astype(F)
    kind = rng.integers(0, 5, shape)
    e = np.where(kind == 1, np.nextafter(e, F(0)), np.where(kind == 2, np.nextafter(e, F(2)), e))
    e = np.where(kind >= 3, e + rng.uniform(-0.02, 0.02, shape).astype(F), e).astype(F)
    return np.clip(e, 0, 1).astype(F)


def cell_edges(dim, seed=0, npts=3000, nq=3600):
    """Rows and queries with every coordinate at a cell edge j / G of the existence grid, at one of its float neighbours or just beside it, in groups
    around common edges: a row and a query in adjacent cells less than the radius apart; rows in the border cells (neighbour cells outside the grid);
    coordinates at 0, at 1.0 and at the float below 1.0."""
    rng = np.random.default_rng(4000 + 10 * dim + 1000 * seed)
    G, r2 = grid_g(dim), radius_sq(dim)
    ngroups = 300
    anchors = rng.integers(0, G + 1, (ngroups, dim))
    border = rng.random((ngroups, dim)) < 0.25
    anchors[border] = rng.choice([0, G], border.sum())
    pts = _edge_values(rng, anchors[rng.integers(0, ngroups, npts)], G, (npts, dim))
    n1 = nq // 2
    q1 = _edge_values(rng, anchors[rng.integers(0, ngroups, n1)], G, (n1, dim))
    n2 = nq // 4
    rows = pts[rng.integers(0, npts, n2)]
    q_in, q_out = bisect_to_radius(rows, rows, _directions(rng, rows, rng.choice([1, 2, 3, dim], n2)), r2, 3 * np.sqrt(float(r2)))
    return _finish("cell_edges", dim, rng, pts, np.concatenate([q1, q_in, q_out]))


def one_cell(dim, seed=0, npts=3000, nq=3000):
    """All rows but five inside one cell of the existence grid and its neighbours: the longest candidate list (2995 rows, not a multiple of the batch),
    scan tiles with one huge entry.  Queries inside the cell and just outside it."""
    rng = np.random.default_rng(5000 + 10 * dim + 1000 * seed)
    G = grid_g(dim)
    j0 = rng.integers(1, G - 1, dim)
    lo, hi = (j0 - 1) / G + 1e-4, (j0 + 2) / G - 1e-4
    centre = (j0 + 0.5) / G
    sig = rng.choice([0.003, 0.006, 0.012, 0.03], (npts, 1))
    pts = np.clip(centre + rng.normal(0, 1, (npts, dim)) * sig, lo, hi).astype(F)
    pts[:5] = np.clip(pts[:5] + 0.4 * np.where(centre > 0.5, -1, 1), 0, 1).astype(F)
    sigq = rng.choice([0.004, 0.008, 0.011, 0.02], (nq, 1))
    q = np.clip(centre + rng.normal(0, 1, (nq, dim)) * sigq, 0, 1).astype(F)
    return _finish("one_cell", dim, rng, pts, q)


def small(dim, npts, nq, seed=0):
    """a handful of rows (the one-leaf tree) up to 2999, and 1, 63, 64, 65 queries: a ragged last block"""
    rng = np.random.default_rng(6000 + 10 * dim + npts + 1000 * seed)
    centre = rng.uniform(0.2, 0.8, dim)
    pts = np.clip(centre + rng.normal(0, 0.004, (npts, dim)), 0, 1).astype(F)
    if npts > 100:
        pts[npts // 2 :] = rng.random((npts - npts // 2, dim)).astype(F)
    q = np.clip(centre + rng.normal(0, 0.008, (nq, dim)), 0, 1).astype(F)
    if npts <= 2:
        q[0] = pts[0]
    queried = (np.arange(nq) % 4 == 3).astype(np.int32)  # the first queries do query
    return _finish("small_%d_%d" % (npts, nq), dim, rng, pts, q, queried, rng.random((nq, dim)).astype(F))


SMALL_SHAPES = ((1, 1), (2, 63), (11, 64), (2999, 65))
CASE_NAMES = ("bulk", "boundary", "lattice3", "lattice4", "cell_edges", "one_cell") + tuple("small_%d_%d" % s for s in SMALL_SHAPES)
_memo = {}


def cases(dim):
    """every case of one dimension, built once per process (the arrays are shared: do not write to them)"""
    if dim not in _memo:
        cs = [bulk(dim), boundary(dim), lattice(dim, 3), lattice(dim, 4), cell_edges(dim), one_cell(dim)] + [small(dim, n, nq) for n, nq in SMALL_SHAPES]
        for c in cs:
            for a in c[2:]:
                a.setflags(write=False)
        _memo[dim] = {c.name: c for c in cs}
        assert tuple(_memo[dim]) == CASE_NAMES
    return _memo[dim]


def oracle_gaussian(L, c):
    """orc_cache_gaussian (oracle/capi.cpp) on a case: ints nq x 9 = [branch, matches, rows in search order (5), cache-query and cache-hit increments],
    weights nq x 5, chain nq x 3 x dim = v1, v2, last_pss afterwards, gauss nq x (3 dim + 1) = mean, covL, invCov, logDet"""
    nq, dim = c.q.shape
    ints, w = np.zeros((nq, 9), np.int32), np.zeros((nq, 5), F)
    chain, gauss = np.zeros((nq, 3, dim), F), np.zeros((nq, 3 * dim + 1), F)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    r = L.orc_cache_gaussian(dim, len(c.pts), ptr(c.pts), ptr(c.v1), ptr(c.v2), ctypes.c_float(MALA_STEPSIZE), ctypes.c_float(MALA_STDDEV), nq, ptr(c.q),
                             ptr(c.queried), ptr(c.last_pss), ptr(c.ch_v1), ptr(c.ch_v2), ptr(c.ss), ptr(ints), ptr(w), ptr(chain), ptr(gauss))
    assert r == 0
    return ints, w, chain, gauss


def branch_counts(c, ints):
    """how often a case reaches each branch of the look-up, from the oracle's outputs, the float32 brute-force count and the grid over the leading
    four coordinates: re-use, one row within the radius (the shortcut), 2-4, more than 5 (the search stops early), no candidate in the query's
    cell (the existence test says no), candidates but none within the radius"""
    cnt = count32(c.pts, c.q, radius_sq(c.dim))
    asks = ints[:, 0] != BRANCH_REUSE
    cand = has_candidates(c.pts, c.q, c.dim)
    return {
        "reuse": int((~asks).sum()),
        "one": int((asks & (cnt == 1)).sum()),
        "few": int((asks & (cnt >= 2) & (cnt <= 4)).sum()),
        "many": int((asks & (cnt > 5)).sum()),
        "empty_cell": int((asks & ~cand).sum()),
        "none_within": int((asks & cand & (cnt == 0)).sum()),
    }


def hunt_queries(dim, seed):
    """The queries of the hunt for a row the search prunes although the leaf arithmetic counts it: (pts, q, bisected) of one seed's boundary, lattice
    and cell-edge clouds -- smaller than the cases' clouds, so that the float32 brute-force count stays cheap, and nearly all of the queries
    bisected to the radius (`bisected` marks them)."""
    out = []
    b = boundary(dim, seed, npts=400, nitems=1900, nre=4)
    out.append((b.pts, b.q, np.arange(len(b.q)) < 3800))
    l = lattice(dim, 3 + seed % 2, seed, npts=400, nitems=600, n_on=20)
    out.append((l.pts, l.q, np.arange(len(l.q)) < 1200))
    e = cell_edges(dim, seed, npts=400, nq=1200)
    out.append((e.pts, e.q, np.arange(len(e.q)) >= 600))
    return out
