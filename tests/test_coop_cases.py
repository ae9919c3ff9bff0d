"""CPU tier: the case builder of tests/coop_cases.py against its own claims -- every case obeys the validity rules the work-list probes state
(include/lmc_abi.h), covers the edges it is there for (bin populations around a task's size, the last bin, every signature, more tasks than blocks,
both bounds of the states per task) and is deterministic.  Keeps the yardstick of tests/test_gpu_coop_lists.py honest without a GPU."""
import numpy as np
import pytest

from tests import coop_cases as cc

RECORD_KERNELS = ("mala_grad", "h2_hess")


def _all_cases():
    out = []
    for kernel in RECORD_KERNELS:
        for sid in (0, 1):
            out += [cc.baseline_case(kernel, sid, t) for t in cc.scene_techs(sid)]
            out += [cc.count_edge_case(kernel, sid, kind) for kind in cc.POPULATION_KINDS]
            m = cc.mixed_case(kernel, sid)
            out += [m.with_grid(g) for g in cc.grid_sizes(cc.total_tasks(kernel, m.count))]
    out += [cc.gauss_count_edge_case(kind) for kind in cc.POPULATION_KINDS]
    for stage in (0, 1):
        m = cc.gauss_mixed_case(stage)
        out += [m.with_grid(g) for g in cc.grid_sizes(cc.total_tasks("h2_gauss", m.count))]
    return out


def test_the_restated_plan():
    assert [cc.tech_index(*cc.tech_of(t)) for t in range(cc.NTECH)] == list(range(cc.NTECH))
    assert cc.tech_index(1, 8) == 41 and cc.tech_index(3, 0) == 0 and cc.tech_index(2, 0) == -1 and cc.tech_index(9, 1) == -1 and cc.tech_index(0, 5) == -1
    assert sorted({cc.tech_dim(t) for t in range(cc.NTECH)}) == [4, 6, 8, 10, 12, 14, 16]
    # the figures the kernels' comments give: 13 / 8 states of dim 6 / 12 per gradient wave, 10 / 3 per Hessian wave
    t6, t12 = cc.tech_index(4, 0), cc.tech_index(7, 0)
    assert (cc.rec_words(t6), cc.rec_words(t12)) == (320, 496)
    assert (cc.ipw("mala_grad", t6), cc.ipw("mala_grad", t12), cc.ipw("h2_hess", t6), cc.ipw("h2_hess", t12)) == (13, 8, 10, 3)
    assert cc.ipw("h2_hess", cc.tech_index(9, 0)) == 1 and cc.ipw("h2_gauss", 7) == 4
    for kernel, words in (("mala_grad", cc.MG_LDS_WORDS), ("h2_hess", cc.HESS_LDS_WORDS)):
        for t in range(cc.NTECH):
            n = cc.ipw(kernel, t)
            lanes = cc.tech_dim(t) // 2 if kernel == "mala_grad" else cc.blocks_of_dim(cc.tech_dim(t))
            assert n >= 1 and n * lanes <= 64 and n * cc.rec_words(t) <= words  # a task fits the wave and its LDS


def test_both_bounds_of_the_states_per_task_are_among_the_golden_techniques():
    bounds = {k: {cc.tech_dim(t): cc.plan(k, t)[1] for t in cc.golden_techs()} for k in cc.KERNELS}
    assert sorted(bounds["h2_hess"]) == [6, 8, 10, 12, 14, 16]
    # the Hessian: lanes bound dims 8 to 16, dim 6 is the tie (ten states by lanes and by LDS words)
    assert bounds["h2_hess"] == {6: "tie", 8: "lanes", 10: "lanes", 12: "lanes", 14: "lanes", 16: "lanes"}
    # the gradient: LDS words bound every golden dimension -- this kernel has NO technique here whose lanes bound a task (dim 4 would: out of scope)
    assert set(bounds["mala_grad"].values()) == {"lds"}
    # the Gaussian: four states whatever the technique -- neither bound applies
    assert set(bounds["h2_gauss"].values()) == {"fixed"}


def test_every_case_obeys_the_probes_validity_rules():
    cases = _all_cases()
    assert len(cases) > 150
    for c in cases:
        assert cc.case_problem(c) is None, c.name
        assert c.items.dtype == np.int32 and c.count.shape == (cc.BINS,) and c.start.shape == (cc.BINS,)
        assert c.listed.sum() == c.count.sum() == c.n_list
    for where in ("hess", "grad"):
        for group in (0, 3):
            c, pool, bad = cc.gauss_nonfinite_case(where, group)
            dims = pool["dim"][c.src]
            assert cc.check_valid(c.N, c.n_list, c.items, c.count, c.start, c.grid_blocks, lambda i, t: cc.tech_dim(t) == dims[i]) is None
    e = cc.empty_case(cc.mixed_case("h2_hess", 0))
    assert cc.case_problem(e) is None and e.count.sum() == 0 and e.n_list >= 1 and not e.listed.any()


def test_the_validity_rules_refuse_what_they_should():
    c = cc.mixed_case("h2_hess", 0)
    tech = cc.golden()["tech"][c.src]
    fits = lambda i, t: tech[i] == t
    ok = lambda **kw: cc.check_valid(**dict(dict(N=c.N, n_list=c.n_list, items=c.items, count=c.count, start=c.start, grid_blocks=3, fits=fits), **kw))
    assert ok() is None
    assert ok(n_list=0) == "n_list" and ok(N=c.n_list - 1) == "N" and ok(grid_blocks=0) == "grid_blocks" and ok(grid_blocks=4097) == "grid_blocks"
    it = c.items.copy()
    it[5] = c.N
    assert ok(items=it) == "items"
    it[5] = c.items[6]
    assert ok(items=it) == "items"
    b0, b1 = np.flatnonzero(c.count)[:2]
    st = c.start.copy()
    st[b1] = c.start[b0]
    assert ok(start=st) == "start"
    st[b1] = c.n_list
    assert ok(start=st) == "start"
    cnt = c.count.copy()
    cnt[b0] = -1
    assert ok(count=cnt) == "count"
    it = c.items.copy()
    a, b = c.start[b0], c.start[np.flatnonzero(c.count)[-1]]  # entries of the first and of the last bin: different techniques
    it[a], it[b] = it[b], it[a]
    assert ok(items=it) == "technique"


@pytest.mark.parametrize("kernel", cc.KERNELS)
def test_count_edges_cover_the_populations_they_claim(kernel):
    for sid in (0, 1):
        techs = cc.scene_techs(sid) if kernel != "h2_gauss" else cc.golden_techs()
        seen = {t: [] for t in techs}
        for kind in cc.POPULATION_KINDS:
            c = cc.count_edge_case(kernel, sid, kind) if kernel != "h2_gauss" else cc.gauss_count_edge_case(kind)
            bins = np.flatnonzero(c.count)
            assert len(set(bins // cc.NSIG)) == len(bins)  # one bin per technique
            for b in bins:
                seen[b // cc.NSIG].append(int(c.count[b]))
            assert c.N >= 2 * c.n_list and not c.listed.all()  # unlisted chains in between
            assert c.grid_blocks >= cc.total_tasks(kernel, c.count)
        for t, pops in seen.items():
            n = cc.ipw(kernel, t)
            assert pops == [p for p in (1, n - 1, n, n + 1, 2 * n, 2 * n + 1) if p > 0], (t, pops)
    if kernel != "h2_gauss":  # replication: a population beyond a technique's six golden states repeats them
        c = cc.count_edge_case(kernel, 0, "2ipw+1")
        assert max(np.bincount(c.src[c.listed])) >= 2


@pytest.mark.parametrize("kernel", cc.KERNELS)
def test_mixed_lists_cover_the_edges_they_claim(kernel):
    cases = [cc.mixed_case(kernel, sid) for sid in (0, 1)] if kernel != "h2_gauss" else [cc.gauss_mixed_case(0), cc.gauss_mixed_case(1)]
    for c in cases:
        bins = np.flatnonzero(c.count)
        techs = sorted(set(bins // cc.NSIG))
        assert techs == (cc.scene_techs(c.scene) if kernel != "h2_gauss" else cc.gauss_techs())
        assert len(bins) == 8 * len(techs)  # every signature of every technique
        tasks = cc.total_tasks(kernel, c.count)
        assert tasks >= 40 and tasks > len(bins)  # some bins need a second task
        assert [g for g in cc.grid_sizes(tasks) if g < tasks] == [1, 2, 3, tasks - 1] and cc.grid_sizes(tasks)[-1] == 1024 > tasks  # second trips; one wave walks all
        # bins in bin order, start = the exclusive prefix over all bins (what LaunchBinsCompact leaves)
        assert np.array_equal(c.start, np.concatenate([[0], np.cumsum(c.count)[:-1]]))
        # chain ids shuffled within and across bins, about half the chains unlisted and interleaved
        assert (np.diff(c.items) < 0).sum() > c.n_list // 4 and c.N == 2 * c.n_list + 1
        assert 0.3 < c.listed[: c.N // 2].mean() < 0.7
        for t in techs:
            pops = c.count[t * 8: t * 8 + 8]
            assert sorted(pops) == sorted([1, 1, 1, 1, 1, 1, 2, cc.ipw(kernel, t) + 1])
        assert c.n_list < 1000
    if kernel == "h2_gauss":
        for c in cases:
            assert sorted(set(cc.gauss_pool()["dim"][c.src[c.listed]])) == [6, 8, 10, 12, 14, 16]
            on = (c.flags[c.listed] & cc.F_GSEL) != 0
            assert 0.35 < on.mean() < 0.65 and (c.flags & ~cc.F_GSEL).any()
        assert [c.stage for c in cases] == [0, 1] and cases[0].count[335] > 0
    else:
        assert cases[1].count[335] > 0 and cc.tech_of(335 // 8) == (1, 8)  # the last bin: the door set's (c = 1, l = 8), signature 7
        assert cases[0].count[335] == 0  # (the torus set has no such paths)


def _fits(case):
    if case.kernel == "h2_gauss":
        dims = cc.gauss_pool()["dim"][case.src]
        return lambda i, t: cc.tech_dim(t) == dims[i]
    tech = cc.golden()["tech"][case.src]
    return lambda i, t: tech[i] == t


@pytest.mark.parametrize("kernel", cc.KERNELS)
def test_the_documented_walk_visits_every_listed_chain_once_and_the_cases_tell_a_broken_walk(kernel):
    """The walk of dh2coop.h restated (coop_cases.model_walk) takes every listed chain exactly once, as a state of its own technique, on every case; with
    start[bin] dropped, with the count not reduced by `first`, or with the bin looked up by w instead of wr it does not -- on the count edges and on the
    mixed list alike -- so a launch with one of these mistakes cannot produce the rows tests/test_gpu_coop_lists.py asks for."""
    cases = [c for c in _all_cases() if c.kernel == kernel and "/grid" not in c.name] + [cc.gauss_mixed_case(1) if kernel == "h2_gauss" else cc.mixed_case(kernel, 1)]
    caught = {m: 0 for m in cc.WALK_MISTAKES}
    for c in cases:
        fits = _fits(c)
        right = cc.model_walk(c)
        assert sorted(i for i, t in right) == sorted(np.flatnonzero(c.listed)) and all(fits(i, t) for i, t in right), c.name
        if c.name.startswith("baseline") or c.n_list < 2:
            continue
        for m in cc.WALK_MISTAKES:
            wrong = cc.model_walk(c, m)
            broken = any(i is None or not fits(i, t) for i, t in wrong) or sorted(i for i, t in wrong) != sorted(np.flatnonzero(c.listed))
            caught[m] += broken
            if c.name.startswith("mixed"):
                assert broken, (c.name, m)
    assert all(n >= 3 for n in caught.values()), caught  # (a count that is not reduced shows only where a bin has a second task: "ipw+1", "2ipw", "2ipw+1", mixed)


def test_nonfinite_cases():
    for where in ("hess", "grad"):
        for group in (0, 3):
            c, pool, bad = cc.gauss_nonfinite_case(where, group)
            d, g, h, f, o = cc.gauss_inputs(c, pool)
            assert c.n_list == 4 and c.count.sum() == 4 and cc.total_tasks("h2_gauss", c.count) == 1 and bad == group and (d == 8).all()
            finite = np.isfinite(g).all(axis=1) & np.isfinite(h).all(axis=1)
            assert list(np.flatnonzero(~finite)) == [bad]
            if where == "hess":
                r, col = np.argwhere(~np.isfinite(h[bad, :64].reshape(8, 8)))[0]
                assert r < col  # in the triangle the launch reads
            norms = np.sqrt((np.where(np.isfinite(h), h, 0).astype(np.float64) ** 2).sum(axis=1))
            assert (norms > 4 * cc.EARLYOUT_NORM).all()  # the finite three are dense records: a leaked flag would change them
            assert len(set(c.src)) == 4
            assert np.isfinite(cc.gauss_pool()["hess"]).all() and np.isfinite(cc.gauss_pool()["grad"]).all()  # the shared pool stays clean


def test_the_builder_is_deterministic():
    a, b = _all_cases(), _all_cases()
    for x, y in zip(a, b):
        assert x.name == y.name and x.grid_blocks == y.grid_blocks
        for f in ("src", "items", "count", "start"):
            assert np.array_equal(getattr(x, f), getattr(y, f)), (x.name, f)
        if x.kernel == "h2_gauss":
            assert np.array_equal(x.flags, y.flags)
    assert len({c.name for c in a}) == len(a)
    p = cc.gauss_pool()
    assert p["hess"].dtype == np.float32 and len(p["dim"]) == 24 * 6
