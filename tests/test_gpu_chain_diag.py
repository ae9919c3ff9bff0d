"""GPU tier: the chain diagnostics (include/lmc_abi.h "Chain diagnostics"; device/chaindiag.hip, host/chaindiag.cpp): rows gathered on the device
against lmc_chain_summary, traces against single steps, the step table against a recount from a trace of every chain and against lmc_stats.
Everything compared is a copied word or an integer count: exact comparisons only (rows are compared as 32-bit patterns, so a NaN word counts too).
Populations and scene as tests/test_gpu_lists.py: the Lambertian torus at 128 x 96, max depth 6, gradients on, 1000 / 4097 / 5000 chains."""
import functools
import os

import numpy as np
import pytest

from tests import gpu_checks as gc

pytestmark = pytest.mark.gpu

H2MC_XML = os.path.join(gc.ROOT, "scenes", "torus", "h2mc.xml")
STEPS = 40  # the fill-phase pipeline and the full re-sorts after step 4 and step 36
ROW = 48


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _renderer(xml=None, max_depth=6, force_diffuse=1, opts=None):
    ren = gc.pkg().Renderer(xml or gc.TORUS, force_diffuse=force_diffuse, max_depth=max_depth, width=128, height=96, seed_offset=0, use_gradient=1)
    for k, v in (opts or {}).items():
        ren.set_option(k, v)
    return ren


def _init(ren, n, relocate=True, begin=0, end=None):
    os.environ["LMC_RELOCATE"] = "1" if relocate else "0"
    try:
        ren.init_chains(200000, n, 64, 10 ** 6, chain_begin=begin, chain_end=end)
    finally:
        del os.environ["LMC_RELOCATE"]
    return ren


def _summary48(ren, which=0):
    p = gc.pkg()
    out = np.zeros((ren.num_chains, ROW), np.float32)
    assert p.lib().lmc_chain_summary(ren.h, which, p.P(out), ROW) >= 0, p._err()
    return out


def _ids(n, extra, seed=7):
    """{0, 1, 63, 64, n - 1} plus `extra` random ids, in a shuffled order"""
    rng = np.random.default_rng(seed)
    rest = rng.choice(np.setdiff1d(np.arange(n), [0, 1, 63, 64, n - 1]), extra, replace=False)
    ids = np.concatenate([[0, 1, 63, 64, n - 1], rest]).astype(np.int32)
    rng.shuffle(ids)
    return ids


@functools.lru_cache(maxsize=None)
def _single_steps(n, xml=None, steps=STEPS):
    """context B: step(1) `steps` times, lmc_chain_summary (stride 48) of every chain after each -> [steps, n, 48], read-only"""
    ren = _init(_renderer(xml), n)
    out = np.zeros((steps, n, ROW), np.float32)
    for s in range(steps):
        ren.step(1)
        out[s] = _summary48(ren)
    ren.close()
    out.setflags(write=False)
    return out


def _trace(n, ids, steps=STEPS, xml=None, relocate=True, opts=None, capacity=None):
    """context A: a trace of `ids` over ONE step(steps) call -> (first_step, dropped, rows, resident stats)"""
    ren = _init(_renderer(xml, opts=opts), n, relocate=relocate)
    ren.trace_chains(ids, capacity or steps)
    ren.step(steps)
    first, dropped, rows = ren.trace_read()
    rs = ren.resident_stats()
    ren.trace_end()
    ren.close()
    return first, dropped, rows, rs


def _same_as_single_steps(rows, ids, ref):
    assert rows.shape == (ref.shape[0], len(ids), ROW)
    got, want = _bits(rows[:, :, :40]), _bits(ref[:, ids, :40])
    bad = np.argwhere(got != want)
    assert not len(bad), (len(bad), bad[:5])


# ---------------------------------------------------------------------------------------------- 1. rows against the summary
@pytest.mark.parametrize("which", [0, 1])
def test_rows_equal_the_summary(which):
    n = 5000
    ren = _init(_renderer(), n)
    ren.step(7)
    assert ren.relocation_stats() is not None and (ren.chain_slots()[0] != np.arange(n)).sum() > n // 2, "test set-up: the chains did not move"
    rng = np.random.default_rng(3)
    ids = np.concatenate([[0, n - 1, 17, 17], rng.choice(n, 65, replace=False)]).astype(np.int32)
    rows = ren.chain_rows(ids, which)
    want = _summary48(ren, which)
    ren.close()
    assert rows.shape == (len(ids), ROW)
    assert np.array_equal(_bits(rows[:, :40]), _bits(want[ids, :40]))
    assert (rows[:, 43:] == 0).all()
    if which == 1:
        assert (rows[:, 40:43] == 0).all()
    else:
        assert (rows[:, 40] == -1).all(), "word 40 outside a trace"
        assert np.array_equal(rows[:, 42].astype(np.int64) & 1, rows[:, 0].astype(np.int64)), "flags word: F_VALID"
        assert (rows[:, 41] >= 0).all() and (rows[:, 41] == np.trunc(rows[:, 41])).all()


def test_rows_of_long_paths_carry_pss_16_to_23():
    n = 1000
    ren = _init(_renderer(max_depth=12, force_diffuse=0), n)
    ren.step(7)
    ids = np.arange(n, dtype=np.int32)
    for which in (0, 1):
        rows, want = ren.chain_rows(ids, which), _summary48(ren, which)
        assert np.array_equal(_bits(rows[:, :40]), _bits(want[:, :40])), which
        assert (rows[:, 32:40] != 0).any(), ("no row with a primary sample beyond the 16th", which)
    ren.close()


# ---------------------------------------------------------------------------------------------- 2 - 4. traces against single steps
N_TRACE = 4097


def test_trace_equals_single_steps():
    ids = _ids(N_TRACE, 60)
    first, dropped, rows, rs = _trace(N_TRACE, ids)
    assert (first, dropped, rows.shape[0]) == (1, 0, STEPS)
    _same_as_single_steps(rows, ids, _single_steps(N_TRACE))
    kinds = rows[:, :, 40]
    assert np.isin(kinds, [1, 2, 3]).all() and (kinds[0] == 1).all(), "every chain steps, and its first step is a large step"
    assert (rows[:, :, 43:] == 0).all()


@pytest.mark.parametrize("variant", ["relocation_off", "resort_every_1"])
def test_trace_does_not_depend_on_the_slot_order(variant):
    ids = _ids(N_TRACE, 60)
    first, dropped, rows, rs = _trace(N_TRACE, ids, relocate=variant != "relocation_off", opts={"resort_every": 1, "resort_first": 0} if variant == "resort_every_1" else None)
    assert (first, dropped) == (1, 0)
    _same_as_single_steps(rows, ids, _single_steps(N_TRACE))


def test_an_open_trace_keeps_the_resident_option_in_lock_step():
    ids = _ids(N_TRACE, 60)
    first, dropped, rows, rs = _trace(N_TRACE, ids, opts={"resident_steps": 8})
    assert rs["k"] >= 1, "test set-up: the resident option is not in force"
    assert rs["launches"] == 0 and rs["lock_steps"] == STEPS, rs
    assert (first, dropped) == (1, 0)
    _same_as_single_steps(rows, ids, _single_steps(N_TRACE))


# ---------------------------------------------------------------------------------------------- 5. group
def test_group_members_trace_their_own_chains():
    n = 1000
    p = gc.pkg()
    ids = _ids(n, 60)
    _, _, whole, _ = _trace(n, ids)
    rens = [_renderer(), _renderer()]
    grp = p.Group(rens)
    os.environ["LMC_RELOCATE"] = "1"
    try:
        grp.init_chains(200000, n, 64, 10 ** 6)
    finally:
        del os.environ["LMC_RELOCATE"]
    halves = [ids[ids < n // 2], ids[ids >= n // 2]]
    with pytest.raises(RuntimeError):  # a member refuses the other member's chains
        rens[0].trace_chains(halves[1][:3], STEPS)
    for ren, h in zip(rens, halves):
        ren.trace_chains(h, STEPS)
    grp.step(STEPS)
    union = np.zeros_like(whole)
    for ren, h in zip(rens, halves):
        first, dropped, rows = ren.trace_read()
        assert (first, dropped, rows.shape[0]) == (1, 0, STEPS)
        union[:, np.isin(ids, h)] = rows
        ren.trace_end()
    for ren in rens:
        ren.close()
    assert np.array_equal(_bits(union), _bits(whole))


# ---------------------------------------------------------------------------------------------- 6. capacity
def test_a_full_buffer_drops_and_counts():
    n = 1000
    ids = _ids(n, 11)
    ren = _init(_renderer(), n)
    ren.trace_chains(ids, 5)
    ren.step(8)
    first, dropped, rows = ren.trace_read()
    assert (first, dropped, rows.shape) == (1, 3, (5, len(ids), ROW))
    ren.step(2)
    first, dropped, more = ren.trace_read()
    assert (first, dropped, more.shape) == (9, 0, (2, len(ids), ROW))
    assert np.array_equal(_bits(more[-1]), _bits(ren.chain_rows(ids))), "the row of step s is what chain_rows returns after step s"
    ren.trace_end()
    ren.close()
    ref = _single_steps(n)
    assert np.array_equal(_bits(rows[:, :, :40]), _bits(ref[:5][:, ids, :40])) and np.array_equal(_bits(more[:, :, :40]), _bits(ref[8:10][:, ids, :40]))


# ---------------------------------------------------------------------------------------------- 7, 8. the step table
def _recount(rows):
    """the table from trace rows: word 40 the kind, word 41 == 0 accepted, words 1 and 2 the technique"""
    t = np.zeros((3, 13, 13, 2), np.int64)
    r = rows.reshape(-1, ROW)
    r = r[r[:, 40] >= 1]
    k, c, l = r[:, 40].astype(np.int64) - 1, r[:, 1].astype(np.int64), r[:, 2].astype(np.int64)
    np.add.at(t, (k, c, l, 0), 1)
    acc = r[:, 41] == 0
    np.add.at(t, (k[acc], c[acc], l[acc], 1), 1)
    return t


# (name, chains, gradients, untraced steps first, planes that must be non-empty)
RECOUNT_CASES = (("lmc_1000", 1000, True, 0, (0, 1)), ("mlt_1000", 1000, False, 0, (0, 2)), ("lmc_4097_caches_ready", 4097, True, 200, (0, 1, 2)))


@pytest.mark.parametrize("name,n,mala,warm,planes", RECOUNT_CASES, ids=[c[0] for c in RECOUNT_CASES])
def test_table_equals_a_recount_from_the_trace_of_every_chain(name, n, mala, warm, planes):
    """ALL chains traced and the table on for 40 steps: the NumPy recount from the rows equals the table cell for cell, and at least three techniques
    are hit.  The planes: with gradients on, a chain takes the lean launch only once its dimension's gradient cache (3000 rows) is ready, and at 1000
    chains none becomes ready -- measured on an MI355X: steps per kind [large, generic, lean] of steps 1..40 [6735, 33265, 0], of every later 20 steps up
    to step 320 about [1000, 19000, 0], lmc_stats' cacheReadyMask 0 throughout; at 4097 chains the first cache is ready between steps 141 and 160
    ([4100, 36944, 40896] for steps 141..160).  So the 1000-chain render with gradients can only show the large and the generic plane; the lean plane is
    asserted where it exists: on the same 1000 chains as plain MLT (every small step is a lean one), and with gradients at 4097 chains after 200 untraced
    steps, where all three planes are filled."""
    ren = _renderer(opts=None if mala else {"mala": 0})
    _init(ren, n)
    if warm:
        ren.step(warm)
    ren.trace_chains(np.arange(n, dtype=np.int32), STEPS)
    ren.set_option("step_table", 1)
    assert ren.get_option("step_table") == 1
    ren.step(STEPS)
    first, dropped, rows = ren.trace_read()
    table = ren.step_table()
    ren.trace_end()
    ren.close()
    assert (first, dropped, rows.shape[0]) == (warm + 1, 0, STEPS)
    want = _recount(rows)
    print(name, "steps per kind", table[..., 0].sum((1, 2)), "accepted per kind", table[..., 1].sum((1, 2)), "techniques", int((table[..., 0].sum(0) > 0).sum()))
    assert np.array_equal(table, want)
    for k in range(3):
        assert (table[k, :, :, 0].sum() > 0) == (k in planes), ("plane", k, table[..., 0].sum((1, 2)))
    assert (table[..., 0].sum(0) > 0).sum() >= 3, "techniques hit"
    assert table[..., 0].sum() == n * STEPS and (table[..., 1] <= table[..., 0]).all()


def test_table_equals_the_counters():
    n = N_TRACE
    ren = _init(_renderer(), n)
    ren.step(3)
    assert not ren.step_table().any()
    ren.set_option("step_table", 1)
    st0 = ren.stats()
    ren.step(STEPS)
    st1 = ren.stats()
    table = ren.step_table()
    assert table[..., 0].sum() == st1["steps"] - st0["steps"] == n * STEPS
    assert table[0, :, :, 0].sum() == st1["largeSteps"] - st0["largeSteps"]
    assert table[..., 1].sum() == st1["accepted"] - st0["accepted"]
    ren.set_option("step_table", 0)
    assert ren.get_option("step_table") == 0
    ren.step(2)
    assert np.array_equal(ren.step_table(), table), "with the option off the table stays put"
    assert np.array_equal(ren.step_table(clear=True), table) and not ren.step_table().any(), "clear zeroes the table behind the copy"
    ren.close()


# ---------------------------------------------------------------------------------------------- 9. H2MC
def test_h2mc_trace_equals_single_steps_and_runs_generic_small_steps():
    n, steps = 1000, 6
    ids = _ids(n, 60)
    first, dropped, rows, rs = _trace(n, ids, steps=steps, xml=H2MC_XML)
    assert (first, dropped) == (1, 0)
    _same_as_single_steps(rows, ids, _single_steps(n, H2MC_XML, steps))
    kinds = rows[:, :, 40]
    assert np.isin(kinds, [1, 2]).all() and (kinds == 2).any() and (kinds == 1).any(), np.unique(kinds)


# ---------------------------------------------------------------------------------------------- 10. refusals
def test_refusals_leave_the_context_usable():
    p = gc.pkg()
    L = p.lib()
    n = 1000
    ids = _ids(n, 11)

    def refused(call):
        assert call() == -1
        assert len(p._err()) > 0
        return p._err()

    ren = _renderer()
    refused(lambda: L.lmc_chain_trace_begin(ren.h, p.P(ids), len(ids), 4))  # before lmc_chains_init
    refused(lambda: L.lmc_chain_rows(ren.h, 0, p.P(ids), len(ids), p.P(np.zeros((len(ids), ROW), np.float32))))
    _init(ren, n, begin=0, end=n)
    refused(lambda: L.lmc_chain_trace_read(ren.h, None, 0, None, None, None))
    refused(lambda: L.lmc_chain_trace_end(ren.h))
    refused(lambda: L.lmc_chain_trace_begin(ren.h, p.P(ids), 0, 4))
    refused(lambda: L.lmc_chain_trace_begin(ren.h, p.P(ids), -2, 4))
    refused(lambda: L.lmc_chain_trace_begin(ren.h, p.P(ids), len(ids), 0))
    for bad in (-1, n, 1 << 30):
        wrong = ids.copy()
        wrong[5] = bad
        assert str(bad) in refused(lambda: L.lmc_chain_trace_begin(ren.h, p.P(wrong), len(wrong), 4))
        out = np.full((len(ids), ROW), 7.0, np.float32)
        refused(lambda: L.lmc_chain_rows(ren.h, 0, p.P(wrong), len(wrong), p.P(out)))
        assert (out == 7.0).all(), "nothing is written"
    huge = 2 ** 31 - 1  # steps x 16 chains x 192 bytes: 6.6 TB, more than the device has
    assert str(huge * 16 * ROW * 4) in refused(lambda: L.lmc_chain_trace_begin(ren.h, p.P(ids), 16, huge)), "an allocation failure names the byte count"
    refused(lambda: L.lmc_chain_trace_read(ren.h, None, 0, None, None, None))  # none of the refused calls opened a trace
    ren.trace_chains(ids, 4)
    refused(lambda: L.lmc_chain_trace_begin(ren.h, p.P(ids), len(ids), 4))  # while a trace is open
    ren.step(4)
    small = np.zeros((2, len(ids), ROW), np.float32)
    refused(lambda: L.lmc_chain_trace_read(ren.h, p.P(small), 2, None, None, None))  # rows too small: nothing read, nothing lost
    first, dropped, rows = ren.trace_read()
    assert (first, dropped, rows.shape[0]) == (1, 0, 4)
    assert np.array_equal(_bits(rows[:, :, :40]), _bits(_single_steps(n)[:4][:, ids, :40]))
    ren.init_chains(200000, n, 64, 10 ** 6)  # closes the open trace
    refused(lambda: L.lmc_chain_trace_end(ren.h))
    ren.close()


# ---------------------------------------------------------------------------------------------- 11. non-interference
def test_diagnostics_change_nothing_in_the_render():
    n, steps = 1000, 24
    runs = []
    for diag in (False, True):
        ren = _renderer(opts={"film_exact": 1})
        _init(ren, n)
        if diag:
            ren.trace_chains(_ids(n, 60), steps)
            ren.set_option("step_table", 1)
        ren.step(steps)
        runs.append((_summary48(ren), ren.stats(), ren.film_fixed().copy()))
        ren.close()
    (s0, st0, f0), (s1, st1, f1) = runs
    assert np.array_equal(_bits(s0), _bits(s1))
    for k in gc.STAT_KEYS:  # (weightSum is a sum of double atomics: its last bits depend on the order of the adds, with or without diagnostics)
        assert st0[k] == st1[k], (k, st0[k], st1[k])
    assert f0.any() and np.array_equal(f0, f1)


# ---------------------------------------------------------------------------------------------- the command line
def test_dpt_amd_writes_the_trace_file_and_prints_the_table(tmp_path):
    """dpt_amd --trace-chains / --trace-file / --trace-steps / --step-table on a small mcmc scene: the file holds the rows of a Python trace of the
    same render, the table's lines sum to the mutations the tool reports; the flags' errors name their reason"""
    import re
    import subprocess

    from tests.test_gpu_cli import CLI, _small_scene

    p = gc.pkg()
    scene = _small_scene(tmp_path, spp=8)  # 8 x 96 x 72 samples over 1000 chains: 55 each, one call of 64 steps
    n, ids, steps = 1000, [999, 0, 17, 500], 10
    out = str(tmp_path / "chains.lmctrace")
    r = subprocess.run([CLI, "--seedoffset", "0", "--chains", str(n), "--trace-chains", ",".join(map(str, ids)), "--trace-file", out, "--trace-steps", str(steps), "--step-table", scene],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("Done!"), r.stdout
    t = p.trace_file_read(out)
    assert list(t["ids"]) == ids and t["first_step"] == 1 and t["rows"].shape == (steps, len(ids), ROW)
    per_chain = 8 * 96 * 72 // n
    ren = p.Renderer(scene, seed_offset=0, use_gradient=1)
    ren.init_chains(max(int(ren.get_option("numinitsamples")), 8 * n), n, 65536, per_chain, per_chain % n)  # what dpt_amd passes (tools/dpt_amd.cpp)
    ren.trace_chains(ids, steps)
    ren.step(steps)
    _, _, rows = ren.trace_read()
    ren.close()
    assert np.array_equal(_bits(t["rows"]), _bits(rows))
    cells = [[int(v) for v in m] for m in re.findall(r"^([123]) (\d+) (\d+) (\d+) (\d+)$", r.stdout, re.M)]
    mutations = int(re.search(r"(\d+) mutations", r.stdout).group(1))
    assert cells and sum(c[3] for c in cells) == mutations and all(c[4] <= c[3] for c in cells), (cells, mutations)
    for argv, what in ((["--trace-chains", "1,2", scene], "--trace-file"), (["--trace-file", out, scene], "--trace-chains"),
                       (["--devices", "0,0", "--step-table", scene], "one device"), (["--devices", "0,0", "--trace-chains", "1", "--trace-file", out, scene], "one device")):
        r = subprocess.run([CLI] + argv, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        assert r.returncode == 2 and what in r.stdout, (argv, r.stdout)
    mc = tmp_path / "mc.xml"
    mc.write_text(open(scene).read().replace('name="integrator"     value="mcmc"', 'name="integrator"     value="mc"'))
    assert 'value="mc"' in mc.read_text()
    for argv in (["--step-table"], ["--trace-chains", "1", "--trace-file", out]):
        r = subprocess.run([CLI] + argv + [str(mc)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        assert r.returncode == 2 and "integrator=mc" in r.stdout, (argv, r.stdout)
