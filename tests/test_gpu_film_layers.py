"""Layered MLT film (include/lmc_abi.h "Layered MLT film", langevin-mcmc_amd/csrc/device/dchain.h ChainFilmLayers, INTEGRATION.md "Layered MLT film"): with
film_layers = 1 | 2 (and film_exact = 1) every splat of the chain loop goes to the exact film of its contribution's path length or technique.  Every
comparison here is WORD FOR WORD (np.array_equal of int64).  Shapes, cases and helpers are those of tests/test_gpu_film_exact.py: the torus at 128 x 96,
force_diffuse, `plain` (4096 chains, maxdepth 6), `mala4` / `mux` / `samplecache` (16384 chains, maxdepth 4, FILL), 30 steps; the unlayered reference
of a case is that file's shared run."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import gpu_checks as gc
from tests import test_gpu_film_exact as fe
from tests.test_gpu_relocate import _same_states

pytestmark = pytest.mark.gpu
LENGTH, TECHNIQUE = 1, 2
NAMES = ("plain", "mala4", "mux", "samplecache")
STEPS = fe.STEPS


def _layered(cfg, mode, env=None, resident=0):
    with fe._Env(env):
        ren = fe._renderer(resident=resident, **cfg)
        ren.set_option("film_layers", mode)
        ren.init_chains(200000, cfg["n"], 64, 10 ** 6)
    return ren


def _layered_result(ren):
    out = fe._result(ren)
    out["layers"] = ren.film_layers_fixed().copy()
    out["info"] = ren.film_layer_info()
    return out


@functools.lru_cache(maxsize=None)
def _layered_run(name, mode):
    """the layered run of a case, computed once and shared (never written to)"""
    ren = _layered(fe.CASES[name], mode)
    ren.step(STEPS)
    out = _layered_result(ren)
    ren.close()
    out["layers"].setflags(write=False)
    return out


def _table(mode, D):
    return [(L, -1) for L in range(1, D + 1)] if mode == LENGTH else [(L + 1 - l, l) for L in range(1, D + 1) for l in range(L + 1)]


def _layer_of(mode, c, l):
    """vectorised numbering rule of the header; -1: no such technique"""
    L = c + l - 1
    k = np.where(mode == LENGTH, L - 1, (L - 1) * (L + 2) // 2 + l)
    return np.where((c < 1) | (l < 0) | (L < 1), -1, k)


def _expected_layers(W, H, mode, D, xy, v, c, l):
    """the integer rule of the device's layered splat routine: (words [n, H, W, 3], overflow word, finite splats outside the table)"""
    n_layers = D if mode == LENGTH else D * (D + 3) // 2
    finite = np.isfinite(v).all(axis=1)
    in_range = (np.abs(v) < np.float32(2.0 ** 30)).all(axis=1)
    layer = _layer_of(mode, c.astype(np.int64), l.astype(np.int64))
    inside = (layer >= 0) & (layer < n_layers)
    ix = np.clip((xy[:, 0] * np.float32(W)).astype(np.int32), 0, W - 1)
    iy = np.clip((xy[:, 1] * np.float32(H)).astype(np.int32), 0, H - 1)
    keep = finite & in_range & inside
    q = np.rint(v[keep].astype(np.float64) * 2.0 ** 32).astype(np.int64)
    exp = np.zeros((n_layers, H, W, 3), np.int64)
    np.add.at(exp, (layer[keep], iy[keep], ix[keep]), q)
    return exp, int((finite & ~(in_range & inside)).sum()), int((finite & ~inside).sum()), (layer, ix, iy, keep)


# ------------------------------------------------------------------------------------------------ 1. the splat routine against integers
@pytest.mark.parametrize("D", [3, 12])
@pytest.mark.parametrize("mode", [LENGTH, TECHNIQUE], ids=["length", "technique"])
def test_probe_against_integers(mode, D):
    """1. the 4096 splats of tests/test_gpu_film_exact.py::_probe_splats on a 4 x 3 film, labelled over the whole table of D: at least 1024 on one
    (pixel, layer); c < 1, l < 0, L < 1 and L > D (counted in `outside`, nothing written); the non-finite ones dropped silently and those of 2^30 or more
    counted, exactly as unlayered.  The words equal the numpy integers; three permutations give the same words."""
    W, H, xy, v = fe._probe_splats()
    n = len(v)
    rng = np.random.default_rng(20262 + D)
    L = rng.integers(1, D + 1, n)
    l = (rng.random(n) * (L + 1)).astype(np.int64)
    c = L + 1 - l
    c[:1100], l[:1100] = 2, 1  # the first 1500 splats share pixel (2, 1): 1100 of them on one layer
    bad = rng.choice(np.arange(1500, n), 16, replace=False)
    c[bad[0:2]], l[bad[0:2]] = 0, 3           # c < 1
    c[bad[2:4]], l[bad[2:4]] = -2, 5
    c[bad[4:6]], l[bad[4:6]] = 3, -1          # l < 0
    c[bad[6:8]], l[bad[6:8]] = 1, 0           # L < 1
    c[bad[8:10]], l[bad[8:10]] = D + 1, 1     # L = D + 1
    c[bad[10:12]], l[bad[10:12]] = 1, D + 1   # L = D + 1, light tracing
    c[bad[12:14]], l[bad[12:14]] = 13, 12     # far outside
    v[bad[14]] = [np.nan, 1.0, 1.0]           # outside AND non-finite: dropped silently, not counted
    c[bad[14]], l[bad[14]] = 0, 0
    v[bad[15]] = [np.float32(2.0 ** 31), 1.0, 1.0]  # outside AND out of range: counted once
    c[bad[15]], l[bad[15]] = D + 2, 0
    cl = np.stack([c, l], axis=1).astype(np.int32)
    exp, n_over, n_outside, (layer, ix, iy, keep) = _expected_layers(W, H, mode, D, xy, v, c, l)
    per_cell = np.bincount((layer[keep] * H + iy[keep]) * W + ix[keep])
    assert per_cell.max() >= 1024 and n_outside >= 12 and n_over > n_outside
    assert (exp.reshape(len(exp), -1) != 0).any(axis=1).all(), "test set-up: a layer of the table received nothing"
    fx, over, outside = gc.pkg().film_layer_splat_probe(W, H, mode, D, xy, v, cl)
    print("mode %d D %d: %d layers, overflow word %d, outside %d, busiest (pixel, layer) %d" % (mode, D, len(exp), over, outside, per_cell.max()))
    fe._assert_same_words(fx, exp)
    assert (over, outside) == (n_over, n_outside)
    for seed in range(3):
        perm = np.random.default_rng(seed).permutation(n)
        fx2, over2, outside2 = gc.pkg().film_layer_splat_probe(W, H, mode, D, xy[perm], v[perm], cl[perm])
        fe._assert_same_words(fx2, exp)
        assert (over2, outside2) == (n_over, n_outside)
    # a caller that ignores the layers: their sum is the unlayered probe's film of the splats inside the table
    inside = (layer >= 0) & (layer < len(exp))
    un, _, over_un = gc.pkg().film_splat_probe(W, H, xy[inside], v[inside], exact=True)
    fe._assert_same_words(fx.sum(0), un)
    assert over_un == n_over - n_outside


# ------------------------------------------------------------------------------------------------ 2. the layers sum to the unlayered exact film
@pytest.mark.parametrize("mode", [LENGTH, TECHNIQUE], ids=["length", "technique"])
@pytest.mark.parametrize("name", NAMES)
def test_layers_sum_to_the_unlayered_exact_film(name, mode):
    """2. a layered context and a separate unlayered exact context: the same states, counters and overflow, sum(layers) == film_fixed of the unlayered
    run, and film_fixed / film of the layered context are that same film"""
    ref, lay = fe._run(name), _layered_run(name, mode)
    D = fe.CASES[name]["max_depth"]
    assert lay["info"] == (mode, _table(mode, D)) and lay["layers"].shape == (len(_table(mode, D)), 96, 128, 3)
    _same_states(ref["cur"], lay["cur"])
    _same_states(ref["init"], lay["init"])
    assert ref["stats"] == lay["stats"] and ref["stats"]["steps"] == fe.CASES[name]["n"] * STEPS
    assert ref["overflow"] == lay["overflow"] == 0
    fe._assert_same_words(lay["layers"].sum(0), ref["fixed"])
    fe._assert_same_words(lay["fixed"], ref["fixed"])
    assert np.array_equal(lay["film"].view(np.uint32), ref["film"].view(np.uint32))


# ------------------------------------------------------------------------------------------------ 3. the two modes agree
@pytest.mark.parametrize("name", NAMES)
def test_modes_agree(name):
    """3. from two renders: length layer L equals the sum over l of the technique layers (L, l)"""
    by_len, by_tech = _layered_run(name, LENGTH), _layered_run(name, TECHNIQUE)
    table = by_tech["info"][1]
    for k, (L, _) in enumerate(by_len["info"][1]):
        members = [j for j, (c, l) in enumerate(table) if c + l - 1 == L]
        assert len(members) == L + 1
        fe._assert_same_words(by_len["layers"][k], by_tech["layers"][members].sum(0))


# ------------------------------------------------------------------------------------------------ 4. the labels against the read-out
@pytest.mark.parametrize("name", ["plain", "mux"])
def test_labels_against_the_read_out(name):
    """4. after step 1 from a clear film every chain has taken its unconditionally accepted large step (a = 1: the set-up marks the states invalid), so
    the film holds each chain's stored list exactly once, weighted by 1: the layered film equals the film rebuilt on the host from lmc_chain_splats of all
    chains -- values as stored, labels as stored, the probe's integer rule"""
    cfg = dict(fe.CASES[name], n=4096)
    ren = _layered(cfg, TECHNIQUE)
    ren.step(1)
    layers, over, stats = ren.film_layers_fixed(), ren.film_overflow(), ren.stats()
    counts, ent = ren.chain_splats(np.arange(cfg["n"]))
    rows = ren.chain_rows(np.arange(cfg["n"]))
    ren.close()
    assert stats["steps"] == stats["largeSteps"] == cfg["n"]
    assert np.array_equal(counts, rows[:, 15].astype(np.int32)) and counts.max() <= ent.shape[1]
    # (most bidirectional samples of a fresh large step carry no contribution: such a chain has a = 0, stores nothing and stays invalid)
    assert stats["accepted"] == int((counts > 0).sum()) > 0
    live = np.arange(ent.shape[1])[None, :] < counts[:, None]
    assert (ent[~live] == 0).all()
    e = ent[live]
    lab = e[:, 5].astype(np.int64)
    assert (lab >= 16).all() and np.array_equal(lab.astype(np.float32), e[:, 5])
    c, l = lab >> 4, lab & 15
    if name == "plain":
        assert counts.max() > 1 and len(set(zip(c.tolist(), l.tolist()))) >= 6, "test set-up: the lists carry too few techniques"
    else:  # one technique per multiplexed large step, the chain's own
        assert counts.max() == 1
    ci = np.repeat(np.arange(cfg["n"]), counts)  # the chain of every entry: the chain's own technique is one of its list's labels
    own = (c == rows[ci, 1].astype(np.int64)) & (l == rows[ci, 2].astype(np.int64))
    assert (np.bincount(ci, weights=own, minlength=cfg["n"])[counts > 0] >= 1).all()
    exp, n_over, n_outside, _ = _expected_layers(128, 96, TECHNIQUE, cfg["max_depth"], e[:, 0:2], e[:, 2:5], c, l)
    assert n_outside == 0 and over == n_over
    fe._assert_same_words(layers, exp)


# ------------------------------------------------------------------------------------------------ 5. layout and schedule
@pytest.mark.parametrize("env", [fe.RELOC, fe.NORELOC], ids=["relocated_resorted", "no_relocation"])
def test_layout_independence(env):
    """5a. chains relocated and fully re-sorted every 4th step, and not relocated at all: the words of the default layout, layer by layer (the labels
    are indexed by chain id: neither moves them)"""
    ren = _layered(fe.MALA4, TECHNIQUE, env=env)
    ren.step(STEPS)
    out = _layered_result(ren)
    reloc = ren.relocation_stats()
    ren.close()
    if env is fe.RELOC:
        assert reloc is not None and reloc["relocations"] > 0
    else:
        assert reloc is None
    fe._assert_same_words(_layered_run("mala4", TECHNIQUE)["layers"], out["layers"])


def test_run_to_run_and_schedule_independence():
    """5b. a second fresh context: the same words; with resident_steps set the mode keeps the context in lock step (as an open trace does): the same
    words, and lmc_resident_stats shows lock steps only"""
    ref = _layered_run("plain", TECHNIQUE)
    for resident in (0, 8):
        ren = _layered(fe.PLAIN, TECHNIQUE, resident=resident)
        ren.step(STEPS)
        out, rs = _layered_result(ren), ren.resident_stats()
        ren.close()
        assert rs["launches"] == 0 and rs["lock_steps"] == STEPS and rs["guard"] == 0, rs
        fe._assert_same_words(ref["layers"], out["layers"])
        assert out["stats"] == ref["stats"]


# ------------------------------------------------------------------------------------------------ 6. members
def test_group_members_sum_to_the_single_context():
    """6. three contexts on one device, after film_reduce(): every member holds the single context's layers, layer by layer"""
    p = gc.pkg()
    rens = [fe._renderer(**fe.MALA4) for _ in range(3)]
    for r in rens:
        r.set_option("film_layers", TECHNIQUE)
    g = p.Group(rens)
    g.init_chains(200000, fe.MALA4["n"], 64, 10 ** 6)
    g.step(STEPS)
    g.film_reduce()
    ref = _layered_run("mala4", TECHNIQUE)
    for r in rens:
        fe._assert_same_words(ref["layers"], r.film_layers_fixed())
        fe._assert_same_words(ref["fixed"], r.film_fixed())
        assert r.film_overflow() == 0
    for r in rens:
        r.close()


# ------------------------------------------------------------------------------------------------ 7. the split is real
def _init_techniques(ren):
    cap = 8 * 200000
    s, cl, ls = np.zeros(cap, np.int64), np.zeros(cap, np.int32), np.zeros(cap, np.float32)
    fn = gc.pkg().lib().lmc_init_contribs
    fn.restype = ctypes.c_longlong
    fn.argtypes = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    n = fn(ren.h, cap, gc.pkg().P(s), gc.pkg().P(cl), gc.pkg().P(ls))
    assert 0 < n <= cap
    return sorted(set((int(x) >> 4, int(x) & 15) for x in np.unique(cl[:n])))


def test_the_split_is_real():
    """7. the lengths the chain loop produces are those of MLTInit's contributions, inside the scene's depth range [max(mindepth, 3), maxdepth]: every
    other layer is all zero, every such length is populated, at maxdepth 6 at least two technique layers of one length are non-zero, and lmc_film_clear
    zeroes every layer"""
    ren = _layered(fe.PLAIN, TECHNIQUE)
    D, min_depth = fe.PLAIN["max_depth"], int(ren.get_option("mindepth"))
    tech = _init_techniques(ren)
    lengths = sorted(set(c + l - 1 for c, l in tech))
    lo = max(min_depth, 3)
    assert lengths and lo <= lengths[0] and lengths[-1] <= D, (lengths, lo, D)
    ren.step(STEPS)
    layers = ren.film_layers_fixed()
    table = ren.film_layer_info()[1]
    filled = [cl for cl, w in zip(table, layers) if w.any()]
    print("init lengths", lengths, "non-zero technique layers", filled)
    for (c, l), w in zip(table, layers):
        if not lo <= c + l - 1 <= D or (c + l - 1) not in lengths:
            assert not w.any(), (c, l)
    by_len = _layered_run("plain", LENGTH)["layers"]
    for L in range(1, D + 1):
        assert by_len[L - 1].any() == (L in lengths), L
    assert max(sum(1 for c, l in filled if c + l - 1 == L) for L in lengths) >= 2
    ren.film_clear()
    assert not ren.film_layers_fixed().any() and not ren.film_fixed().any() and ren.film_overflow() == 0
    ren.step(2)  # ... and goes on
    assert ren.film_layers_fixed().any()
    ren.close()


# ------------------------------------------------------------------------------------------------ 8. refusals
def test_refusals(tmp_path):
    """8. each returns -1 with a message naming film_layers, writes nothing, and leaves a context that still steps"""
    p = gc.pkg()
    small = dict(fe.PLAIN, n=1024)
    # without film_exact: lmc_chains_init names both options; the context is usable once one of them changes
    ren = fe._renderer(exact=0, **small)
    ren.set_option("film_layers", LENGTH)
    with pytest.raises(RuntimeError, match=r"(?s)film_layers.*film_exact"):
        ren.init_chains(200000, small["n"], 64, 10 ** 6)
    ren.set_option("film_exact", 1)
    ren.init_chains(200000, small["n"], 64, 10 ** 6)
    ren.step(2)
    # the mode is fixed once the chains are set up
    with pytest.raises(RuntimeError, match="film_layers"):
        ren.set_option("film_layers", TECHNIQUE)
    with pytest.raises(RuntimeError, match="film_layers"):
        ren.set_option("film_layers", 0)
    ren.set_option("film_layers", LENGTH)  # no change: accepted
    with pytest.raises(RuntimeError, match="film_layers"):
        ren.set_option("film_layers", 3)
    # a layer index outside [0, n_layers)
    n = len(ren.film_layer_info()[1])
    for k in (-1, n):
        with pytest.raises(RuntimeError, match=r"film_layers"):
            ren.film_layer_fixed(k)
        with pytest.raises(RuntimeError, match=r"film_layers"):
            ren.film_layer(k)
    # checkpoints
    ck = str(tmp_path / "l.ckpt")
    with pytest.raises(RuntimeError, match="film_layers"):
        ren.save_checkpoint(ck)
    assert not os.path.exists(ck) and not os.path.exists(ck + ".tmp")
    un = fe._fresh(small)
    un.step(2)
    un.save_checkpoint(ck)
    before = ren.film_layers_fixed()
    with pytest.raises(RuntimeError, match="film_layers"):
        ren.load_checkpoint(ck)
    fe._assert_same_words(before, ren.film_layers_fixed())
    g = p.Group([ren])
    with pytest.raises(RuntimeError, match="film_layers"):
        g.save_checkpoint(ck + "g")
    with pytest.raises(RuntimeError, match="film_layers"):
        g.load_checkpoint(ck)
    assert not os.path.exists(ck + "g")
    ren.step(2)
    assert ren.stats()["steps"] == 4 * small["n"] and ren.film_layers_fixed().any()
    # the layer readers on an unlayered context
    assert un.film_layer_info() == (0, [])
    for call in (lambda: un.film_layer(0), lambda: un.film_layer_fixed(0), un.film_layers_fixed):
        with pytest.raises(RuntimeError, match="film_layers"):
            call()
    counts, ent = un.chain_splats([0, 5, 5, 1023])
    assert (ent[np.arange(ent.shape[1])[None, :] < counts[:, None]][:, 5] == -1).all() and np.array_equal(ent[1], ent[2])
    with pytest.raises(RuntimeError, match="chain id"):
        un.chain_splats([1024])
    un.step(1)
    un.close()
    ren.close()
    # H2MC contexts
    h2 = fe._renderer(**fe.H2)
    h2.set_option("film_layers", TECHNIQUE)
    with pytest.raises(RuntimeError, match=r"(?s)film_layers.*H2MC"):
        h2.init_chains(200000, fe.H2["n"], 64, 10 ** 6)
    h2.set_option("film_layers", 0)
    h2.init_chains(200000, fe.H2["n"], 64, 10 ** 6)
    h2.step(1)
    h2.close()
    # a group with mixed modes, by the package and by the library itself
    rens = [fe._renderer(**small), fe._renderer(**small)]
    rens[0].set_option("film_layers", TECHNIQUE)
    with pytest.raises(RuntimeError, match="film_layers"):
        p.Group(rens).init_chains(200000, small["n"], 64, 10 ** 6)
    arr = (p.vp * 2)(*[r.h for r in rens])
    L = p.lib()
    L.lmc_group_chains_init.argtypes = [p.vp, p.ctypes.c_int, p.c_ll, p.ctypes.c_int, p.ctypes.c_int, p.c_ll, p.c_ll]
    assert L.lmc_group_chains_init(arr, 2, 200000, small["n"], 64, 10 ** 6, 0) != 0 and "film_layers" in L.lmc_last_error().decode()
    rens[1].set_option("film_layers", TECHNIQUE)
    g = p.Group(rens)
    g.init_chains(200000, small["n"], 64, 10 ** 6)
    g.step(2)
    g.film_reduce()
    fe._assert_same_words(rens[0].film_layers_fixed(), rens[1].film_layers_fixed())
    for r in rens:
        r.close()


def test_allreduce_of_more_than_one_rank_is_refused(tmp_path):
    """8. lmc_film_allreduce on a communicator of two ranks (two processes over the stand-in for librccl of tests/test_gpu_film_exact.py): -1 naming
    film_layers on both, nothing reduced, and both contexts still step"""
    worker = os.path.join(gc.ROOT, "tests", "helpers", "rank_worker_film_layers.py")
    env = dict(os.environ, LMC_RCCL_LIB=fe._rccl_stub_i64())
    procs = [subprocess.Popen([sys.executable, worker, str(r), "2", str(tmp_path)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
             for r in range(2)]
    outs = []
    for q in procs:
        try:
            outs.append(q.communicate(timeout=120)[0])
        except subprocess.TimeoutExpired:
            q.kill()
            outs.append(q.communicate()[0] + "\n[timed out]")
    assert all(q.returncode == 0 for q in procs), outs
    for o in outs:
        assert "refused: " in o and "film_layers" in o and "still steps" in o, o


# ------------------------------------------------------------------------------------------------ 9. the command line
def test_dpt_amd_film_layers(tmp_path):
    """9. dpt_amd --film-layers technique on the 128 x 96 torus: the main EXR byte-equal to an --exact-film run's, one file per non-empty layer beside it;
    with --devices 0,0 the same bytes; --checkpoint with it is an error at start"""
    assert os.path.exists(fe.CLI), "dpt_amd not built"

    def run(d, *flags):
        before = set(os.listdir(d))
        r = subprocess.run([fe.CLI, "--chains", "4096"] + list(flags) + [os.path.join(d, "lmc.xml")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
        assert r.returncode == 0 and r.stdout.rstrip().endswith("Done!"), r.stdout
        new = sorted(f for f in set(os.listdir(d)) - before if f.endswith(".exr"))
        main = [f for f in new if f.endswith("s.exr")]
        assert len(main) == 1, (new, r.stdout)
        stem = main[0][:-4]
        return r.stdout, open(os.path.join(d, main[0]), "rb").read(), {f[len(stem):-4]: open(os.path.join(d, f), "rb").read() for f in new if f != main[0]}

    for k in "abc":
        fe._small_scene(tmp_path / k, width=128, height=96, spp=32)
    _, a, extra_a = run(str(tmp_path / "a"), "--exact-film")
    assert len(a) > 1000 and not extra_a
    out_b, b, layers_b = run(str(tmp_path / "b"), "--film-layers", "technique")
    assert "Exact film" in out_b and "Layered film (by technique)" in out_b
    assert b == a
    assert len(layers_b) >= 6 and all(t.startswith("_c") and "_l" in t for t in layers_b), sorted(layers_b)
    assert "%d of" % len(layers_b) in out_b
    _, c, layers_c = run(str(tmp_path / "c"), "--film-layers", "technique", "--devices", "0,0")
    assert c == a and layers_c == layers_b
    r = subprocess.run([fe.CLI, "--film-layers", "length", "--checkpoint", str(tmp_path / "x.ckpt"), os.path.join(str(tmp_path / "a"), "lmc.xml")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=60)
    assert r.returncode != 0 and "--film-layers" in r.stdout and not os.path.exists(tmp_path / "x.ckpt")
    h = subprocess.run([fe.CLI, "--help"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert "--film-layers" in h.stdout
