"""Exact film (include/lmc_abi.h "Exact film", langevin-mcmc_amd/csrc/device/dchain.h Splat, INTEGRATION.md "Exact film"): with film_exact = 1 the MLT film
is accumulated in 64-bit fixed point with integer atomics, so it is a pure function of the chains' trajectories.  Every comparison of two exact films
here is WORD FOR WORD (np.array_equal of int64): run to run, across slot layouts and schedules, across in-process members and rank processes, across a
checkpoint.  Shapes are those of tests/test_gpu_checkpoint.py: the torus at 128 x 96, force_diffuse, 4096 chains (plain MLT, H2MC) or 16384 chains at
maxdepth 4 (`FILL`: both cache dims fill within ~25 steps), 30 steps.  The option dictionaries are copies of that file's."""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import gpu_checks as gc
from tests.test_gpu_relocate import _same_states

pytestmark = pytest.mark.gpu
CLI = os.path.join(gc.ROOT, "langevin-mcmc_amd", "dpt_amd")
FILL = {"largestepprob": 0.5, "largestepscale": 1.0}
PLAIN = dict(opts={"largestepprob": 0.3, "largestepscale": 1.0}, mala=False, max_depth=6, n=4096)
MALA4 = dict(opts=FILL, mala=True, max_depth=4, n=16384)
H2 = dict(opts={"h2mc": 1, "largestepprob": 0.2, "perturbstddev": 0.01}, mala=True, max_depth=6, n=4096)
CASES = {
    "plain": PLAIN,
    "mala4": MALA4,  # k_mala_finish / the lean-gradient launch while the caches fill, then the lean kernel; the large step throughout
    "mux": dict(MALA4, opts=dict(FILL, largestepmultiplexed=1)),
    "samplecache": dict(MALA4, opts=dict(FILL, samplecache=1, largestepmultiplexed=1)),
    "h2": H2,  # k_h2_finish
}
COUNTERS = ("steps", "largeSteps", "accepted", "gradCalls", "cacheQueries", "cacheHits", "resets", "cacheReadyMask")
RELOC, NORELOC = {"LMC_RELOCATE": "1", "LMC_RESORT_EVERY": "4"}, {"LMC_RELOCATE": "0", "LMC_RESORT_EVERY": "0"}
STEPS = 30


class _Env:
    def __init__(self, env):
        self.env = env or {}

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _renderer(opts, mala, max_depth, exact=1, resident=0, width=128, **_):
    ren = gc.pkg().Renderer(gc.TORUS, force_diffuse=1, max_depth=max_depth, width=width, height=96, seed_offset=0, use_gradient=1)
    for k, v in opts.items():
        ren.set_option(k, v)
    if not mala:
        ren.set_option("mala", 0)
    if resident:
        ren.set_option("resident_steps", resident)
    ren.set_option("film_exact", exact)
    return ren


def _fresh(cfg, exact=1, env=None, resident=0):
    with _Env(env):
        ren = _renderer(exact=exact, resident=resident, **cfg)
        ren.init_chains(200000, cfg["n"], 64, 10 ** 6)
    return ren


def _result(ren, exact=1):
    st = ren.stats()
    out = dict(cur=ren.summary(0).copy(), init=ren.summary(1).copy(), stats={k: st[k] for k in COUNTERS}, film=ren.film().copy(), overflow=ren.film_overflow())
    if exact:
        out["fixed"] = ren.film_fixed().copy()
    return out


@functools.lru_cache(maxsize=None)
def _run(name, exact=1):
    """the reference run of a case, computed once and shared (and never written to): the configuration stepped straight through"""
    ren = _fresh(CASES[name], exact)
    ren.step(STEPS)
    out = _result(ren, exact)
    ren.close()
    return out


def _assert_same_words(a, b):
    assert a.dtype == b.dtype == np.int64 and a.shape == b.shape
    assert np.array_equal(a, b), "%d of %d words differ" % (int((a != b).sum()), a.size)


# ------------------------------------------------------------------------------------------------ 1. the splat routine against integers
def _probe_splats():
    rng = np.random.default_rng(20261)
    n, W, H = 4096, 4, 3
    xy = rng.random((n, 2), dtype=np.float32)
    xy[:1500] = np.float32([0.6, 0.4]) + rng.random((1500, 2), dtype=np.float32) * np.float32(0.1)  # pixel (ix 2, iy 1): at least 1024 splats on one pixel
    k = rng.integers(-40, 21, (n, 3))
    m = 1.0 + rng.random((n, 3))
    v = (rng.choice([-1.0, 1.0], (n, 3)) * np.ldexp(m, k)).astype(np.float32)
    bad = rng.choice(n, 24, replace=False)
    v[bad[0], 0], v[bad[1], 1], v[bad[2], 2] = np.nan, np.inf, -np.inf
    v[bad[3]] = [np.nan, 2.0 ** 31, 1.0]  # non-finite wins: dropped, not counted
    v[bad[4], 1] = np.float32(2.0 ** 30)  # exactly at the limit: out of range
    v[bad[5], 0] = -np.float32(2.0 ** 30)
    v[bad[6], 2] = np.float32(2.0 ** 30) * (1 - 2.0 ** -24)  # the float below it: in range
    v[bad[7], 0] = -np.float32(2.0 ** 30) * (1 - 2.0 ** -24)
    v[bad[8]] = [3e38, -3e38, 1e35]
    v[bad[9], 2] = np.float32(2.0 ** 40)
    v[bad[10], 1] = -np.float32(2.0 ** 62)
    return W, H, xy, v


def _probe_expectation(W, H, xy, v):
    finite = np.isfinite(v).all(axis=1)
    in_range = (np.abs(v) < np.float32(2.0 ** 30)).all(axis=1)
    ix = np.clip((xy[:, 0] * np.float32(W)).astype(np.int32), 0, W - 1)  # float32 products, truncated: the device's pixel rule
    iy = np.clip((xy[:, 1] * np.float32(H)).astype(np.int32), 0, H - 1)
    keep = finite & in_range
    q = np.rint(v[keep].astype(np.float64) * 2.0 ** 32).astype(np.int64)
    exp = np.zeros((H, W, 3), np.int64)
    np.add.at(exp, (iy[keep], ix[keep]), q)
    return exp, int((finite & ~in_range).sum()), ix, iy


def test_probe_against_integers():
    """1. 4096 splats onto a 4 x 3 film through the device's Splat, one launch, 64-thread blocks; components +-2^k m (k in [-40, 20], m in [1, 2)), a
    handful non-finite, a handful at or above 2^30.  The words equal the numpy integers BIT FOR BIT; the overflow count is the number of finite
    out-of-range splats; three permutations of the list give the same words; the float view is np.float32(np.float64(q) * 2^-32) exactly."""
    W, H, xy, v = _probe_splats()
    exp, n_over, ix, iy = _probe_expectation(W, H, xy, v)
    assert np.bincount(iy * W + ix, minlength=W * H).max() >= 1024 and n_over >= 5 and (exp != 0).all()
    fx, fl, over = gc.pkg().film_splat_probe(W, H, xy, v, exact=True)
    _assert_same_words(fx, exp)
    assert over == n_over
    assert np.array_equal(fl.view(np.uint32), np.float32(np.float64(exp) * 2.0 ** -32).view(np.uint32))
    rng = np.random.default_rng(7)
    for _ in range(3):
        perm = rng.permutation(len(v))
        fx2, fl2, over2 = gc.pkg().film_splat_probe(W, H, xy[perm], v[perm], exact=True)
        _assert_same_words(fx2, exp)
        assert over2 == n_over and np.array_equal(fl2.view(np.uint32), fl.view(np.uint32))
    # the float film of the same list: same pixel rule, nothing dropped by range, non-finite splats dropped
    _, ff, over0 = gc.pkg().film_splat_probe(W, H, xy[:2048], np.clip(np.nan_to_num(v[:2048], nan=0.0, posinf=0.0, neginf=0.0), -1e3, 1e3), exact=False)
    assert over0 == 0 and np.isfinite(ff).all()


# ------------------------------------------------------------------------------------------------ 2. run to run
@pytest.mark.parametrize("name", list(CASES))
def test_run_to_run_equality(name):
    """2. two fresh contexts with the same options: film_fixed() word for word, film_overflow() == 0 (every splatting kernel is on the path of one case)"""
    a = _run(name)
    ren = _fresh(CASES[name])
    ren.step(STEPS)
    b = _result(ren)
    ren.close()
    assert a["stats"]["steps"] == CASES[name]["n"] * STEPS and np.abs(a["fixed"]).sum() > 0
    if name in ("mala4", "mux", "samplecache"):
        assert a["stats"]["cacheReadyMask"] != 0 and a["stats"]["gradCalls"] > 0, "test set-up: the cache never filled"
    assert a["overflow"] == 0 and b["overflow"] == 0
    _assert_same_words(a["fixed"], b["fixed"])
    assert np.array_equal(a["film"].view(np.uint32), np.float32(np.float64(a["fixed"]) * 2.0 ** -32).view(np.uint32))


# ------------------------------------------------------------------------------------------------ 3. the mode does not touch a trajectory
@pytest.mark.parametrize("name", ["plain", "mala4"])
def test_mode_independence_of_the_chains(name):
    """3. film_exact = 0 against 1 on the same run: identical summary(0), summary(1) and counters; the luminance of the exact film's float view within
    1e-5 of the float film's norm (the bar tests/test_gpu_checkpoint.py sets between two float films)"""
    e, f = _run(name), _run(name, 0)
    assert np.array_equal(e["cur"].view(np.uint32), f["cur"].view(np.uint32))
    assert np.array_equal(e["init"].view(np.uint32), f["init"].view(np.uint32))
    assert e["stats"] == f["stats"]
    assert f["overflow"] == 0
    le, lf = gc.lum(e["film"]), gc.lum(f["film"])
    print("exact vs float film luminance: |d| / |f| = %.3g" % (np.linalg.norm(le - lf) / np.linalg.norm(lf)))
    assert np.isfinite(le).all() and np.linalg.norm(le - lf) <= 1e-5 * np.linalg.norm(lf)


def test_the_mode_is_fixed_once_the_chains_are_set_up():
    ren = _fresh(dict(PLAIN, n=1024))
    with pytest.raises(RuntimeError, match="film_exact"):
        ren.set_option("film_exact", 0)
    assert ren.get_option("film_exact") == 1
    ren.set_option("film_exact", 1)  # no change: accepted
    ren.step(2)  # still usable
    assert ren.film_overflow() == 0 and np.abs(ren.film_fixed()).sum() > 0
    ren.close()
    ren = _fresh(dict(PLAIN, n=1024), exact=0)
    with pytest.raises(RuntimeError, match="float film"):
        ren.film_fixed()
    ren.close()


# ------------------------------------------------------------------------------------------------ 4. layout and schedule
@pytest.mark.parametrize("env", [RELOC, NORELOC], ids=["relocated_resorted", "no_relocation"])
def test_layout_independence(env):
    """4a. chains relocated and fully re-sorted every 4th step, and not relocated at all: the words of the default layout"""
    ren = _fresh(MALA4, env=env)
    ren.step(STEPS)
    out = _result(ren)
    ren.close()
    assert out["overflow"] == 0
    _assert_same_words(_run("mala4")["fixed"], out["fixed"])


@pytest.mark.parametrize("name", ["plain", "mala4"])
def test_schedule_independence(name):
    """4b. resident_steps 8 against lock step (plain MLT: resident from the first step; MALA: once the caches are frozen)"""
    ren = _fresh(CASES[name], resident=8)
    ren.step(STEPS)
    out, rs = _result(ren), ren.resident_stats()
    ren.close()
    assert rs["launches"] > 0 and rs["guard"] == 0, rs
    _assert_same_words(_run(name)["fixed"], out["fixed"])


# ------------------------------------------------------------------------------------------------ 5. members
@pytest.mark.parametrize("members", [2, 3])
def test_group_members_sum_to_the_single_context(members):
    """5. groups of 2 and 3 contexts on one device, after film_reduce(): every member holds the single context's words"""
    p = gc.pkg()
    rens = [_renderer(**MALA4) for _ in range(members)]
    g = p.Group(rens)
    g.init_chains(200000, MALA4["n"], 64, 10 ** 6)
    g.step(STEPS)
    assert g.film_overflow() == 0
    g.film_reduce()
    ref = _run("mala4")
    for r in rens:
        _assert_same_words(ref["fixed"], r.film_fixed())
    assert np.array_equal(rens[0].film().view(np.uint32), ref["film"].view(np.uint32))
    for r in rens:
        r.close()


def test_a_group_with_mixed_modes_is_refused_and_stays_usable():
    p = gc.pkg()
    small = dict(PLAIN, n=2048)
    rens = [_renderer(exact=1, **small), _renderer(exact=0, **small)]
    with pytest.raises(RuntimeError, match="film_exact"):
        p.Group(rens).init_chains(200000, small["n"], 64, 10 ** 6)
    arr = (p.vp * 2)(*[r.h for r in rens])  # ... and the library itself, without the package's own check in front
    L = p.lib()
    L.lmc_group_chains_init.argtypes = [p.vp, p.ctypes.c_int, p.c_ll, p.ctypes.c_int, p.ctypes.c_int, p.c_ll, p.c_ll]
    assert L.lmc_group_chains_init(arr, 2, 200000, small["n"], 64, 10 ** 6, 0) != 0 and "film_exact" in L.lmc_last_error().decode()
    rens[1].set_option("film_exact", 1)  # no chains were set up: the mode can still change
    g = p.Group(rens)
    g.init_chains(200000, small["n"], 64, 10 ** 6)
    g.step(3)
    g.film_reduce()
    _assert_same_words(rens[0].film_fixed(), rens[1].film_fixed())
    assert np.abs(rens[0].film_fixed()).sum() > 0
    for r in rens:
        r.close()


# ------------------------------------------------------------------------------------------------ 6. checkpoint
@pytest.mark.parametrize("save_at", [12, 28])
@pytest.mark.parametrize("members", [1, 2])
def test_checkpoint_resumes_to_the_same_words(tmp_path, save_at, members):
    """6. saved at step 12 of 30 (inside the cache fill) and at step 28, resumed in a fresh context and in a group of 2: the final words equal the
    uninterrupted run's, and the overflow counter reads 0 after the load as it did before the save (a non-zero counter cannot be produced by a render of
    the shipped scenes, so its way through a file is not exercised here)"""
    p = gc.pkg()
    ref, path = _run("mala4"), str(tmp_path / "e.ckpt")
    ren = _fresh(MALA4)
    ren.step(save_at)
    if save_at == 12:
        assert ren.stats()["cacheReadyMask"] != ref["stats"]["cacheReadyMask"], "test set-up: the save is not inside the fill"
    ren.save_checkpoint(path)
    at_save = ren.film_fixed().copy()
    ren.close()
    info = p.checkpoint_info(path)
    assert info["film_format"] == "fixed64" and info["version"] == 2 and info["steps_done"] == save_at
    rens = [_renderer(**MALA4) for _ in range(members)]
    if members == 1:
        rens[0].load_checkpoint(path)
        _assert_same_words(at_save, rens[0].film_fixed())
        rens[0].step(STEPS - save_at)
    else:
        g = p.Group(rens)
        g.load_checkpoint(path)
        g.step(STEPS - save_at)
        g.film_reduce()
    assert sum(r.film_overflow() for r in rens[:1]) == 0
    _assert_same_words(ref["fixed"], rens[0].film_fixed())
    _same_states(ref["cur"], np.concatenate([r.summary(0) for r in rens]))
    for r in rens:
        r.close()


def test_checkpoint_modes_do_not_mix_and_float_files_are_unchanged(tmp_path):
    """6. an exact-mode file is refused by a float-mode context and the reverse, with both modes named, and both contexts stay usable; the film section
    of a float-mode file is film().tobytes() (format version 1, as before)"""
    p = gc.pkg()
    small = dict(PLAIN, n=1024)
    pe, pf = str(tmp_path / "e.ckpt"), str(tmp_path / "f.ckpt")
    fixed, flt = {}, {}
    for exact, path, res in ((1, pe, fixed), (0, pf, flt)):
        ren = _fresh(small, exact)
        ren.step(3)
        ren.save_checkpoint(path)
        res["film_at_save"] = ren.film().copy()
        ren.step(4)
        res["cur"] = ren.summary(0).copy()
        if exact:
            res["fixed"] = ren.film_fixed().copy()
        ren.close()
    info = p.checkpoint_info(pf)
    assert info["film_format"] == "float32" and info["version"] == 1
    blob = open(pf, "rb").read()
    end = 176 + info["job_bytes"]  # header | job-wide section, the film last | records
    assert blob[end - flt["film_at_save"].nbytes:end] == flt["film_at_save"].tobytes()
    assert len(blob) == info["total_bytes"]
    for exact, wrong, right, res in ((0, pe, pf, flt), (1, pf, pe, fixed)):
        ren = _renderer(exact=exact, **small)
        with pytest.raises(RuntimeError, match=r"(?s)fixed-point.*float32|float32.*fixed-point"):
            ren.load_checkpoint(wrong)
        ren.load_checkpoint(right)  # still usable: ends where the saving run ended
        ren.step(4)
        assert np.array_equal(ren.summary(0).view(np.uint32), res["cur"].view(np.uint32))
        if exact:
            _assert_same_words(res["fixed"], ren.film_fixed())
        ren.close()


# ------------------------------------------------------------------------------------------------ 7. against the oracle
def test_exact_film_against_the_oracle():
    """7. the configuration of tests/test_gpu_checkpoint.py::test_resume_against_the_oracle (plain-MLT torus, 160 x 120, use_gradient = 0), film_exact = 1: chain
    states exact as there, the luminance of the exact film's float view within that test's bar of the oracle's film"""
    cfg = gc.oracle_run_config(160, 120, 40000, 256, 8, 400, 40, mala=False)
    o = gc.oracle_run(cfg, "")
    ren = gc.pkg().Renderer(gc.TORUS, force_diffuse=1, max_depth=6, width=160, height=120, seed_offset=0, use_gradient=0)
    ren.set_option("mala", 0)
    ren.set_option("film_exact", 1)
    norm, contribs = ren.init_chains(40000, 256, 8, 400)
    ren.step(40)
    sg, cg, gi, fg, over = ren.stats(), ren.summary(0), ren.summary(1), ren.film(), ren.film_overflow()
    ren.close()
    assert contribs == o["contribs"] and norm == o["norm"] and over == 0
    si, co = o["init_summary"], o["summary"]
    assert np.array_equal(si[:, 1:4], gi[:, 1:4]) and np.array_equal(si[:, 16:], gi[:, 16:])
    so = o["stats"]
    assert sg["steps"] == so["steps"] == 256 * 40
    for k in ("largeSteps", "accepted", "resets"):
        assert sg[k] == so[k], k
    same = (co[:, 0] == cg[:, 0]) & (co[:, 1] == cg[:, 1]) & (co[:, 2] == cg[:, 2]) & (np.abs(co[:, 3] - cg[:, 3]) <= 1e-3 * np.abs(co[:, 3]) + 1e-12)
    assert same.all()
    lo, lg = gc.lum(o["film"]), gc.lum(fg)
    print("exact film vs oracle film luminance: |d| / |o| = %.3g" % (np.linalg.norm(lo - lg) / np.linalg.norm(lo)))
    assert np.linalg.norm(lo - lg) < 1e-4 * np.linalg.norm(lo)
    assert abs(lg.sum() / (norm * sg["weightSum"]) - 1.0) < 1e-4


# ------------------------------------------------------------------------------------------------ 8. rank processes
def _rccl_stub_i64():
    so = os.path.join(gc.ROOT, "tests", "helpers", "librccl_stub_i64.so")
    src = os.path.join(gc.ROOT, "tests", "helpers", "rccl_stub_i64.cpp")
    if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
        subprocess.check_call(["hipcc", "-O2", "-std=c++17", "-fPIC", "-shared", src, "-o", so, "-lrt"], cwd=gc.ROOT)
    return so


@pytest.mark.parametrize("world", [2, 3])
def test_rank_processes_allreduce_int64(tmp_path, world):
    """8. 2 and 3 rank PROCESSES on the one GPU over tests/helpers/rccl_stub_i64.cpp (a stand-in for librccl that also reduces ncclInt64), 96 x 72 film:
    after lmc_film_allreduce every rank's film_fixed() equals the one-rank run's, and the sum of the ranks' own words"""
    n, steps, ninit, streams = 1 << 14, 30, 1 << 17, 2048
    one = gc.pkg().Renderer(gc.TORUS, force_diffuse=1, max_depth=6, width=96, height=72, seed_offset=0, use_gradient=1)
    one.set_option("film_exact", 1)
    one.init_chains(ninit, n, streams, steps, 0)
    one.step(steps)
    fixed1, film1, over1 = one.film_fixed(), one.film(), one.film_overflow()
    one.close()
    assert over1 == 0
    env = dict(os.environ, LMC_RCCL_LIB=_rccl_stub_i64())
    worker = os.path.join(gc.ROOT, "tests", "helpers", "rank_worker_exact.py")
    procs = [subprocess.Popen([sys.executable, worker, str(r), str(world), str(tmp_path), str(n), str(steps), str(ninit), str(streams)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
             for r in range(world)]  # (the ranks of one job are collective: they start together; each gets its own time limit below)
    outs, failed = [], False
    for q in procs:
        if failed:  # a failed rank ends the job: its peers would wait at a collective for ever
            q.kill()
            outs.append(q.communicate()[0])
            continue
        try:
            outs.append(q.communicate(timeout=180)[0])
        except subprocess.TimeoutExpired:
            q.kill()
            outs.append(q.communicate()[0] + "\n[timed out]")
        failed = q.returncode != 0
    assert all(q.returncode == 0 for q in procs), outs
    R = [np.load(tmp_path / ("rank%d.npz" % r)) for r in range(world)]
    own = sum(x["own"] for x in R)
    for x in R:
        _assert_same_words(fixed1, x["fixed"])
        _assert_same_words(own, x["fixed"])
        assert int(x["overflow"]) == 0 and np.array_equal(x["film"].view(np.uint32), film1.view(np.uint32))


# ------------------------------------------------------------------------------------------------ 9. the command line
def _small_scene(d, width=96, height=72, spp=64):
    """the shipped scene file with a smaller film and budget (as tests/test_gpu_checkpoint.py reduces it)"""
    xml = open(gc.TORUS).read()
    xml = xml.replace('<integer name="height" value="768"/>', '<integer name="height" value="%d"/>' % height)
    xml = xml.replace('<integer name="width" value="1024"/>', '<integer name="width" value="%d"/>' % width)
    xml = re.sub(r'<integer name="spp"\s+value="245"/>', '<integer name="spp" value="%d"/>' % spp, xml)
    assert 'value="%d"' % spp in xml and 'value="%d"' % width in xml
    os.makedirs(d)
    os.symlink(os.path.join(gc.ROOT, "scenes", "torus", "data"), d / "data")
    (d / "lmc.xml").write_text(xml)
    return str(d / "lmc.xml")


def test_dpt_amd_exact_film_writes_the_same_bytes(tmp_path):
    """9. dpt_amd --exact-film twice: byte-identical EXR files; cut by --checkpoint F --max-steps S and finished by --resume F (the mode comes from the
    file): the same bytes again; --exact-film on a float-film checkpoint is an error"""
    assert os.path.exists(CLI), "dpt_amd not built"

    def run(d, *flags, ok=True):
        before = set(os.listdir(d))
        r = subprocess.run([CLI, "--chains", "4096"] + list(flags) + [os.path.join(d, "lmc.xml")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
        if not ok:
            return r
        assert r.returncode == 0 and r.stdout.rstrip().endswith("Done!"), r.stdout
        new = [f for f in set(os.listdir(d)) - before if f.endswith(".exr")]
        assert len(new) == 1, (new, r.stdout)
        return r.stdout, open(os.path.join(d, new[0]), "rb").read()

    for k in "abc":
        _small_scene(tmp_path / k)
    out_a, a = run(str(tmp_path / "a"), "--exact-film")
    assert "Exact film" in out_a
    _, b = run(str(tmp_path / "b"), "--exact-film")
    assert len(a) > 1000 and a == b
    ck = str(tmp_path / "c" / "render.ckpt")
    out1, part = run(str(tmp_path / "c"), "--exact-film", "--checkpoint", ck, "--max-steps", "40")
    assert "Checkpoint after 40 of" in out1 and gc.pkg().checkpoint_info(ck)["film_format"] == "fixed64" and part != a
    out2, c = run(str(tmp_path / "c"), "--resume", ck)
    assert "Resumed" in out2 and "Exact film" in out2
    assert c == a
    fck = str(tmp_path / "c" / "float.ckpt")
    run(str(tmp_path / "c"), "--checkpoint", fck, "--max-steps", "8")
    r = run(str(tmp_path / "c"), "--exact-film", "--resume", fck, ok=False)
    assert r.returncode != 0 and "float film" in r.stdout
