"""Checkpoint and resume (include/lmc_abi.h lmc_checkpoint_*, langevin-mcmc_amd/csrc/device/checkpoint.hip, INTEGRATION.md "Checkpoint and resume").
The reference has no restart file, so the contract checked here is the project's own: a render that is saved between two steps, closed, and
loaded into a NEW context (another slot layout, another schedule, another number of in-process members) ends in the states the uninterrupted
render ends in.  "Same" is _same_states of tests/test_gpu_relocate.py -- valid rows word for word, technique and lsScore of invalid rows,
sampleIdx -- plus equal integer counters, weightSum to rel 1e-6 and film luminance to 1e-5 of its norm (the order of the float atomics).
Every run: the torus at 128 x 96, force_diffuse, chain counts and steps of the relocation / resident tests."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from tests import gpu_checks as gc
from tests.test_gpu_relocate import _same_states

pytestmark = pytest.mark.gpu
CLI = os.path.join(gc.ROOT, "langevin-mcmc_amd", "dpt_amd")
FILL = {"largestepprob": 0.5, "largestepscale": 1.0}  # maxdepth 4: two cache dims (6, 8), both full after ~25 steps of 16384 chains
PLAIN = dict(opts={"largestepprob": 0.3, "largestepscale": 1.0}, mala=False, max_depth=6, n=4096)
MALA4 = dict(opts=FILL, mala=True, max_depth=4, n=16384)
H2 = dict(opts={"h2mc": 1, "largestepprob": 0.2, "perturbstddev": 0.01}, mala=True, max_depth=6, n=4096)
COUNTERS = ("steps", "largeSteps", "accepted", "gradCalls", "cacheQueries", "cacheHits", "resets")


class _Env:
    """variables the library reads when a context is created or its chains are set up (LMC_RELOCATE, LMC_RESORT_EVERY)"""

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


def _renderer(opts, mala, max_depth, width=128, resident=0, **_):
    ren = gc.pkg().Renderer(gc.TORUS, force_diffuse=1, max_depth=max_depth, width=width, height=96, seed_offset=0, use_gradient=1)
    for k, v in opts.items():
        ren.set_option(k, v)
    if not mala:
        ren.set_option("mala", 0)
    if resident:
        ren.set_option("resident_steps", resident)
    return ren


def _fresh(cfg, env=None, resident=0):
    with _Env(env):
        ren = _renderer(resident=resident, **cfg)
        ren.norm, _ = ren.init_chains(200000, cfg["n"], 64, 10 ** 6)
    return ren


def _loaded(cfg, path, env=None, resident=0):
    with _Env(env):
        ren = _renderer(resident=resident, **cfg)
        ren.norm = ren.load_checkpoint(path)
    return ren


def _result(rens, group=None):
    """states in chain order, counters summed over the members, the film (after the group's merge)"""
    sts = [r.stats() for r in rens]
    st = {k: sum(s[k] for s in sts) for k in COUNTERS + ("weightSum",)}
    assert all(s["cacheReadyMask"] == sts[0]["cacheReadyMask"] for s in sts)
    st["cacheReadyMask"] = sts[0]["cacheReadyMask"]
    cur = np.concatenate([r.summary(0) for r in rens])
    if group is not None:
        group.film_reduce()
    return dict(cur=cur, stats=st, film=rens[0].film().copy(), norm=rens[0].norm)


def _assert_same(a, b):
    _same_states(a["cur"], b["cur"])
    for k in COUNTERS + ("cacheReadyMask",):  # all eight stats keys
        assert a["stats"][k] == b["stats"][k], (k, a["stats"][k], b["stats"][k])
    assert b["stats"]["weightSum"] == pytest.approx(a["stats"]["weightSum"], rel=1e-6)
    assert a["norm"] == b["norm"]
    la, lb = gc.lum(a["film"]), gc.lum(b["film"])
    assert np.isfinite(lb).all()
    assert np.linalg.norm(la - lb) <= 1e-5 * np.linalg.norm(la)


@functools.lru_cache(maxsize=None)
def _uninterrupted(name, steps):
    """the reference of a case, computed once and shared: the same configuration stepped straight through"""
    cfg = {"plain": PLAIN, "mala4": MALA4, "h2": H2}[name]
    ren = _fresh(cfg)
    ren.step(steps)
    out = _result([ren])
    ren.close()
    return out


def _interrupted(cfg, steps, save_at, path, save_env=None, load_env=None, save_resident=0, load_resident=0, check_at_save=None):
    ren = _fresh(cfg, save_env, save_resident)
    ren.step(save_at)
    if check_at_save:
        check_at_save(ren)
    init_states = ren.summary(1).copy()
    ren.save_checkpoint(path)
    ren.close()
    ren = _loaded(cfg, path, load_env, load_resident)
    assert np.array_equal(ren.summary(1).view(np.uint32), init_states.view(np.uint32)), "the init states did not travel"
    info = gc.pkg().checkpoint_info(path)
    assert info["steps_done"] == save_at and info["n_chains_total"] == cfg["n"] and info["wall_seconds"] > 0
    ren.step(steps - save_at)
    out = _result([ren])
    ren.close()
    return out


def test_plain_mlt_resumes_exactly(tmp_path):
    """1. 4096 chains x 40 steps against 13 steps, save, close, a new Renderer, load, 27 steps; the init states are the same right after the load"""
    _assert_same(_uninterrupted("plain", 40), _interrupted(PLAIN, 40, 13, str(tmp_path / "c.ckpt")))


@pytest.mark.parametrize("save_at", [8, 40])
def test_mala_resumes_through_and_after_the_cache_fill_phase(tmp_path, save_at):
    """2. MALA at maxdepth 4, 16384 chains x 72 steps: saved at step 8 a cache is still filling and gradients are being evaluated (rows, fill counts,
    moment vectors and stored Gaussians travel; the dims become ready in the same step after the load); saved at step 40 the caches are ready
    (their kd-trees and existence grids are rebuilt on load)"""
    ref = _uninterrupted("mala4", 72)
    assert ref["stats"]["cacheReadyMask"] != 0, "test set-up: the cache never filled"

    def at_save(ren):
        st = ren.stats()
        if save_at == 8:
            assert st["cacheReadyMask"] != ref["stats"]["cacheReadyMask"] and st["gradCalls"] > 0, st
        else:
            assert st["cacheReadyMask"] == ref["stats"]["cacheReadyMask"], st

    _assert_same(ref, _interrupted(MALA4, 72, save_at, str(tmp_path / "c.ckpt"), check_at_save=at_save))


def test_h2mc_resumes_exactly(tmp_path):
    """3. H2MC, 4096 chains x 30 steps, saved at 9: the dense Gaussians of the pipeline's per-slot buffers travel"""
    _assert_same(_uninterrupted("h2", 30), _interrupted(H2, 30, 9, str(tmp_path / "c.ckpt")))


@pytest.mark.parametrize("extra", [{"samplecache": 1, "largestepmultiplexed": 1}, {"uselightcoordinatesampling": 1}], ids=["samplecache_mux", "lightcoord"])
def test_samplecache_and_light_coordinate_sampling_resume_exactly(tmp_path, extra):
    """4. the size of case 2 with `samplecache` + `largestepmultiplexed` (chain.path, cache rows with paths, the length distribution) and with
    `uselightcoordinatesampling`; saved inside the fill phase"""
    cfg = dict(MALA4, opts=dict(FILL, **extra))
    ren = _fresh(cfg)
    ren.step(72)
    ref = _result([ren])
    ren.close()
    _assert_same(ref, _interrupted(cfg, 72, 20, str(tmp_path / "c.ckpt")))


RELOC, NORELOC = {"LMC_RELOCATE": "1", "LMC_RESORT_EVERY": "4"}, {"LMC_RELOCATE": "0", "LMC_RESORT_EVERY": "0"}


@pytest.mark.parametrize("save_env,load_env", [(RELOC, NORELOC), (NORELOC, RELOC)], ids=["relocated_to_plain", "plain_to_relocated"])
def test_layout_independence(tmp_path, save_env, load_env):
    """5a. saved with the chains relocated and re-sorted every 4th step, loaded without relocation, and the reverse"""
    _assert_same(_uninterrupted("mala4", 72), _interrupted(MALA4, 72, 40, str(tmp_path / "c.ckpt"), save_env=save_env, load_env=load_env))


@pytest.mark.parametrize("save_resident,load_resident", [(8, 0), (0, 8)], ids=["resident_to_lock_step", "lock_step_to_resident"])
def test_schedule_independence(tmp_path, save_resident, load_resident):
    """5b. saved after a resident_steps=8 call, loaded into lock step, and the reverse"""
    _assert_same(_uninterrupted("plain", 40), _interrupted(PLAIN, 40, 13, str(tmp_path / "c.ckpt"), save_resident=save_resident, load_resident=load_resident))


def test_group_files_load_into_any_number_of_members(tmp_path):
    """6. 12288 chains (divisible by 6), MALA through the fill phase: saved from a Group of 2 on one device, loaded into a single Renderer and into a
    Group of 3; both end where the uninterrupted single context ends (the group's film after film_reduce)"""
    p = gc.pkg()
    cfg = dict(MALA4, n=12288)
    steps, save_at, path = 48, 10, str(tmp_path / "g.ckpt")
    ren = _fresh(cfg)
    ren.step(steps)
    ref = _result([ren])
    ren.close()
    rens = [_renderer(**cfg) for _ in range(2)]
    g = p.Group(rens)
    g.init_chains(200000, cfg["n"], 64, 10 ** 6)
    g.step(save_at)
    g.save_checkpoint(path)
    for r in rens:
        r.close()
    assert p.checkpoint_info(path)["n_chains_total"] == cfg["n"]
    one = _loaded(cfg, path)
    one.step(steps - save_at)
    _assert_same(ref, _result([one]))
    one.close()
    rens = [_renderer(**cfg) for _ in range(3)]
    g = p.Group(rens)
    norm = g.load_checkpoint(path)
    assert [r.num_chains for r in rens] == [4096] * 3
    for r in rens:
        r.norm = norm
    g.step(steps - save_at)
    _assert_same(ref, _result(rens, group=g))
    for r in rens:
        r.close()


def test_resume_against_the_oracle(tmp_path):
    """7. the configuration of tests/test_gpu_resident.py::test_resident_against_the_oracle_lock_step (plain-MLT torus, the oracle needs no gradient
    library): saved and loaded in the middle, the final device states against the oracle's uninterrupted ones, compared as that test compares them"""
    cfg = gc.oracle_run_config(160, 120, 40000, 256, 8, 400, 40, mala=False)
    o = gc.oracle_run(cfg, "")

    def make():
        ren = gc.pkg().Renderer(gc.TORUS, force_diffuse=1, max_depth=6, width=160, height=120, seed_offset=0, use_gradient=0)
        ren.set_option("mala", 0)
        return ren

    ren = make()
    norm, contribs = ren.init_chains(40000, 256, 8, 400)
    ren.step(17)
    ren.save_checkpoint(str(tmp_path / "o.ckpt"))
    ren.close()
    ren = make()
    assert ren.load_checkpoint(str(tmp_path / "o.ckpt")) == norm
    ren.step(23)
    sg, cg, gi, fg = ren.stats(), ren.summary(0), ren.summary(1), ren.film()
    ren.close()
    assert contribs == o["contribs"] and norm == o["norm"]
    si, co = o["init_summary"], o["summary"]
    assert np.array_equal(si[:, 1:4], gi[:, 1:4]) and np.array_equal(si[:, 16:], gi[:, 16:])
    so = o["stats"]
    assert sg["steps"] == so["steps"] == 256 * 40
    for k in ("largeSteps", "accepted", "resets"):
        assert sg[k] == so[k], k
    same = (co[:, 0] == cg[:, 0]) & (co[:, 1] == cg[:, 1]) & (co[:, 2] == cg[:, 2]) & (np.abs(co[:, 3] - cg[:, 3]) <= 1e-3 * np.abs(co[:, 3]) + 1e-12)
    assert same.all()
    lo, lg = gc.lum(o["film"]), gc.lum(fg)
    assert np.linalg.norm(lo - lg) < 1e-4 * np.linalg.norm(lo)
    assert abs(lg.sum() / (norm * sg["weightSum"]) - 1.0) < 1e-4


def test_save_is_transparent(tmp_path):
    """8. a run that saves twice along the way ends where one that never saves ends; a file under the path is always complete (no .tmp left)"""
    ren = _fresh(PLAIN)
    ren.step(5)
    ren.save_checkpoint(str(tmp_path / "a.ckpt"))
    ren.step(15)
    ren.save_checkpoint(str(tmp_path / "a.ckpt"))
    ren.step(20)
    out = _result([ren])
    ren.close()
    _assert_same(_uninterrupted("plain", 40), out)
    assert sorted(os.listdir(tmp_path)) == ["a.ckpt"]
    assert gc.pkg().checkpoint_info(str(tmp_path / "a.ckpt"))["steps_done"] == 20


def test_refusals_leave_the_context_usable(tmp_path):
    """9. a load into a context that differs in width / maxdepth / seedoffset / mala, or whose scene file changed, returns -1 and names the field; a file
    cut to half its length and a wrong magic are refused; so is a save before init.  In each case the context still steps correctly afterwards."""
    p = gc.pkg()
    small = dict(PLAIN, n=1024)
    path = str(tmp_path / "r.ckpt")
    ren = _fresh(small)
    ren.step(3)
    ren.save_checkpoint(path)
    ren.step(5)
    ref = _result([ren])
    ren.close()

    def still_works(ren):  # ... by loading the good file: it must end where the saving run ended
        ren.norm = ren.load_checkpoint(path)
        ren.step(5)
        _assert_same(ref, _result([ren]))
        ren.close()

    def refused(ren, file, word):
        with pytest.raises(RuntimeError, match=word):
            ren.load_checkpoint(file)

    refused(_renderer(**dict(small, width=160)), path, "width")
    refused(_renderer(**dict(small, max_depth=5)), path, "maxdepth")
    ren = p.Renderer(gc.TORUS, force_diffuse=1, max_depth=6, width=128, height=96, seed_offset=1, use_gradient=1)
    ren.set_option("largestepprob", 0.3), ren.set_option("largestepscale", 1.0), ren.set_option("mala", 0)
    refused(ren, path, "seedoffset")
    ren.close()
    ren = _renderer(**dict(small, mala=True))
    refused(ren, path, "mala")
    ren.set_option("mala", 0)
    still_works(ren)
    # a scene file whose bytes changed (a comment appended): same parse, another content hash
    os.symlink(os.path.join(gc.ROOT, "scenes", "torus", "data"), tmp_path / "data")
    (tmp_path / "lmc.xml").write_text(open(gc.TORUS).read() + "<!-- edited -->\n")
    ren = p.Renderer(str(tmp_path / "lmc.xml"), force_diffuse=1, max_depth=6, width=128, height=96, seed_offset=0, use_gradient=1)
    ren.set_option("largestepprob", 0.3), ren.set_option("largestepscale", 1.0), ren.set_option("mala", 0)
    refused(ren, path, "scene")
    ren.close()
    blob = open(path, "rb").read()
    (tmp_path / "half.ckpt").write_bytes(blob[: len(blob) // 2])
    (tmp_path / "magic.ckpt").write_bytes(b"NOTACKPT" + blob[8:])
    ren = _renderer(**small)
    refused(ren, str(tmp_path / "half.ckpt"), "truncated")
    refused(ren, str(tmp_path / "magic.ckpt"), "magic")
    with pytest.raises(RuntimeError, match="before lmc_chains_init"):
        ren.save_checkpoint(str(tmp_path / "never.ckpt"))
    assert not os.path.exists(tmp_path / "never.ckpt")
    with pytest.raises(RuntimeError, match="truncated"):
        p.checkpoint_info(str(tmp_path / "half.ckpt"))
    still_works(ren)
    # a failed load leaves the chains a context already had
    ren = _fresh(small)
    ren.step(3)
    refused(ren, str(tmp_path / "half.ckpt"), "truncated")
    ren.step(5)
    _assert_same(ref, _result([ren]))
    ren.close()


def _small_scene(d, width=96, height=72, spp=64):
    """the shipped scene file with a smaller film and budget (as tests/test_gpu_cli.py reduces it)"""
    xml = open(gc.TORUS).read()
    xml = xml.replace('<integer name="height" value="768"/>', '<integer name="height" value="%d"/>' % height)
    xml = xml.replace('<integer name="width" value="1024"/>', '<integer name="width" value="%d"/>' % width)
    xml = re.sub(r'<integer name="spp"\s+value="245"/>', '<integer name="spp" value="%d"/>' % spp, xml)
    assert 'value="%d"' % spp in xml and 'value="%d"' % width in xml
    os.makedirs(d)
    os.symlink(os.path.join(gc.ROOT, "scenes", "torus", "data"), d / "data")
    (d / "lmc.xml").write_text(xml)
    return str(d / "lmc.xml")


def test_dpt_amd_max_steps_then_resume(tmp_path):
    """10. dpt_amd straight through, and as --max-steps with --checkpoint followed by --resume: after decoding, the two EXRs agree to one half-float
    step per pixel (2^-10 relative: the film's 1e-5 atomics-order difference can flip a half rounding and nothing more), and the final output name
    carries the seconds of both legs"""
    assert os.path.exists(CLI), "dpt_amd not built"

    def run(d, *flags):
        scene = os.path.join(d, "lmc.xml")
        before = set(os.listdir(d))
        r = subprocess.run([CLI, "--chains", "4096"] + list(flags) + [scene], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
        assert r.returncode == 0 and r.stdout.rstrip().endswith("Done!"), r.stdout
        new = [f for f in set(os.listdir(d)) - before if f.endswith(".exr")]
        assert len(new) == 1, (new, r.stdout)
        return r.stdout, new[0]

    _small_scene(tmp_path / "a")
    _small_scene(tmp_path / "b")
    _, straight = run(str(tmp_path / "a"))
    ck = str(tmp_path / "b" / "render.ckpt")
    out1, first = run(str(tmp_path / "b"), "--checkpoint", ck, "--max-steps", "40")
    assert "Checkpoint after 40 of" in out1 and os.path.exists(ck)
    info = gc.pkg().checkpoint_info(ck)
    assert info["steps_done"] == 40 and info["n_chains_total"] == 4096
    out2, second = run(str(tmp_path / "b"), "--resume", ck)
    assert "Resumed" in out2 and "Average brightness:" in out2
    secs = lambda name: float(re.fullmatch(r"lmc_timeuse_([0-9]+\.[0-9]{6})s\.exr", name).group(1))
    leg2 = float(re.search(r"Elapsed time:([0-9.eE+-]+)", out2).group(1))
    assert secs(second) == pytest.approx(leg2, abs=1e-3)  # ("Elapsed time:" prints six significant digits)
    assert secs(second) > info["wall_seconds"] > 0  # the suffix is the sum: the first leg's seconds + this leg's
    a = gc.pkg().read_image(str(tmp_path / "a" / straight))
    b = gc.pkg().read_image(str(tmp_path / "b" / second))
    assert a.shape == b.shape == (72, 96, 3)
    assert (np.abs(a - b) <= 2.0 ** -10 * np.maximum(np.abs(a), np.abs(b))).all(), float(np.max(np.abs(a - b) / np.maximum(np.abs(a), 1e-30)))
    part = gc.pkg().read_image(str(tmp_path / "b" / first))
    assert 0 < part.mean() < a.mean()  # the image of what had been rendered after 40 steps
