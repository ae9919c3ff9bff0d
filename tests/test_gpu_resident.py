"""The resident schedule (lmc_set_option "resident_steps" = K, device/step_resident.h): once the gradient caches are frozen, one launch advances
every chain by up to K complete mutations.  The contract checked here is that it is a SCHEDULE only: each case runs two contexts with identical
seeds, A in lock step and B resident, and B must follow A chain for chain -- every current and init state bit-equal, the eight counters equal, the
splat-weight sum to 1e-9, the film up to the order of its float atomics, the same energy identity.  Every case also checks that B really ran
resident launches (a silent fall-back to lock step would pass the comparison) and that no resident step would have needed the gradient program
or a cache push (the guard counter the kernel keeps)."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import gpu_checks as gc

pytestmark = pytest.mark.gpu

DOOR = os.path.join(gc.ROOT, "scenes", "veachdoor", "lmc.xml")
AREA = os.path.join(gc.ROOT, "scenes", "torus", "lmc_arealight.xml")
H2MC = os.path.join(gc.ROOT, "scenes", "torus", "h2mc.xml")
CLI = os.path.join(gc.ROOT, "langevin-mcmc_amd", "dpt_amd")
FILL = {"largestepprob": 0.5, "largestepscale": 1.0}  # maxdepth 4: two cache dims (6, 8), both full after ~25 steps of 16384 chains


def _ctx(scene=gc.TORUS, n=4096, resident=0, opts=None, mala=True, max_depth=6, force_diffuse=1, per_chain=10 ** 6, extra=0, num_init=200000,
         init_threads=64, env=None):
    """a context with its chains initialised; `env`: variables read at lmc_create (test hooks)"""
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        ren = gc.pkg().Renderer(scene, force_diffuse=force_diffuse, max_depth=max_depth, width=128, height=96, seed_offset=0, use_gradient=1)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    for k, v in (opts or {}).items():
        ren.set_option(k, v)
    if not mala:
        ren.set_option("mala", 0)
    if resident:
        ren.set_option("resident_steps", resident)
    ren.norm, _ = ren.init_chains(num_init, n, init_threads, per_chain, extra)
    return ren


def _result(ren):
    return dict(cur=ren.summary(0).copy(), init=ren.summary(1).copy(), stats=ren.stats(), film=ren.film().copy(), norm=ren.norm)


def _energy(r):
    return float(gc.lum(r["film"]).sum() / (r["norm"] * r["stats"]["weightSum"]))


def _assert_exact(a, b):
    """B (resident) against A (lock step): the module docstring's "exact" """
    assert a["cur"].shape == b["cur"].shape
    assert np.array_equal(a["cur"].view(np.uint32), b["cur"].view(np.uint32)), "current states differ: %d rows" % int(
        (a["cur"].view(np.uint32) != b["cur"].view(np.uint32)).any(axis=1).sum())
    assert np.array_equal(a["init"].view(np.uint32), b["init"].view(np.uint32))
    for k in gc.STAT_KEYS:
        assert a["stats"][k] == b["stats"][k], (k, a["stats"][k], b["stats"][k])
    assert b["stats"]["weightSum"] == pytest.approx(a["stats"]["weightSum"], rel=1e-9)
    la, lb = gc.lum(a["film"]), gc.lum(b["film"])
    assert np.isfinite(lb).all()
    assert np.linalg.norm(la - lb) < 1e-5 * np.linalg.norm(la)
    ea, eb = _energy(a), _energy(b)
    assert 0.99 < ea <= 1.0001 and abs(eb - ea) < 1e-6, (ea, eb)


def _assert_resident_ran(ren):
    rs = ren.resident_stats()
    assert rs["launches"] > 0 and rs["chain_steps"] > 0, rs
    assert rs["guard"] == 0, rs
    return rs


def _pair(steps, resident, after_fill=False, **kw):
    """A (lock step) and B (resident_steps = resident) through `steps` mutations, B in one call.  after_fill: A steps in batches of 8 until every
    relevant cache dim (6 .. 2 maxdepth, at most 12) is ready, then `steps` more; B runs the same total in one call"""
    a = _ctx(**kw)
    total = 0
    if after_fill:
        md = kw.get("max_depth", 6)
        relevant = sum(1 << d for d in range(6, min(2 * md, 12) + 1, 2))
        while (a.stats()["cacheReadyMask"] & relevant) != relevant:
            assert total < 600, "test set-up: the caches did not fill"
            a.step(8)
            total += 8
    a.step(steps)
    total += steps
    ra = _result(a)
    a.close()
    b = _ctx(resident=resident, **kw)
    b.step(total)
    rb = _result(b)
    rs = _assert_resident_ran(b)
    b.close()
    return ra, rb, rs


@pytest.mark.parametrize("K", [1, 7, 48])
def test_plain_mlt_resident_is_lock_step(K):
    """plain MLT (mala = 0): no cache, so resident from the first step; 4096 chains x 48 steps"""
    a, b, rs = _pair(48, K, mala=False)
    _assert_exact(a, b)
    assert rs["lock_steps"] == 0 and rs["k"] == min(K, 32) and rs["launches"] == -(-48 // rs["k"])
    assert rs["chain_steps"] == b["stats"]["steps"] == 4096 * 48


def test_lmc_crosses_the_fill_to_frozen_hand_over_in_one_call():
    """LMC, torus (diffuse), fresh chains: ONE step(n) call on B runs the cache-fill phase in lock step and the rest resident"""
    n, kw = 72, dict(n=16384, opts=FILL, max_depth=4)
    a = _ctx(**kw)
    a.step(n // 2)
    mask = a.stats()["cacheReadyMask"]
    assert mask == (1 << 6) | (1 << 8), "test set-up: the caches of dims 6 and 8 are not both ready after %d steps (mask %#x)" % (n // 2, mask)
    a.step(n - n // 2)
    ra = _result(a)
    a.close()
    b = _ctx(resident=16, **kw)
    b.step(n)
    rb = _result(b)
    rs = _assert_resident_ran(b)
    b.close()
    assert 0 < rs["lock_steps"] < n // 2 and rs["launches"] == -(-(n - rs["lock_steps"]) // 16)
    assert ra["stats"]["gradCalls"] > 0
    _assert_exact(ra, rb)


@pytest.mark.parametrize("scene,force_diffuse,max_depth", [(DOOR, 0, 8), (gc.TORUS, 0, 8)], ids=["veach_door", "torus_full_material"])
def test_glossy_instantiations(scene, force_diffuse, max_depth):
    """the glossy kernels: the veach-door scene and the full-material torus, LMC with its caches filled first"""
    a, b, rs = _pair(40, 32, after_fill=True, scene=scene, force_diffuse=force_diffuse, max_depth=max_depth, n=16384, opts=FILL)
    assert a["stats"]["gradCalls"] > 0
    _assert_exact(a, b)


@pytest.mark.parametrize("opts,scene", [({"largestepmultiplexed": 1}, gc.TORUS), ({"largestepmultiplexed": 1, "samplecache": 1}, gc.TORUS),
                                        ({"uselightcoordinatesampling": 1}, AREA)], ids=["multiplexed", "samplecache", "lightcoord"])
def test_other_large_steps_and_the_generic_small_step(opts, scene):
    a, b, rs = _pair(40, 16, after_fill=True, scene=scene, n=16384, opts=dict(FILL, **opts), max_depth=4)
    _assert_exact(a, b)


def test_per_chain_sample_budgets():
    """30 samples per chain, the first 1000 chains one more; 64 steps asked for: every chain stops at its own count"""
    a, b, rs = _pair(64, 16, mala=False, per_chain=30, extra=1000)
    _assert_exact(a, b)
    assert np.array_equal(a["cur"][:, 9], b["cur"][:, 9])
    idx = b["cur"][:, 9]
    assert (idx[:1000] == 31).all() and (idx[1000:] == 30).all(), np.unique(idx)
    assert b["stats"]["steps"] == 4096 * 30 + 1000


def test_outlier_reset_path():
    """LMC_EXP_OUTLIER_TEST (bit 128 of expFlags, read at lmc_create): resets after 2 / 6 adjacent rejections, thousands of them"""
    a, b, rs = _pair(48, 12, mala=False, env={"LMC_EXP_OUTLIER_TEST": "1"})
    assert b["stats"]["resets"] > 0
    _assert_exact(a, b)


def test_lock_step_resumes_after_a_resident_run():
    """resident for 24 steps, then resident_steps = 0 and 20 lock steps with chain relocation on (the full re-sort the resident run left due runs first)"""
    kw = dict(mala=False)
    a = _ctx(**kw)
    a.step(44)
    ra, rela = _result(a), a.relocation_stats()
    a.close()
    b = _ctx(resident=8, **kw)
    b.step(24)
    b.set_option("resident_steps", 0)
    b.step(20)
    rb, relb = _result(b), b.relocation_stats()
    rs = _assert_resident_ran(b)
    b.close()
    assert rs["launches"] == 3 and rs["lock_steps"] == 20 and rs["chain_steps"] == 4096 * 24
    _assert_exact(ra, rb)
    assert rela is not None and relb is not None
    assert relb["slots"] == 4096 and relb["relocations"] == 20 and 0 <= relb["moved"] <= 4096 and relb["breaks"] < 4096


def test_in_process_group_with_resident_steps():
    """two members of an in-process group on one device, resident after the fill phase: equal to one context holding all the chains"""
    p = gc.pkg()
    n, steps = 16384, 60
    kw = dict(force_diffuse=1, max_depth=4, width=128, height=96, seed_offset=0, use_gradient=1)
    one = p.Renderer(gc.TORUS, **kw)
    for k, v in FILL.items():
        one.set_option(k, v)
    norm1, _ = one.init_chains(200000, n, 64, 10 ** 6)
    one.step(steps)
    st1, fin1, film1 = one.stats(), one.summary(0), one.film()
    one.close()
    rens = [p.Renderer(gc.TORUS, **kw) for _ in range(2)]
    for r in rens:
        for k, v in FILL.items():
            r.set_option(k, v)
        r.set_option("resident_steps", 16)
    grp = p.Group(rens)
    normg, _ = grp.init_chains(200000, n, 64, 10 ** 6)
    grp.step(steps)
    rs = grp.resident_stats()
    sts = [r.stats() for r in rens]
    fing = np.concatenate([r.summary(0) for r in rens])
    filmg = sum(r.film() for r in rens)
    for r in rens:
        r.close()
    assert normg == norm1
    assert rs["launches"] > 0 and rs["chain_steps"] > 0 and rs["guard"] == 0, rs
    assert all(m["lock_steps"] == rs["lock_steps"] for m in rs["members"])
    for k in ("steps", "largeSteps", "accepted", "gradCalls", "cacheQueries", "cacheHits", "resets"):
        assert sum(s_[k] for s_ in sts) == st1[k], k
    assert all(s_["cacheReadyMask"] == st1["cacheReadyMask"] for s_ in sts)
    assert np.array_equal(fing.view(np.uint32), fin1.view(np.uint32))
    l1, lg = gc.lum(film1), gc.lum(filmg)
    assert np.linalg.norm(l1 - lg) < 1e-5 * np.linalg.norm(l1)


def test_resident_against_the_oracle_lock_step():
    """plain-MLT torus, resident on the device against the CPU oracle's lock-step orc_step: the set-up of test_chain_loop_parity[0] (no gradient
    library needed), chain-exact"""
    cfg = gc.oracle_run_config(160, 120, 40000, 256, 8, 400, 40, mala=False)
    o = gc.oracle_run(cfg, "")
    ren = gc.pkg().Renderer(gc.TORUS, force_diffuse=1, max_depth=6, width=160, height=120, seed_offset=0, use_gradient=0)
    ren.set_option("mala", 0)
    ren.set_option("resident_steps", 16)
    norm, contribs = ren.init_chains(40000, 256, 8, 400)
    ren.step(40)
    sg, cg, gi, fg = ren.stats(), ren.summary(0), ren.summary(1), ren.film()
    rs = _assert_resident_ran(ren)
    ren.close()
    assert rs["lock_steps"] == 0 and rs["launches"] == 3
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


def _small_scene(d, width=96, height=72, spp=320):
    """the shipped torus scene file with a smaller film and budget (as tests/test_gpu_cli.py reduces it)"""
    xml = open(gc.TORUS).read()
    xml = xml.replace('<integer name="height" value="768"/>', '<integer name="height" value="%d"/>' % height)
    xml = xml.replace('<integer name="width" value="1024"/>', '<integer name="width" value="%d"/>' % width)
    xml = re.sub(r'<integer name="spp"\s+value="245"/>', '<integer name="spp" value="%d"/>' % spp, xml)
    # large steps as in FILL, so that the caches of 4096 chains fill early in the render and most of its steps run resident
    xml = re.sub(r'<float\s+name="largestepprob"\s+value="[0-9.]+"/>', '<float name="largestepprob" value="0.5"/>', xml)
    xml = re.sub(r'<float\s+name="largestepscale"\s+value="[0-9.]+"/>', '<float name="largestepscale" value="1"/>', xml)
    assert 'value="%d"' % spp in xml and 'value="%d"' % width in xml and 'name="largestepprob" value="0.5"' in xml
    os.symlink(os.path.join(gc.ROOT, "scenes", "torus", "data"), d / "data")
    p = d / "lmc.xml"
    p.write_text(xml)
    return str(p)


def test_dpt_amd_resident_flag(tmp_path):
    """`dpt_amd --chains 4096 --resident 32` against the same command without --resident: same trajectories, so the same image (up to the
    film's atomics and the half-precision pixels), the same stdout lines and output naming"""
    if not os.path.exists(CLI):
        pytest.skip("dpt_amd not built")
    outs, imgs = [], []
    for k, extra in enumerate(([], ["--resident", "32"])):
        d = tmp_path / ("run%d" % k)
        d.mkdir()
        scene = _small_scene(d)
        r = subprocess.run([CLI, "--seedoffset", "5", "--chains", "4096", "--maxdepth", "4", "--force-diffuse"] + extra + [scene], stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True, timeout=600)
        assert r.returncode == 0, r.stdout
        outs.append(r.stdout)
        exrs = [f for f in os.listdir(d) if f.endswith(".exr")]
        assert len(exrs) == 1 and re.fullmatch(r"lmc_timeuse_[0-9]+\.[0-9]{6}s\.exr", exrs[0]), os.listdir(d)
        imgs.append(gc.pkg().read_image(str(d / exrs[0])))
    mask = lambda s: [re.sub(r"[0-9.eE+-]+", "#", l) for l in s.splitlines()]
    assert mask(outs[0]) == mask(outs[1]), (outs[0], outs[1])
    m = [int(re.search(r"(\d+) mutations", o).group(1)) for o in outs]
    assert m[0] == m[1] > 0
    a, b = gc.lum(imgs[0].reshape(-1, 3)), gc.lum(imgs[1].reshape(-1, 3))
    assert np.linalg.norm(a - b) < 1e-4 * np.linalg.norm(a)
    # the same configuration through the library reaches the resident launches (the command line prints no statistics)
    ren = _ctx(scene=_small_scene(tmp_path), n=4096, max_depth=4, resident=32)
    steps = 96 * 72 * 320 // 4096
    ren.step(steps)
    rs = _assert_resident_ran(ren)
    assert rs["lock_steps"] < steps // 2, rs
    ren.close()


def test_h2mc_refuses_resident_steps():
    ren = gc.pkg().Renderer(H2MC, force_diffuse=1, max_depth=6, width=64, height=48, seed_offset=0, use_gradient=1)
    assert ren.get_option("h2mc") == 1
    with pytest.raises(RuntimeError, match="H2MC"):
        ren.set_option("resident_steps", 8)
    ren.set_option("resident_steps", 0)  # lock step stays allowed
    ren.close()


def test_option_names_and_values():
    ren = gc.pkg().Renderer(gc.TORUS, force_diffuse=1, max_depth=6, width=64, height=48, seed_offset=0, use_gradient=1)
    with pytest.raises(RuntimeError, match="Unknown dpt option"):
        ren.set_option("resident_stepz", 8)
    with pytest.raises(RuntimeError, match="resident_lanes"):
        ren.set_option("resident_lanes", 48)
    ren.set_option("resident_steps", 8)
    assert ren.get_option("resident_steps") == 8 and ren.get_option("resident_lanes") == 0  # 0: chosen by the number of chains
    ren.set_option("resident_lanes", 16)
    assert ren.get_option("resident_lanes") == 16
    ren.close()
