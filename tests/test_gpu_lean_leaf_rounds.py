"""`-m gpu` tier: the Lambertian lightless lean launches fetch a leaf's triangles two per round (dscene.h Stk::kTight / kLeafRound) where every
other launch fetches four.  Tests within a leaf stay in leaf order and the tie rule (equal t: the lower global id wins) is untouched, so nothing a
walk returns may move.

End to end: the chain-exact comparison with the CPU oracle that tests/test_gpu_step_args.py makes (contributions, normalization, init states,
counters and every chain's final state equal; the film up to the order of its float atomic adds, the bar of that file), 4 096 chains x 24
lock-step mutations on the Lambertian torus (the tight instantiation on quantised nodes) and on the veach-door (glossy, with light sub-paths: four
per round, 40 stack words), each once with the default launch and once with LMC_LEAN_LDS=0 (private-stack fallback).  One oracle run per scene is
shared by its two GPU runs.

Exact, GPU against GPU: with the fixed-point film (set_option("film_exact", 1)) a run's film does not depend on the order of its splats, so the
launches can be compared word for word.  On the torus the default launch (tight: two triangles per round, LDS stack, quantised nodes), the same on
the exact nodes (LMC_BVH_NODES=exact) and the private-stack fallback (LMC_LEAN_LDS=0: NOT tight, four per round) must give the same int64 film, the
same counters and bit-equal chain summaries (every score word); on the door the default launch and the fallback.  A wrong tie or a dropped hit in
one of the walks moves a state, and with it words of all three.  Which instantiation a run took is read from lmc_lean_info, not assumed.

The walk alone: lmc_trace / lmc_occluded with LMC_TRACE_TIGHT=1 walk as the tight launches do.  The mesh is 24 clusters of 1 .. 8 triangles, far
apart, each cluster's triangles on top of each other, so that the SAH builder keeps a cluster in one leaf (LMC_BVH_LEAF=8: leaves of 1, 2, 3, 4 and
5 .. 8 triangles) or splits only the large ones (default, leaves of at most 4):
  family A: k coincident copies of one triangle -- equal t on both sides of every round boundary, whatever the leaf order: the lowest id must win;
  family B: k parallel triangles 1/64 apart, ids in shuffled depth order -- the nearest sits at varying places of the leaf;
  family C: the same with every depth taken by two coincident copies.
Every ray is compared with a brute-force closest hit in numpy that repeats TriTest (dscene.h) operation by operation in float32.

Run times on an MI355X: see the case list printed by --durations; every case a few seconds at the most (the oracle runs dominate)."""
import os

import numpy as np
import pytest

from tests import gpu_checks as gc

pytestmark = pytest.mark.gpu
DOOR = os.path.join(gc.ROOT, "scenes", "veachdoor", "lmc.xml")
COUNTERS = ("largeSteps", "accepted", "gradCalls", "cacheQueries", "cacheHits", "resets", "cacheReadyMask")
N_CHAINS, STEPS = 4096, 24
OPTS = {"largestepprob": 0.3, "largestepscale": 1.0}
# (the door needs 80 000 initial samples to seed 4 096 chains: with the 20 000 of tests/test_gpu_step_args.py MLTInit refuses)
SCENES = {
    "torus": dict(width=96, height=72, num_init=20000, init_threads=64, per_chain=400, scene=gc.TORUS, force_diffuse=1),
    "door": dict(width=96, height=54, num_init=80000, init_threads=20000, per_chain=400, scene=DOOR, force_diffuse=0),
}
_oracle_runs = {}


def _oracle(name):
    """the oracle's run of a scene: computed once, read by both GPU runs"""
    if name not in _oracle_runs:
        s = SCENES[name]
        cfg = gc.oracle_run_config(s["width"], s["height"], s["num_init"], N_CHAINS, s["init_threads"], s["per_chain"], STEPS, 6, s["scene"], True, OPTS, s["force_diffuse"])
        _oracle_runs[name] = gc.oracle_run(cfg, "")
    return _oracle_runs[name]


def _check_form(info, name, env):
    """the instantiation of the lean launch a context takes (lmc_lean_info asks the function the launch itself asks, step_small_plain.hip LeanFormOf)"""
    lds = env.get("LMC_LEAN_LDS", "1") != "0"
    want = dict(lds=int(lds), glossy=int(name == "door"), lightless=int(name == "torus" and lds), tight=int(name == "torus" and lds),
                quant=int(name == "torus" and lds and env.get("LMC_BVH_NODES") != "exact"), block=64)
    want.update(dict(stack_need=27, stack_words=28) if name == "torus" else dict(stack_need=37, stack_words=40))
    got = {k: info[k] for k in want}
    assert got == want, (name, env, got, want)


@pytest.mark.parametrize("lean_lds", ["default", "0"])
@pytest.mark.parametrize("name", ["torus", "door"])
def test_chain_exact_against_the_oracle(name, lean_lds, monkeypatch):
    if lean_lds != "default":
        monkeypatch.setenv("LMC_LEAN_LDS", lean_lds)
    s, o = SCENES[name], _oracle(name)
    ren = gc.pkg().Renderer(s["scene"], force_diffuse=s["force_diffuse"], max_depth=6, width=s["width"], height=s["height"], seed_offset=0, use_gradient=0)
    for k, v in OPTS.items():
        ren.set_option(k, v)
    _check_form(ren.lean_info(), name, {} if lean_lds == "default" else {"LMC_LEAN_LDS": lean_lds})
    gn, gcn = ren.init_chains(s["num_init"], N_CHAINS, s["init_threads"], s["per_chain"])
    si, gi = o["init_summary"], ren.summary(1)
    ren.step(STEPS)
    so, sg = o["stats"], ren.stats()
    co, cg = o["summary"], ren.summary(0)
    lo, lg = gc.lum(o["film"]), gc.lum(ren.film())
    nonfinite = int((~np.isfinite(ren.film())).sum())
    ren.close()
    film_rel_l2 = float(np.linalg.norm(lo - lg) / max(np.linalg.norm(lo), 1e-30))
    same = (co[:, 0] == cg[:, 0]) & (co[:, 1] == cg[:, 1]) & (co[:, 2] == cg[:, 2])
    close = same & (np.abs(co[:, 3] - cg[:, 3]) <= 1e-3 * np.abs(co[:, 3]) + 1e-12)
    print(name, lean_lds, dict(film_rel_l2=film_rel_l2, final_state_match=float(close.mean()), bvh_stack_need=ren.bvh_depth), sg)
    # initial states
    assert gcn == o["contribs"] and gn == o["norm"]
    ok = (si[:, 3] > 0)
    assert np.array_equal(si[:, 1:3], gi[:, 1:3])
    assert np.array_equal(si[ok, 3], gi[ok, 3]) and np.array_equal(si[ok, 16:], gi[ok, 16:])
    # counters
    assert sg["steps"] == so["steps"] == N_CHAINS * STEPS
    for k in COUNTERS:
        assert sg[k] == so[k], (k, sg[k], so[k])
    assert so["steps"] - so["largeSteps"] > 4 * N_CHAINS, "test set-up: too few small steps"  # (the door's fresh chains take large steps until their first acceptance)
    # every chain's final state (tests/gpu_checks.py run_pair: same slot, same technique, the score to 1e-3)
    assert float(close.mean()) == 1.0
    # film: the same splats in another order of float atomic adds
    assert film_rel_l2 < 1e-4
    assert nonfinite == 0


VARIANTS = {"torus": [{}, {"LMC_BVH_NODES": "exact"}, {"LMC_LEAN_LDS": "0"}], "door": [{}, {"LMC_LEAN_LDS": "0"}]}


def _exact_run(name, env, monkeypatch):
    with monkeypatch.context() as m:
        for k, v in env.items():
            m.setenv(k, v)  # both switches are read when the context is created (host/context.cpp)
        s = SCENES[name]
        ren = gc.pkg().Renderer(s["scene"], force_diffuse=s["force_diffuse"], max_depth=6, width=s["width"], height=s["height"], seed_offset=0, use_gradient=0)
        for k, v in OPTS.items():
            ren.set_option(k, v)
        ren.set_option("film_exact", 1)
        _check_form(ren.lean_info(), name, env)
        norm_contribs = ren.init_chains(s["num_init"], N_CHAINS, s["init_threads"], s["per_chain"])
        ren.step(STEPS)
        out = dict(norm_contribs=norm_contribs, stats=ren.stats(), film=ren.film_fixed(), overflow=ren.film_overflow(), summary=np.ascontiguousarray(ren.summary(0)))
        ren.close()
    return out


@pytest.mark.parametrize("name", ["torus", "door"])
def test_launch_forms_agree_word_for_word_on_the_exact_film(name, monkeypatch):
    runs = [_exact_run(name, env, monkeypatch) for env in VARIANTS[name]]
    ref = runs[0]
    assert ref["overflow"] == 0 and ref["stats"]["steps"] == N_CHAINS * STEPS
    assert np.count_nonzero(ref["film"]) > 1000 and ref["stats"]["steps"] - ref["stats"]["largeSteps"] > 4 * N_CHAINS, "test set-up: an empty run compares nothing"
    counters = lambda r: {k: r["stats"][k] for k in ("steps",) + COUNTERS}  # (not weightSum: a double sum of block sums in launch order)
    assert counters(ref) == {k: _oracle(name)["stats"][k] for k in ("steps",) + COUNTERS}
    for env, r in zip(VARIANTS[name][1:], runs[1:]):
        print(name, env, dict(film_words_differ=int((r["film"] != ref["film"]).sum()), summary_bytes_equal=r["summary"].tobytes() == ref["summary"].tobytes()))
        assert r["norm_contribs"] == ref["norm_contribs"], env
        assert counters(r) == counters(ref), (env, r["stats"], ref["stats"])
        assert r["overflow"] == 0
        assert np.array_equal(r["film"], ref["film"]), env  # int64 words
        assert r["summary"].dtype == ref["summary"].dtype and r["summary"].tobytes() == ref["summary"].tobytes(), env  # every word of every chain's summary, bit for bit


# ------------------------------------------------------------------------------------------------------------------------ the walk alone
def _cluster_mesh():
    """(vertices [n, 3, 3] float32 in face order = global triangle id, cluster of every triangle)"""
    rng = np.random.default_rng(11)
    tris, cluster = [], []
    for fam in range(3):
        for k in range(1, 9):
            cx, cy = 8.0 * k, 8.0 * fam
            if fam == 0:
                depth = [0] * k
            elif fam == 1:
                depth = list(rng.permutation(k))
            else:
                depth = list(rng.permutation([j // 2 for j in range(k)]))
            for d in depth:
                z = float(d) / 64.0
                tris.append([[cx - 1, cy - 1, z], [cx + 1, cy - 1, z], [cx, cy + 1, z]])
                cluster.append(fam * 8 + k - 1)
    return np.array(tris, np.float32), np.array(cluster)


def _write_scene(tmp_path, tris):
    with open(tmp_path / "clusters.obj", "w") as f:
        for t in tris:
            for v in t:
                f.write("v %r %r %r\n" % (float(v[0]), float(v[1]), float(v[2])))
        for i in range(len(tris)):
            f.write("f %d %d %d\n" % (3 * i + 1, 3 * i + 2, 3 * i + 3))
    xml = tmp_path / "clusters.xml"
    xml.write_text("""<?xml version='1.0' encoding='utf-8'?>
<scene version="0.5.0">
    <dpt>
        <string  name="integrator" value="mcmc"/>
        <integer name="maxdepth" value="4"/>
        <boolean name="bidirectional" value="true"/>
        <boolean name="mala" value="true"/>
    </dpt>
    <sensor type="perspective">
        <float name="fov" value="40"/>
        <transform name="toWorld"><lookat target="36, 8, 0" origin="36, 8, 90" up="0, 1, 0"/></transform>
        <film type="hdrfilm"><integer name="width" value="64"/><integer name="height" value="48"/><rfilter type="box"/></film>
    </sensor>
    <bsdf type="diffuse" id="m"><rgb name="reflectance" value=".5,.5,.5"/></bsdf>
    <emitter type="point"><point name="position" x="36" y="8" z="50"/><spectrum name="intensity" value="100, 100, 100"/></emitter>
    <shape type="obj"><string name="filename" value="clusters.obj"/><ref id="m"/></shape>
</scene>
""")
    return str(xml)


def _rays(tris, cluster):
    """a few hundred oblique rays through the clusters from both sides (a third with a finite tfar), and some that miss everything"""
    rng = np.random.default_rng(12)
    rays = []
    for c in range(cluster.max() + 1):
        t0 = tris[np.nonzero(cluster == c)[0][0]]
        cen = t0.mean(axis=0)
        for side in (1.0, -1.0):
            for _ in range(6):
                tgt = cen + np.array([rng.uniform(-0.45, 0.45), rng.uniform(-0.45, 0.45), 0.0])
                org = np.array([tgt[0] + rng.uniform(-1.5, 1.5), tgt[1] + rng.uniform(-1.5, 1.5), side * rng.uniform(2.0, 4.0)])
                d = tgt - org
                rays.append(list(org) + list(d / np.linalg.norm(d)) + [5e-4, np.inf])
    for _ in range(40):  # between the clusters
        org = np.array([rng.uniform(0, 72), rng.uniform(-4, 20) // 8 * 8 + 4.0, 3.0])
        d = np.array([rng.uniform(-0.05, 0.05), rng.uniform(-0.05, 0.05), -1.0])
        rays.append(list(org) + list(d / np.linalg.norm(d)) + [5e-4, np.inf])
    rays = np.array(rays, np.float32)
    rays[::3, 7] = rng.uniform(2.0, 6.0, len(rays[::3])).astype(np.float32)
    return rays


def _brute(tris, rays):
    """TriTest (dscene.h) on every triangle, float32, one rounding per operation, the operations in the device's order.
    -> (closest id or -1 with ties to the lower id, its t or 0, any hit inside [tnear, tfar])"""
    f = np.float32
    p0, e1, e2 = tris[:, 0], tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0]

    def cross(a, b):
        return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2], a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)

    def dot(a, b):
        return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]

    prim, tt, occ = np.full(len(rays), -1, np.int32), np.zeros(len(rays), f), np.zeros(len(rays), np.int32)
    with np.errstate(divide="ignore", invalid="ignore"):
        for i, r in enumerate(rays):
            org, d, tnear, tfar = r[0:3][None, :], r[3:6][None, :], r[6], r[7]
            s1 = cross(np.broadcast_to(d, e2.shape), e2)
            div = dot(s1, e1)
            inv = f(1.0) / div
            s = org - p0
            u = dot(s, s1) * inv
            s2 = cross(s, e1)
            v = dot(np.broadcast_to(d, s2.shape), s2) * inv
            t = dot(e2, s2) * inv
            hit = (div != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t >= tnear) & (t <= tfar)
            assert s1.dtype == u.dtype == t.dtype == np.float32
            if hit.any():
                tm = t[hit].min()
                prim[i], tt[i], occ[i] = int(np.nonzero(hit & (t == tm))[0][0]), tm, 1
    return prim, tt, occ


@pytest.fixture(scope="module")
def clusters(tmp_path_factory):
    tris, cluster = _cluster_mesh()
    rays = _rays(tris, cluster)
    return _write_scene(tmp_path_factory.mktemp("clusters"), tris), tris, cluster, rays, _brute(tris, rays)


@pytest.mark.parametrize("tight", ["1", "0"])
@pytest.mark.parametrize("max_leaf", ["8", "default"])
def test_walks_on_leaves_of_one_to_eight_triangles_against_brute_force(clusters, max_leaf, tight, monkeypatch):
    xml, tris, cluster, rays, (bprim, bt, bocc) = clusters
    assert 300 <= len(rays) <= 500 and len(tris) == 3 * 36
    # test set-up: the brute force meets what the mesh was built for
    assert (bprim >= 0).mean() > 0.5 and (bprim < 0).sum() >= 20
    fam_a = cluster[np.maximum(bprim, 0)] < 8
    first_of_cluster = np.array([np.nonzero(cluster == c)[0][0] for c in cluster[np.maximum(bprim, 0)]])
    assert ((bprim < 0) | ~fam_a | (bprim == first_of_cluster)).all(), "coincident copies: the brute force itself must return the lowest id"
    if max_leaf != "default":
        monkeypatch.setenv("LMC_BVH_LEAF", max_leaf)  # read when the scene is loaded (host/accel.cpp)
    monkeypatch.setenv("LMC_TRACE_TIGHT", tight)  # read at every probe call (host/probes.cpp)
    ren = gc.pkg().Renderer(xml, force_diffuse=1, max_depth=4, width=64, height=48, seed_offset=0, use_gradient=0)
    assert ren.num_tris == len(tris)
    hist = ren.lean_info()["leaf_hist"]  # leaves that hold 1 .. 8 triangles
    print("leaf sizes 1 .. 8:", hist)
    assert sum((k + 1) * h for k, h in enumerate(hist)) == len(tris)
    if max_leaf == "8":
        assert hist == [3] * 8, "test set-up: every cluster of k triangles must be ONE leaf (three families x sizes 1 .. 8)"
    else:
        assert hist[4:] == [0] * 4 and all(h >= 3 for h in hist[:4]), "test set-up: leaves of 1, 2, 3 and 4 triangles, none larger"
    prim, t = ren.trace(rays)
    occ = ren.occluded(rays)
    ren.close()
    print(dict(max_leaf=max_leaf, tight=tight, rays=len(rays), hits=int((bprim >= 0).sum()), prim_mismatch=int((prim != bprim).sum()),
               t_mismatch=int((t != bt).sum()), occ_mismatch=int((occ != bocc).sum())))
    assert np.array_equal(prim, bprim)
    assert np.array_equal(t, bt)
    assert np.array_equal(occ, bocc)
