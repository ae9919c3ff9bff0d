"""`-m gpu` tier, second shipped scene (scenes/veachdoor/lmc.xml: BASELINE.json configs[3]): OBJ meshes, JPEG textures with
uvscale, twosided BSDFs, a rough-dielectric teapot and an AREA light -- the emitter code (arealight.cpp:12-104: SampleDirect,
Emission, Emit; trianglemesh.cpp:291-365 area sampling) that the torus scene (one environment light) never reaches."""
import os

import numpy as np
import pytest

from tests import _orc
from tests import gpu_checks as gc

pytestmark = pytest.mark.gpu
DOOR = os.path.join(gc.ROOT, "scenes", "veachdoor", "lmc.xml")


@pytest.fixture(scope="module")
def L():
    return gc.oracle_lib()


def test_door_scene_loads_and_rays_match(L):
    orc = _orc.Oracle(L, DOOR, 0, 8, 160, 90, 0, gc.pathref())
    ren = gc.pkg().Renderer(DOOR, width=160, height=90, seed_offset=0)
    assert ren.num_tris == orc.num_tris == 20764 and ren.num_lights == 1
    assert np.array_equal(orc.scene_params(), ren.scene_params())
    rng = np.random.default_rng(3)
    n = 100000
    org = np.array([-71.39, 71.49, 205.3]) + rng.normal(0, 40, (n, 3))
    d = rng.normal(0, 1, (n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.zeros((n, 8), np.float32)
    rays[:, :3], rays[:, 3:6], rays[:, 6], rays[:, 7] = org, d, 5e-4, np.inf
    rays[: n // 3, 7] = rng.uniform(20, 300, n // 3)
    prim, t = ren.trace(rays)
    oprim, ot = np.zeros(n, np.int32), np.zeros(n, np.float32)
    L.orc_trace(orc.h, n, _orc.P(rays), _orc.P(oprim), _orc.P(ot))
    assert (oprim >= 0).mean() > 0.5
    assert np.array_equal(prim, oprim) and np.array_equal(t, ot)  # tree-independent closest hit: bit-identical
    occ, oocc = ren.occluded(rays), np.zeros(n, np.int32)
    L.orc_occluded(orc.h, n, _orc.P(rays), _orc.P(oocc))
    assert np.array_equal(occ, oocc)
    orc.close()
    ren.close()


def _hist_l1(r):
    keys = set(r["hist_oracle"]) | set(r["hist_gpu"])
    return sum(abs(r["hist_oracle"].get(k, 0.0) - r["hist_gpu"].get(k, 0.0)) for k in keys)


@pytest.mark.parametrize("use_gradient,oracle_grad", [(0, "reference"), (1, "product"), (1, "reference")])
def test_door_chain_parity(use_gradient, oracle_grad):
    """MLTInit + 60 lock-step mutations of 2048 chains on the door scene, GPU vs oracle: area-light sampling in every large step (EmitFromLight,
    DirectLighting, hitting the emitter), twosided Lambertian / Phong, textured reflectances.

    Until round 6 this comparison was statistical (counts within 1-3 %, histogram L1 < 0.08): the room is ~400 units across with centimetre-scale
    features, one ulp between the device libm's sinf / cosf and glibc's moved a hit point by ~3e-5, about one init sample in 400 took another
    Russian-roulette branch, and MLTInit seeds its resampling stream with the NUMBER of contributions (mlt.h:115), so a single flipped sample re-seeded
    every chain (profiles/r02_d_door_init_diff.txt).  With one deterministic sin / cos / acos / atan2 on both sides (device/dtrig.h) and glibc's logf
    restated for the normal variates (drng.h) the chains are the oracle's, one by one -- what test_chain_loop_parity asserts on the torus holds here:
      * without gradients, and with the oracle drawing its gradients from the product's path program compiled for the host: EXACT -- contributions,
        normalization, every init state, large steps, accepted steps, gradient calls, every final state; film 1e-6 (atomics' order);
      * with the oracle on the reference's generated derivative programs (1e-2 from the product's, test_full_material_gradient_kernel_*): a chain whose
        accept decision the gradients flip diverges; measured 2037 / 2048 final states equal, large steps 27722 / 27715 (profiles/r06_h_door_parity.jsonl)."""
    r = gc.run_pair(160, 90, 40000, 2048, 40000, 400, 60, use_gradient=use_gradient, max_depth=8, scene=DOOR, force_diffuse=0, oracle_grad=oracle_grad)
    assert r["contribs_gpu"] == r["contribs_oracle"] and r["norm_gpu"] == r["norm_oracle"]
    assert r["init_cl_match"] == 1.0 and r["init_ls_relerr_max"] == 0.0 and r["init_pss_maxdiff"] == 0.0
    so, sg = r["stats_oracle"], r["stats_gpu"]
    assert sg["steps"] == so["steps"] == 2048 * 60
    if use_gradient == 0 or oracle_grad == "product":
        for k in ("largeSteps", "accepted", "gradCalls"):
            assert sg[k] == so[k], (k, sg[k], so[k])
        assert r["final_state_match"] == 1.0 and r["film_rel_l2"] < 1e-6
        assert r["hist_gpu"] == r["hist_oracle"]
    else:
        assert abs(sg["largeSteps"] - so["largeSteps"]) <= 30 and abs(sg["accepted"] - so["accepted"]) <= 40 and abs(sg["gradCalls"] - so["gradCalls"]) <= 60
        assert r["final_state_match"] > 0.985 and r["film_rel_l2"] < 0.1 and _hist_l1(r) < 0.02
    if use_gradient:
        assert sg["gradCalls"] > 10000
    assert abs(r["film_sum_gpu"] / r["film_sum_oracle"] - 1) < 1e-6
    assert r["nonfinite_gpu"] == 0
    # film luminance / (normalization x splat weights): below 1 by the splats both sides DROP as non-finite (image.h:72): states with a
    # denormal lsScore (3e-39 occurs in this scene) give normalization / lsScore = inf.  Same deficit on both sides.
    assert 0.99 < r["energy_gpu"] <= 1.0001 and abs(r["energy_gpu"] - r["energy_oracle"]) < 1e-6


def test_door_diffuse_chain_parity():
    """every BSDF forced to `diffuse`, gradients on (the oracle's from the reference's programs): the init is exact, the chains diverge only where the two
    gradient implementations flip an accept decision (see test_door_chain_parity)"""
    grad = 1 if gc.pathref() else 0
    r = gc.run_pair(160, 90, 40000, 2048, 40000, 400, 60, use_gradient=grad, max_depth=6, scene=DOOR, force_diffuse=1)
    assert r["contribs_gpu"] == r["contribs_oracle"] and r["norm_gpu"] == r["norm_oracle"]
    assert r["init_cl_match"] == 1.0 and r["init_ls_relerr_max"] == 0.0 and r["init_pss_maxdiff"] == 0.0
    so, sg = r["stats_oracle"], r["stats_gpu"]
    if grad:
        assert abs(sg["largeSteps"] - so["largeSteps"]) <= 30 and abs(sg["accepted"] - so["accepted"]) <= 40
        assert r["final_state_match"] > 0.985 and _hist_l1(r) < 0.02, (r["final_state_match"], r["hist_oracle"], r["hist_gpu"])
    else:
        assert sg["largeSteps"] == so["largeSteps"] and sg["accepted"] == so["accepted"] and r["final_state_match"] == 1.0
    assert abs(r["film_sum_gpu"] / r["film_sum_oracle"] - 1) < 1e-6
    assert 0.99 < r["energy_gpu"] <= 1.0001 and abs(r["energy_gpu"] - r["energy_oracle"]) < 1e-6


def test_door_render_matches_reference_image():
    """GPU render of the shipped scene file, reference semantics, 1024 chains x 23 k mutations at 320x180 (420 spp), against the
    reference authors' render (tests/golden/veachdoor_ref_images_320x180.npz = scenes/veachdoor/lmc_timeuse_30.236183s.exr
    box-downsampled 4x).  The two renders the reference ships for this scene differ by relMSE 0.031, so the bars are on means:
    image 3 %, 3x4 grid of regions 12 % (the CPU oracle meets the same bars, tests/test_scene_io.py)."""
    p = gc.pkg()
    ref = np.load(os.path.join(gc.ROOT, "tests", "golden", "veachdoor_ref_images_320x180.npz"))["lmc"]
    lum = lambda x: x @ np.array([0.212671, 0.715160, 0.072169])
    lr = lum(ref)
    W, H, dspp, spp, chains = 320, 180, 32, 420, 1024
    ren = p.Renderer(DOOR, width=W, height=H, seed_offset=0)
    direct = ren.direct_lighting(dspp)
    per = spp * W * H // chains
    ren.init_chains(300000, chains, 8192, per, per % chains)
    done = 0
    while done < per + 1:
        ren.step(min(4096, per + 1 - done))
        done += 4096
    lg = lum(direct / dspp + ren.film() / spp)
    st = ren.stats()
    ren.close()
    assert np.isfinite(lg).all()
    assert abs(lg.mean() / lr.mean() - 1) < 0.03
    for gy in range(3):
        for gx in range(4):
            a, b = lg[gy * 60:(gy + 1) * 60, gx * 80:(gx + 1) * 80].mean(), lr[gy * 60:(gy + 1) * 60, gx * 80:(gx + 1) * 80].mean()
            assert abs(a / b - 1) < 0.12, (gy, gx, a / b)
    assert st["cacheReadyMask"] != 0


def test_door_init_contributions_per_sample():
    """Tightens the statistical door comparison where it can be tightened: BEFORE the count-seeded resampling (mlt.h:115), MLTInit's
    contributions are compared sample by sample through lmc_init_contribs / orc_init_contribs (same streams: init sample k of
    stream t on both sides).  A sample agrees if both sides emit the same list of techniques with lsScores within 1e-3 relative
    (the scene's scale turns one ulp of sinf / cosf into 1e-5 .. 1e-4, profiles/r02_d_door_init_diff.txt).  >= 99 % of the
    samples must agree exactly in technique list, >= 98.5 % also in every score; the rest took another Russian-roulette branch."""
    import ctypes
    from collections import defaultdict
    from tests._orc import P

    L = gc.oracle_lib()
    p = gc.pkg()
    ninit, nth = 40000, 40000  # one stream per sample: a flipped branch stays local to its sample
    orc = _orc.Oracle(L, DOOR, 0, 8, 160, 90, 0, "")
    ren = p.Renderer(DOOR, max_depth=8, width=160, height=90, seed_offset=0, use_gradient=0)
    orc.init(ninit, 64, nth)
    ren.init_chains(ninit, 64, nth, 10)

    def dump(fn, h):
        cap = 8 * ninit
        s, cl, ls = np.zeros(cap, np.int64), np.zeros(cap, np.int32), np.zeros(cap, np.float32)
        fn.restype = ctypes.c_longlong
        fn.argtypes = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        n = fn(h, cap, P(s), P(cl), P(ls))
        assert n <= cap
        d = defaultdict(list)
        for a, b, c in zip(s[:n], cl[:n], ls[:n]):
            d[int(a)].append((int(b), float(c)))
        return d, n

    do, no = dump(L.orc_init_contribs, orc.h)
    dg, ng = dump(p.lib().lmc_init_contribs, ren.h)
    orc.close()
    ren.close()
    assert no > 8000 and abs(no - ng) <= 0.01 * no  # about one contribution per three init samples on this scene
    same_cl = same_all = 0
    for k in range(ninit):
        a, b = do.get(k, []), dg.get(k, [])
        if [x[0] for x in a] == [x[0] for x in b]:
            same_cl += 1
            same_all += all(abs(x[1] - y[1]) <= 1e-3 * abs(x[1]) for x, y in zip(a, b))
    assert same_cl >= 0.99 * ninit, same_cl
    assert same_all >= 0.985 * ninit, same_all


def test_door_light_coordinate_sampling():
    """SURVEY §8(f) item 4, `uselightcoordinatesampling` (path.cpp:1339-1360 GeneratePathBidir, :1881-1951 LightCoordinateSampling,
    :2120-2150 PerturbPathBidir, trianglemesh.cpp:238-285 GetSampleParam; derivative programs: the doLightCoordinateSampling branch,
    path.cpp:2979-3025): a camera path that ends on an area light keeps its last bounce in the light's own sampling coordinates.
    (1) The shipped scene with an area light, option on, 60 lock-step mutations of 2048 chains: the statistical bars of
        test_door_chain_parity (chain-by-chain comparison is impossible on this scene).
    (2) scenes/torus/lmc_arealight.xml (ours: the floor of the torus scene as the emitter, scenes/README.md), every BSDF diffuse: state by state.
        MLTInit: every init state equal (technique, lsScore, ssScore, pss) with the option on AND off, and the states that end on
        the emitter differ between the two runs (the re-parameterised ssJacobian and bsdfRndParam); 40 mutations: identical step counters,
        film within 5e-3 (a handful of 8192 chains flip one accept); the product's path program == the reference's programs with scene[0] = 1 on the emitter-hit states."""
    L = gc.oracle_lib()
    p = gc.pkg()
    r = gc.run_pair(160, 90, 40000, 2048, 40000, 400, 60, use_gradient=1, max_depth=8, scene=DOOR, force_diffuse=0, oracle_grad="reference",
                    opts={"uselightcoordinatesampling": 1})
    so, sg = r["stats_oracle"], r["stats_gpu"]
    assert abs(r["contribs_gpu"] - r["contribs_oracle"]) <= 0.01 * r["contribs_oracle"]
    assert abs(r["norm_gpu"] - r["norm_oracle"]) <= 2e-3 * r["norm_oracle"]
    assert sg["steps"] == so["steps"] == 2048 * 60
    assert abs(sg["largeSteps"] - so["largeSteps"]) <= 0.03 * so["largeSteps"]
    assert abs(sg["accepted"] - so["accepted"]) <= 0.02 * so["accepted"]
    assert abs(sg["gradCalls"] - so["gradCalls"]) <= 0.03 * max(so["gradCalls"], 100) and sg["gradCalls"] > 0
    assert _hist_l1(r) < 0.08
    assert abs(r["film_sum_gpu"] / r["film_sum_oracle"] - 1) < 0.01 and r["nonfinite_gpu"] == 0
    # (2)
    AREA = os.path.join(gc.ROOT, "scenes", "torus", "lmc_arealight.xml")
    ninit, n, streams = 1 << 17, 1 << 13, 4096
    emitter_ss = {}
    for flag in (1, 0):
        orc = _orc.Oracle(L, AREA, 1, 6, 160, 120, 0, gc.pathref())
        ren = p.Renderer(AREA, force_diffuse=1, max_depth=6, width=160, height=120, seed_offset=0, use_gradient=1)
        L.orc_set_option(orc.h, b"uselightcoordinatesampling", float(flag))
        ren.set_option("uselightcoordinatesampling", flag)
        no, co = orc.init(ninit, n, streams)
        ng, cg = ren.init_chains(ninit, n, streams, 10)
        assert co == cg and abs(no - ng) <= 1e-5 * no
        si, gi = orc.summary(1), ren.summary(1)
        sp = ren.scene_params()
        assert sp[0] == float(flag) and np.array_equal(sp, orc.scene_params())
        assert np.array_equal(si[:, 1:3], gi[:, 1:3])
        # one state of 8192 sits on an ill-conditioned path (2e-4 relative, 1.5e-3 in one pss entry): scripts/debug/arealight_state_diff.py
        assert np.allclose(si[:, 3], gi[:, 3], rtol=1e-3) and np.allclose(si[:, 4], gi[:, 4], rtol=1e-3)
        assert (np.abs(si[:, 3] / gi[:, 3] - 1) > 1e-5).sum() <= 8 and (np.abs(si[:, 16:] - gi[:, 16:]).max(axis=1) > 1e-5).sum() <= 8
        emit, n_emit = gc.emitter_end_states(orc, si)
        assert n_emit >= 1000, n_emit
        if flag:
            for (i, c, l, prim, vert), (rll, rg) in zip(emit, gc.ref_evals("lightcoord_arealight", orc, emit)):
                ll, g = p.grad_batch(c, l, prim[: 2 * (c + l - 1) + 1, None].copy(), sp, vert[: 238 + 59 * (c + l - 3), None].copy())
                assert abs(ll[0] - rll) < 2e-3 and np.linalg.norm(rg - g[:, 0]) <= 1e-2 * max(np.linalg.norm(rg), 1e-2), (i, c, l)
        emitter_ss[flag] = {i: (float(si[i, 4]), si[i, 16:].copy()) for i, *_ in emit}
        orc.close()
        ren.close()
    common = set(emitter_ss[0]) & set(emitter_ss[1])
    assert len(common) >= 30
    for i in common:  # the option re-parameterises exactly these states: another ssScore, another pss at the last bounce
        assert abs(emitter_ss[1][i][0] / emitter_ss[0][i][0] - 1) > 1e-3 and np.abs(emitter_ss[1][i][1] - emitter_ss[0][i][1]).max() > 1e-4
    r = gc.run_pair(160, 120, 1 << 17, 1 << 13, 4096, 400, 40, use_gradient=1, max_depth=6, scene=AREA, force_diffuse=1, oracle_grad="reference",
                    opts={"uselightcoordinatesampling": 1})
    so, sg = r["stats_oracle"], r["stats_gpu"]
    assert r["contribs_gpu"] == r["contribs_oracle"] and r["init_cl_match"] == 1.0
    assert sg["steps"] == so["steps"]
    # the oracle draws its gradients from the reference's programs, the device from its own (1e-2 apart): a chain whose accept decision they flip
    # consumes its stream differently from then on -- a large step more or less per such chain (round 6: 101381 vs 101382)
    assert abs(sg["largeSteps"] - so["largeSteps"]) <= 2, (sg["largeSteps"], so["largeSteps"])
    assert abs(sg["accepted"] - so["accepted"]) <= 4 and abs(sg["gradCalls"] - so["gradCalls"]) <= 4
    assert r["film_rel_l2"] < 5e-3 and r["final_state_match"] > 0.998 and abs(r["energy_gpu"] - 1.0) < 1e-4, (r["film_rel_l2"], r["final_state_match"], r["energy_gpu"])
