"""`-m gpu` tier: the step kernels read their launch arguments through the kernel-argument segment (step_kernel.h StepKernArgs,
KernArgs) and the lean launch runs one chain per thread without a grid-stride loop.  Nothing the kernels compute may move:
every case below is the chain-exact comparison with the CPU oracle of test_gpu_parity.py::test_chain_loop_parity -- contributions,
normalization, init states, counters and every chain's final state equal, the film up to the order of its float atomics -- at the edges of
the launch geometry: one lane, a ragged wave (63), two blocks (65), many blocks (1 000).

No gradients (use_gradient=0): every small step then takes the lean launch from the first mutation on, every large step the large-step launch.
maxdepth 6: states of dimension 12 fill all 24 staging words of the lean kernel's LDS stack region.

The private-stack instantiations (the fallback of trees deeper than the 40-entry LDS stack; neither shipped scene has one) run through the switches
LMC_LEAN_LDS=0 and LMC_LARGE_LDS=0 of host/context.cpp: the launches then take those instantiations on a tree that would fit, with their LDS still
sized from the tree's real stack need.  The context reports no query for which instantiation a launch took, so these cases cannot assert that a
switch was honoured; host/context.cpp reads the variables next to each other when a context is created.

Run times on an MI355X: every case 0.2 - 1.5 s, the 1.5 x 2^20-chain coverage case 0.8 s."""
import os

import pytest

from tests import gpu_checks as gc

pytestmark = pytest.mark.gpu
DOOR = os.path.join(gc.ROOT, "scenes", "veachdoor", "lmc.xml")
COUNTERS = ("largeSteps", "accepted", "gradCalls", "cacheQueries", "cacheHits", "resets", "cacheReadyMask")


def _assert_chain_exact(r, n_chains, steps):
    print({k: r[k] for k in ("film_rel_l2", "final_state_match", "energy_gpu", "init_cl_match")}, r["stats_gpu"])
    assert r["contribs_gpu"] == r["contribs_oracle"] and r["norm_gpu"] == r["norm_oracle"]
    assert r["init_cl_match"] == 1.0 and r["init_ls_relerr_max"] == 0.0 and r["init_pss_maxdiff"] == 0.0
    so, sg = r["stats_oracle"], r["stats_gpu"]
    assert sg["steps"] == so["steps"] == n_chains * steps
    for k in COUNTERS:
        assert sg[k] == so[k], (k, sg[k], so[k])
    assert r["final_state_match"] == 1.0
    assert r["film_rel_l2"] < 1e-4  # float add order of the splats, as in test_chain_loop_parity
    assert r["nonfinite_gpu"] == 0


@pytest.mark.parametrize("n_chains", [1, 63, 65, 1000])
def test_torus_chain_exact_at_the_edges_of_the_launch(n_chains):
    """30 lock-step mutations, Lambertian torus: the lightless lean instantiation on quantised nodes (the headline's) and the large-step launch"""
    r = gc.run_pair(96, 72, 20000, n_chains, 64, 400, 30, use_gradient=0, max_depth=6, opts={"largestepprob": 0.3, "largestepscale": 1.0})
    _assert_chain_exact(r, n_chains, 30)


def test_torus_chain_exact_through_the_cache_ready_transition():
    """1 000 chains need 150 mutations for the cache of dimension 6 to fill (3 000 rows): from then on the lean launch queries it
    (the oracle counts 21 679 queries in this run).  Same bars."""
    r = gc.run_pair(96, 72, 20000, 1000, 64, 400, 150, use_gradient=0, max_depth=6, opts={"largestepprob": 0.3, "largestepscale": 1.0})
    assert r["stats_oracle"]["cacheReadyMask"] != 0 and r["stats_oracle"]["cacheQueries"] > 10000, "test set-up: the cache never filled"
    _assert_chain_exact(r, 1000, 150)


@pytest.mark.parametrize("n_chains", [1, 63, 65, 1000])
def test_door_chain_exact_at_the_edges_of_the_launch(n_chains):
    """30 lock-step mutations on the door scene with its own materials: the glossy lean instantiation WITH light sub-paths on exact nodes,
    the glossy large-step launch (three waves per SIMD).  (The door's caches do not fill with 1 000 chains in any run of a test's length.)"""
    r = gc.run_pair(96, 54, 20000, n_chains, 20000, 400, 30, use_gradient=0, max_depth=6, scene=DOOR, force_diffuse=0,
                    opts={"largestepprob": 0.3, "largestepscale": 1.0})
    _assert_chain_exact(r, n_chains, 30)


@pytest.mark.parametrize("env", [{"LMC_LEAN_LDS": "0"}, {"LMC_LARGE_LDS": "0"}, {"LMC_BVH_NODES": "exact"}])
def test_torus_chain_exact_on_the_other_instantiations(env, monkeypatch):
    """the lean launch on its private-stack fallback (k_step_small<FILM, false, false>); the large-step launch with its traversal stack in private
    memory; both launches on the exact (128-byte) nodes"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    r = gc.run_pair(96, 72, 20000, 65, 64, 400, 30, use_gradient=0, max_depth=6, opts={"largestepprob": 0.3, "largestepscale": 1.0})
    _assert_chain_exact(r, 65, 30)


def test_door_chain_exact_on_the_lean_private_stack_fallback(monkeypatch):
    """the glossy fallback instantiation (k_step_small<FILM, false, true>), 65 chains x 30 mutations on the door"""
    monkeypatch.setenv("LMC_LEAN_LDS", "0")
    r = gc.run_pair(96, 54, 20000, 65, 20000, 400, 30, use_gradient=0, max_depth=6, scene=DOOR, force_diffuse=0,
                    opts={"largestepprob": 0.3, "largestepscale": 1.0})
    _assert_chain_exact(r, 65, 30)


def test_lean_launch_covers_a_population_larger_than_its_former_grid():
    """The lean launch used to cap its grid at 2^20 threads and stride over longer lists; it now runs one chain per thread.  With 1.5 x 2^20 chains and
    no large steps beyond those a fresh chain takes until its first acceptance, the lean launch's work list passes 2^20 entries within a few mutations.
    A chain the grid does not reach is neither stepped nor counted: every step must count every chain."""
    n = 3 << 19
    ren = gc.pkg().Renderer(gc.TORUS, force_diffuse=1, max_depth=6, width=160, height=120, seed_offset=0, use_gradient=0)
    ren.set_option("largestepprob", 0.0)
    ren.init_chains(8 * n, n, 65536, 64)  # as many init samples per chain as the benchmark takes
    longest, before = 0, ren.stats()
    for _ in range(10):
        ren.step(1)
        st = ren.stats()
        assert st["steps"] - before["steps"] == n
        longest = max(longest, n - (st["largeSteps"] - before["largeSteps"]))
        before = st
    ren.close()
    print("longest lean work list:", longest)
    assert longest > 1 << 20, "test set-up: no lean work list longer than the former grid"
