"""Generates tests/golden/ref_runs/: the oracle's side of the GPU chain-parity runs whose oracle draws its gradients (and H2MC Hessians)
from the reference's generated derivative programs (oracle/_ref/libpathref.so, built by `make -f oracle/Makefile.ref` from the reference
tree), so that those GPU tests hold where the programs are not built.  One file per run_pair configuration (tests/gpu_checks.py:
oracle_run_config, keyed by its hash) with the figures run_pair compares -- normalization, contributions, init and final chain summaries,
step counters, film -- and the reference programs' (log-luminance, gradient) on the emitter-ending init states of
test_door_light_coordinate_sampling.  Run in the build container only (no GPU: the oracle is host code); the output is data."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests import _orc  # noqa: E402
from tests import gpu_checks as gc  # noqa: E402

DOOR = os.path.join(ROOT, "scenes", "veachdoor", "lmc.xml")
AREA = os.path.join(ROOT, "scenes", "torus", "lmc_arealight.xml")
POINT = os.path.join(ROOT, "scenes", "torus", "lmc_pointlight.xml")
H2 = {"h2mc": 1, "largestepprob": 0.2, "perturbstddev": 0.01}
LC = {"uselightcoordinatesampling": 1}

# the run_pair(..., use_gradient=1, oracle_grad="reference") calls of the GPU tests that run without a skip where oracle/_ref is absent
RUNS = [
    ((160, 90, 40000, 2048, 40000, 400, 60), dict(max_depth=8, scene=DOOR, force_diffuse=0)),  # test_door_chain_parity[1-reference]
    ((160, 90, 40000, 2048, 40000, 400, 60), dict(max_depth=8, scene=DOOR, force_diffuse=0, opts=LC)),  # test_door_light_coordinate_sampling
    ((160, 120, 1 << 17, 1 << 13, 4096, 400, 40), dict(max_depth=6, scene=AREA, force_diffuse=1, opts=LC)),  # test_door_light_coordinate_sampling
    ((160, 120, 40000, 256, 8, 400, 30), dict(opts=H2)),  # test_h2mc_chain_parity_diffuse
    ((160, 120, 20000, 256, 20000, 400, 30), dict(max_depth=8, force_diffuse=0, opts=H2)),  # test_h2mc_chain_parity_full_materials
    ((160, 120, 40000, 2048, 8, 400, 6), dict(opts=H2)),  # test_h2mc_per_step_agreement[1]
    ((160, 120, 40000, 2048, 40000, 400, 6), dict(max_depth=8, force_diffuse=0, opts=H2)),  # test_h2mc_per_step_agreement[0]
    ((160, 120, 20000, 256, 20000, 400, 40), dict(max_depth=12, force_diffuse=0)),  # test_maxdepth_12_chain_parity
    ((40, 25, 20000, 4, 20000, 1000, 1000), dict(max_depth=8, force_diffuse=1)),  # test_cfg1_twin_four_chains_thousand_mutations[1]
    ((40, 25, 20000, 4, 20000, 1000, 1000), dict(max_depth=8, force_diffuse=0)),  # test_cfg1_twin_four_chains_thousand_mutations[0]
    ((160, 120, 20000, 256, 20000, 400, 40), dict(max_depth=8, scene=POINT, force_diffuse=1)),  # test_point_light_scene_chain_parity[1]
    ((160, 120, 20000, 256, 20000, 400, 40), dict(max_depth=8, scene=POINT, force_diffuse=0)),  # test_point_light_scene_chain_parity[0]
]


def lightcoord_arealight_evals():
    """test_door_light_coordinate_sampling (2), option on: the reference programs on the sampled emitter-ending init states"""
    L = gc.oracle_lib()
    orc = _orc.Oracle(L, AREA, 1, 6, 160, 120, 0, gc.pathref())
    L.orc_set_option(orc.h, b"uselightcoordinatesampling", 1.0)
    orc.init(1 << 17, 1 << 13, 4096)
    emit, _ = gc.emitter_end_states(orc, orc.summary(1))
    lls, gs = [], []
    for _, c, l, prim, vert in emit:
        ll, g = orc.ref_eval(c, l, prim, vert)
        lls.append(ll)
        gs.append(np.pad(g, (0, 16 - len(g))))
    orc.close()
    np.savez_compressed(os.path.join(gc.REF_RUNS, "ref_eval_lightcoord_arealight.npz"), index=np.array([e[0] for e in emit], np.int64),
                        loglum=np.array(lls, np.float32), grad=np.array(gs, np.float32))


def main():
    assert gc.pathref(), "needs oracle/_ref/libpathref.so"
    os.makedirs(gc.REF_RUNS, exist_ok=True)
    for a, k in RUNS:
        cfg = gc.oracle_run_config(*a, **k)
        gc.save_ref_run(cfg, gc.oracle_run(cfg, gc.pathref()))
        print(os.path.relpath(gc.ref_run_path(cfg), ROOT), os.path.getsize(gc.ref_run_path(cfg)), flush=True)
    lightcoord_arealight_evals()


if __name__ == "__main__":
    main()
