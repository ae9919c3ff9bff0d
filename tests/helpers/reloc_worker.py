#!/usr/bin/env python3
"""TEST HELPER: one render with chain relocation on, recorded at several points: every chain's summary row, the counters, the relocation counters and
the slot tables (lmc_chain_slots).  tests/test_gpu_lists.py imports run() for the default library configuration and starts this file as a fresh
process for the variants that the library reads from the environment once per process (LMC_RELOC_COOP=0, LMC_RELOC_FINE=1).
usage: reloc_worker.py <out.npz> <chains>[,<chains>...]      (plain MLT, the torus at 128 x 96, 12 steps, recorded after steps 1, 6 and 12)"""
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
POINTS = (1, 6, 12)
PLAIN_OPTS = {"largestepprob": 0.3, "largestepscale": 1.0}


def run(n_chains, mala, opts, points=POINTS, max_depth=6, resort_every=2, resort_first=0):
    """-> ([(summary, stats, relocation stats, slot_of, chain_id) per point], film); the set-up of tests/test_gpu_relocate.py _run with relocation on"""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    p = importlib.import_module("langevin-mcmc_amd")
    os.environ["LMC_RELOCATE"] = "1"
    try:
        ren = p.Renderer(os.path.join(ROOT, "scenes", "torus", "lmc.xml"), force_diffuse=1, max_depth=max_depth, width=128, height=96, seed_offset=0, use_gradient=1)
        for k, v in opts.items():
            ren.set_option(k, v)
        if not mala:
            ren.set_option("mala", 0)
        ren.set_option("resort_every", resort_every)
        ren.set_option("resort_first", resort_first)
        ren.init_chains(200000, n_chains, 64, 10 ** 6)
    finally:
        del os.environ["LMC_RELOCATE"]
    out, done = [], 0
    for upto in points:
        ren.step(upto - done)
        done = upto
        slot_of, chain_id = ren.chain_slots()
        out.append((ren.summary(0).copy(), ren.stats(), ren.relocation_stats(), slot_of, chain_id))
    film = ren.film().copy()
    ren.close()
    return out, film


if __name__ == "__main__":
    save = {}
    for n in [int(x) for x in sys.argv[2].split(",")]:
        out, film = run(n, False, PLAIN_OPTS)
        save["film_%d" % n] = film
        for k, (summ, st, rs, slot_of, chain_id) in enumerate(out):
            save["summary_%d_%d" % (n, k)], save["slot_of_%d_%d" % (n, k)], save["chain_id_%d_%d" % (n, k)] = summ, slot_of, chain_id
            save["stats_%d_%d" % (n, k)], save["reloc_%d_%d" % (n, k)] = json.dumps(st), json.dumps(rs)
    np.savez(sys.argv[1], **save)
