#!/usr/bin/env python3
"""Cost of the chain diagnostics while they are ON, on the headline workload (Lambertian torus, max depth 6, 2^20 chains): ms per lock step over 64
steps, stream drained on both sides, for: both off / step table on (latch + k_step_table) / a trace of 4096 chains (latch + k_chain_rows) / both off
again.  One JSON line.   usage: scripts/measure_chain_diag.py [log2 chains, default 20]"""
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
p = importlib.import_module("langevin-mcmc_amd")
n = 1 << (int(sys.argv[1]) if len(sys.argv) > 1 else 20)
STEPS = 64
ren = p.Renderer(os.path.join(ROOT, "scenes", "torus", "lmc.xml"), force_diffuse=1, max_depth=6, seed_offset=0, use_gradient=1)
ren.init_chains(8 * n, n, 65536, 4096)
ren.step(64)  # past the cache-fill phase
ren.sync()


def leg():
    ren.sync()
    t0 = time.perf_counter()
    ren.step(STEPS)
    ren.sync()
    return (time.perf_counter() - t0) * 1e3 / STEPS


out = {"chains": n, "steps_per_leg": STEPS, "ready_mask": ren.stats()["cacheReadyMask"]}
out["off_ms"] = leg()
ren.set_option("step_table", 1)
out["table_ms"] = leg()
ren.set_option("step_table", 0)
table = ren.step_table()
out["table_steps"] = int(table[..., 0].sum())
ids = np.random.default_rng(1).choice(n, min(4096, n), replace=False).astype(np.int32)
ren.trace_chains(ids, STEPS)
out["trace4096_ms"] = leg()
first, dropped, rows = ren.trace_read()
ren.trace_end()
out["trace_rows"] = list(rows.shape)
out["off_again_ms"] = leg()
print(json.dumps(out))
