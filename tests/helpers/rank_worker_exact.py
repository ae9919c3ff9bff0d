#!/usr/bin/env python3
"""TEST HELPER: one rank PROCESS of a multi-rank job with the exact film (film_exact = 1): lmc_comm_init -> collective lmc_chains_init -> lmc_chains_step ->
lmc_film_allreduce over ncclInt64.  The communicator is tests/helpers/rccl_stub_i64.cpp (LMC_RCCL_LIB): all ranks share device 0.
usage: rank_worker_exact.py <rank> <world> <dir> <chains> <steps> <init samples> <init streams>"""
import importlib, os, sys, time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
rank, world, d, n, steps, ninit, streams = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], int(sys.argv[4]), int(sys.argv[5]), int(sys.argv[6]), int(sys.argv[7])
p = importlib.import_module("langevin-mcmc_amd")
sharding = importlib.import_module("langevin-mcmc_amd.sharding")
scene = os.path.join(ROOT, "scenes", "torus", "lmc.xml")
ren = p.Renderer(scene, force_diffuse=1, max_depth=6, width=96, height=72, seed_offset=0, device=0, use_gradient=1)
ren.set_option("film_exact", 1)
idf = os.path.join(d, "id.bin")
if rank == 0:
    open(idf + ".tmp", "wb").write(p.comm_unique_id())
    os.rename(idf + ".tmp", idf)
t0 = time.time()
while not os.path.exists(idf):
    if time.time() - t0 > 60:
        sys.exit("rank %d: no communicator id" % rank)
    time.sleep(0.01)
ren.comm_init(world, rank, open(idf, "rb").read())
b, e = sharding.group_ranges(n, world)[rank]
ren.init_chains(ninit, n, streams, steps, 0, b, e)
ren.step(steps)
own = ren.film_fixed()
ren.film_allreduce()
np.savez(os.path.join(d, "rank%d.npz" % rank), own=own, fixed=ren.film_fixed(), film=ren.film(), overflow=ren.film_overflow())
ren.comm_barrier()
ren.close()
