#!/usr/bin/env python3
"""TEST HELPER: one rank PROCESS of a two-rank job whose film is layered (film_exact = 1, film_layers = 2): lmc_comm_init -> collective lmc_chains_init ->
lmc_chains_step -> lmc_film_allreduce, which this version refuses on a communicator of more than one rank.  The communicator is
tests/helpers/rccl_stub_i64.cpp (LMC_RCCL_LIB): all ranks share device 0.
usage: rank_worker_film_layers.py <rank> <world> <dir>"""
import importlib, os, sys, time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
rank, world, d = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
n, steps, ninit, streams = 2048, 3, 1 << 15, 512
p = importlib.import_module("langevin-mcmc_amd")
sharding = importlib.import_module("langevin-mcmc_amd.sharding")
scene = os.path.join(ROOT, "scenes", "torus", "lmc.xml")
ren = p.Renderer(scene, force_diffuse=1, max_depth=6, width=96, height=72, seed_offset=0, device=0, use_gradient=1)
ren.set_option("film_exact", 1)
ren.set_option("film_layers", 2)
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
ren.init_chains(ninit, n, streams, 10 ** 6, 0, b, e)
ren.step(steps)
own = ren.film_layers_fixed()
try:
    ren.film_allreduce()
    sys.exit("rank %d: lmc_film_allreduce of a layered film over %d ranks was not refused" % (rank, world))
except RuntimeError as err:
    print("refused: %s" % err)
assert np.array_equal(own, ren.film_layers_fixed()), "the refused call changed the film"
ren.step(steps)
assert ren.stats()["steps"] == 2 * steps * (e - b) and not np.array_equal(own, ren.film_layers_fixed())
print("still steps")
ren.comm_barrier()
ren.close()
