#!/usr/bin/env python3
"""Records of the layered MLT film (lmc_set_option "film_layers", device/step_*_layers.hip) beside the unlayered exact film: ms per lock step of the torus
headline (force_diffuse, maxdepth 6, 2^20 chains) and of veach-door LMC (2^18 chains), measured over `--steps` steps behind `--warmup` steps of a fresh
context (so the layered and the unlayered contexts run the same trajectories: the same work).  The three modes are ALTERNATED: every repetition is one
child process per mode.  One JSON line per measurement, every repetition kept so that the run-to-run spread shows.  No bar; a layered mode that costs
more than twice the exact unlayered step is to be diagnosed.
usage: python scripts/film_layers_sweep.py [--out profiles/r14_film_layers_sweep.jsonl] [--reps 3] [--steps 20] [--warmup 40]"""
import argparse
import importlib
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKLOADS = {
    "torus_headline": dict(xml=os.path.join(ROOT, "scenes", "torus", "lmc.xml"), force_diffuse=1, max_depth=6, chains=1 << 20),
    "veachdoor_lmc": dict(xml=os.path.join(ROOT, "scenes", "veachdoor", "lmc.xml"), force_diffuse=0, max_depth=0, chains=1 << 18),
}
LAYER_MODES = {0: "none", 1: "length", 2: "technique"}


def child(mode, rep, steps, warmup):
    sys.path.insert(0, ROOT)
    p = importlib.import_module("langevin-mcmc_amd")
    host = socket.gethostname()
    for name, w in WORKLOADS.items():
        ren = p.Renderer(w["xml"], force_diffuse=w["force_diffuse"], max_depth=w["max_depth"], seed_offset=0, use_gradient=1)
        ren.set_option("film_exact", 1)
        ren.set_option("film_layers", mode)
        n = w["chains"]
        ren.init_chains(8 * n, n, 65536, max(256, warmup + steps), 0)
        ren.step(warmup)
        ren.sync()
        t0 = time.perf_counter()
        ren.step(steps)
        ren.sync()
        ms = (time.perf_counter() - t0) * 1e3 / steps
        st = ren.stats()
        print(json.dumps(dict(record="step_ms", rep=rep, workload=name, width=ren.width, height=ren.height, chains=n, warmup=warmup, steps=steps, film="exact",
                              layers=LAYER_MODES[mode], n_layers=len(ren.film_layer_info()[1]), ms_per_step=round(ms, 4), chain_steps_per_s=n * steps / (ms * steps * 1e-3),
                              cache_ready_mask=st["cacheReadyMask"], overflow=ren.film_overflow(), host=host)), flush=True)
        ren.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_film_layers_sweep.jsonl"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--child", type=int, default=None)
    ap.add_argument("--rep", type=int, default=0)
    a = ap.parse_args()
    if a.child is not None:
        return child(a.child, a.rep, a.steps, a.warmup)
    lines = []
    for rep in range(a.reps):
        for mode in (0, 1, 2):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(mode), "--rep", str(rep), "--steps", str(a.steps), "--warmup", str(a.warmup)],
                               stdout=subprocess.PIPE, text=True, timeout=600)
            sys.stdout.write(r.stdout)
            sys.stdout.flush()
            if r.returncode != 0:  # nothing more is started on the device after a child that failed
                raise SystemExit("the pass of mode %d in repetition %d ended with status %d" % (mode, rep, r.returncode))
            lines += [l for l in r.stdout.splitlines() if l.startswith("{")]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
