#!/usr/bin/env python3
"""Records of the layered mc film (lmc_set_option "mc_layers", device/mc.hip) beside the unlayered float and exact films, and of the unlayered films
beside the parent commit's: ms per lmc_mc_render call (the call alone: launches + the wait, no read-back) of full-size torus and veach-door at 64 spp,
both generators.  The method of scripts/mc_exact_sweep.py, with the two libraries ALTERNATED in one session: every repetition is one child process per
library (parent first), each of which renders every configuration twice and records the second call (the first pays module load and allocation).
One JSON line per measurement, every repetition kept so that the run-to-run spread shows.
usage: python scripts/mc_layers_sweep.py --parent-lib <liblmc_hip.so built from the parent commit> [--out profiles/r13_mc_layers_sweep.jsonl] [--reps 3]
(--child this|parent is the per-library pass the driver starts; the parent's library has no "mc_layers" and is asked for its unlayered films only)"""
import argparse
import importlib
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = {"torus": os.path.join(ROOT, "scenes", "torus", "lmc.xml"), "veachdoor": os.path.join(ROOT, "scenes", "veachdoor", "lmc.xml")}
SPP = 64
LAYER_MODES = {0: "none", 1: "length", 2: "technique"}


def child(which, rep):
    sys.path.insert(0, ROOT)
    p = importlib.import_module("langevin-mcmc_amd")
    host = socket.gethostname()
    for name, xml in SCENES.items():
        ren = p.Renderer(xml, seed_offset=0, use_gradient=0)
        for bidir in (1, 0):
            ren.set_option("bidirectional", bidir)
            for exact in (0, 1):
                ren.set_option("mc_film_exact", exact)
                for layers in ((0,) if which == "parent" else (0, 1, 2)):
                    if which != "parent":
                        ren.set_option("mc_layers", layers)
                    ms = []
                    for _ in range(2):
                        t0 = time.perf_counter()
                        if p.lib().lmc_mc_render(ren.h, SPP, 0, -1) != 0:
                            raise RuntimeError(p.lib().lmc_last_error().decode())
                        ms.append((time.perf_counter() - t0) * 1e3)
                    paths, splats = ren.mc_stats()
                    print(json.dumps(dict(record="render_64", lib=which, rep=rep, scene=name, width=ren.width, height=ren.height, spp=SPP, bidirectional=bidir,
                                          film="exact" if exact else "float", layers=LAYER_MODES[layers], n_layers=len(ren.mc_layer_info()[1]) if which != "parent" else 0,
                                          ms=round(ms[1], 3), ms_first=round(ms[0], 3), samples=paths, contributions=splats, samples_per_s=paths / (ms[1] * 1e-3), host=host)),
                          flush=True)
        ren.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13_mc_layers_sweep.jsonl"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--parent-lib")
    ap.add_argument("--child")
    ap.add_argument("--rep", type=int, default=0)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.rep)
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        raise SystemExit("--parent-lib: the parent commit's liblmc_hip.so expected")
    lines = []
    for rep in range(a.reps):
        for which in ("parent", "this"):
            env = dict(os.environ)
            if which == "parent":
                env["LMC_LIB"] = os.path.abspath(a.parent_lib)
            else:
                env.pop("LMC_LIB", None)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", which, "--rep", str(rep)], env=env, stdout=subprocess.PIPE, text=True, timeout=900)
            sys.stdout.write(r.stdout)
            sys.stdout.flush()
            if r.returncode != 0:  # nothing more is started on the device after a child that failed
                raise SystemExit("the %s pass of repetition %d ended with status %d" % (which, rep, r.returncode))
            lines += [l for l in r.stdout.splitlines() if l.startswith("{")]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
