#!/usr/bin/env python3
"""Records of the "mc" integrator (lmc_mc_render, device/mc.hip): ms per render and samples/s, bidirectional and unidirectional, on the shipped
torus and veach-door films at 1 and 64 spp, next to the estimators that share its generators -- lmc_bidir_mc (GeneratePathBidir at random screen
positions, path length >= 3) and lmc_path_trace (GeneratePath, one thread per 16x16 tile above maxdepth 2).  One JSON line per measurement.
usage: python scripts/mc_sweep.py [--out profiles/r07_mc_sweep.jsonl] [--quick] [--mc-only]
(--quick: one torus render, for a profiler run; --mc-only: without the two other estimators, for A/B builds selected with LMC_LIB)"""
import argparse
import importlib
import json
import os
import socket
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
p = importlib.import_module("langevin-mcmc_amd")

SCENES = {"torus": os.path.join(ROOT, "scenes", "torus", "lmc.xml"), "veachdoor": os.path.join(ROOT, "scenes", "veachdoor", "lmc.xml")}


def timed(fn, reps=2):
    """last of `reps` calls (the first one pays module load / allocation)"""
    dt = 0.0
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        dt = time.perf_counter() - t0
    return dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_mc_sweep.jsonl"))
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--mc-only", action="store_true")
    a = ap.parse_args()
    rows = []
    host = socket.gethostname()
    for name, xml in SCENES.items():
        if a.quick and name != "torus":
            continue
        ren = p.Renderer(xml, seed_offset=0, use_gradient=0)
        W, H = ren.width, ren.height
        for spp in ((1,) if a.quick else (1, 64)):
            n = W * H * spp
            for bidir in ((1,) if a.quick else (1, 0)):
                ren.set_option("bidirectional", bidir)
                dt = timed(lambda: ren.mc_render(spp), 1 if a.quick else 2)
                paths, splats = ren.mc_stats()
                rows.append(dict(record="mc_render", scene=name, width=W, height=H, spp=spp, bidirectional=bidir, ms=dt * 1e3, samples=paths,
                                 contributions=splats, samples_per_s=paths / dt, host=host))
            if a.quick or a.mc_only:
                continue
            dt = timed(lambda: ren.bidir_mc(spp))
            per = (n + 65535) // 65536
            rows.append(dict(record="lmc_bidir_mc", scene=name, width=W, height=H, spp=spp, ms=dt * 1e3, samples=per * 65536,
                             samples_per_s=per * 65536 / dt, note="65536 threads, random screen positions, path length >= 3", host=host))
            dt = timed(lambda: ren.path_trace(spp))
            rows.append(dict(record="lmc_path_trace", scene=name, width=W, height=H, spp=spp, ms=dt * 1e3, samples=n, samples_per_s=n / dt,
                             note="one thread per 16x16 tile (k_direct) at maxdepth > 2", host=host))
        ren.close()
    for r in rows:
        print(json.dumps(r))
    if not a.quick:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
