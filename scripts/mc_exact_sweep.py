#!/usr/bin/env python3
"""Records of the exact mc film (lmc_set_option "mc_film_exact", device/mc.hip) beside the float film, and of the bounded launches: ms per
lmc_mc_render call (the call alone: launches + the wait, no read-back), every repetition kept so that the run-to-run spread shows.
  render_64     full-size torus and veach-door at 64 spp (one launch), both generators, float and exact film
  render_256    the same films at 256 spp, bidirectional: the default "mc_launch_streams" (4 launches) against one launch of everything
  launch_at_cap one launch of the default cap's size (the first chunk of the 256 spp render)
One JSON line per measurement.
usage: python scripts/mc_exact_sweep.py [--out profiles/r10_mc_exact_sweep.jsonl] [--reps 3] [--parent]
(--parent: the library selected with LMC_LIB is built from a tree without the exact film and the launch cap: float film, its single launch only)"""
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
ONE_LAUNCH = 1 << 38


def render_ms(ren, spp, reps, streams=(0, -1)):
    """ms of `reps` + 1 lmc_mc_render calls without the first (it pays module load and allocation)"""
    out = []
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        if p.lib().lmc_mc_render(ren.h, spp, streams[0], streams[1]) != 0:
            raise RuntimeError(p.lib().lmc_last_error().decode())
        out.append((time.perf_counter() - t0) * 1e3)
    return out[1:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_mc_exact_sweep.jsonl"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--parent", action="store_true")
    a = ap.parse_args()
    host, lib = socket.gethostname(), "parent" if a.parent else "this"
    rows = []

    def row(record, scene, ren, spp, bidir, exact, ms, **kw):
        paths, splats = ren.mc_stats()
        r = dict(record=record, lib=lib, scene=scene, width=ren.width, height=ren.height, spp=spp, bidirectional=bidir, film="exact" if exact else "float", ms=[round(v, 3) for v in ms],
                 ms_min=round(min(ms), 3), samples=paths, contributions=splats, samples_per_s=paths / (min(ms) * 1e-3), host=host)
        if not a.parent:
            r.update(launches=int(ren.get_option("mc_launches")), launch_streams=int(ren.get_option("mc_launch_streams")), overflow=ren.mc_overflow())
        r.update(kw)
        rows.append(r)
        print(json.dumps(r), flush=True)

    for name, xml in SCENES.items():
        ren = p.Renderer(xml, seed_offset=0, use_gradient=0)
        n_tiles = ((ren.width + 15) // 16) * ((ren.height + 15) // 16)
        for bidir in (1, 0):
            ren.set_option("bidirectional", bidir)
            for exact in ((0,) if a.parent else (0, 1)):
                if not a.parent:
                    ren.set_option("mc_film_exact", exact)
                row("render_64", name, ren, 64, bidir, exact, render_ms(ren, 64, a.reps))
        ren.set_option("bidirectional", 1)
        for exact in ((0,) if a.parent else (0, 1)):
            if a.parent:
                row("render_256", name, ren, 256, 1, 0, render_ms(ren, 256, a.reps))
                continue
            ren.set_option("mc_film_exact", exact)
            default_cap = int(ren.get_option("mc_launch_streams"))
            row("render_256", name, ren, 256, 1, exact, render_ms(ren, 256, a.reps))
            cap_chunk = p.mc_chunks_probe(0, 256 * n_tiles, n_tiles, default_cap)[0]
            row("launch_at_cap", name, ren, 256, 1, exact, render_ms(ren, 256, a.reps, streams=cap_chunk), streams=list(cap_chunk))
            ren.set_option("mc_launch_streams", ONE_LAUNCH)
            row("render_256", name, ren, 256, 1, exact, render_ms(ren, 256, a.reps))
            ren.set_option("mc_launch_streams", default_cap)
        ren.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
