#!/usr/bin/env python3
"""Cost of a checkpoint: file bytes per chain, save ms and load ms (split into device pack / unpack, copies and file I/O by the library's
LMC_CKPT_LOG line) and the lmc_chains_init a load replaces, per workload and chain count.  One JSON line per measurement:

    python scripts/measure_checkpoint.py --out profiles/<name>_checkpoint.jsonl [--chains 65536 1048576] [--scenes torus door] [--dir /tmp]

Every (scene, chains) pair runs in a child process of its own (a fresh runtime; the library's log line goes to the child's stderr).  The file goes
to --dir: what "file I/O" means depends on that file system (page cache included), so the line records it."""
import argparse
import importlib
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = {"torus": ("scenes/torus/lmc.xml", dict(force_diffuse=1, max_depth=6)), "door": ("scenes/veachdoor/lmc.xml", dict(force_diffuse=0, max_depth=0))}


def child(scene, chains, steps, d):
    sys.path.insert(0, ROOT)
    p = importlib.import_module("langevin-mcmc_amd")
    xml, kw = SCENES[scene]
    path = os.path.join(d, "measure_%s_%d.ckpt" % (scene, chains))

    def make():
        return p.Renderer(os.path.join(ROOT, xml), seed_offset=0, use_gradient=1, **kw)

    ren = make()
    t = time.perf_counter()
    ren.init_chains(8 * chains, chains, 65536, 256)
    ren.sync()
    init_ms = (time.perf_counter() - t) * 1e3
    ren.step(steps)
    ren.sync()
    saves = []
    for _ in range(3):  # the first save pays the scene hash and the first launch of the pack kernel
        t = time.perf_counter()
        ren.save_checkpoint(path)
        saves.append((time.perf_counter() - t) * 1e3)
    ren.close()
    ren = make()
    t = time.perf_counter()
    ren.load_checkpoint(path)
    load_ms = (time.perf_counter() - t) * 1e3
    ren.step(1)
    ren.sync()
    ren.close()
    info = p.checkpoint_info(path)
    size = os.path.getsize(path)
    os.remove(path)
    print(json.dumps(dict(scene=scene, chains=chains, steps_before_save=steps, file_bytes=size, bytes_per_chain=size / chains, record_bytes=info["record_bytes"],
                          job_bytes=info["job_bytes"], init_ms=init_ms, save_ms=saves, load_ms=load_ms, dir=d)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--chains", type=int, nargs="+", default=[1 << 16, 1 << 20])
    ap.add_argument("--scenes", nargs="+", default=["torus", "door"])
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--dir", default="/tmp")
    ap.add_argument("--child", nargs=2)
    a = ap.parse_args()
    if a.child:
        return child(a.child[0], int(a.child[1]), a.steps, a.dir)
    lines = []
    for scene in a.scenes:
        for n in a.chains:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", scene, str(n), "--steps", str(a.steps), "--dir", a.dir],
                               env=dict(os.environ, LMC_CKPT_LOG="1"), capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                sys.stderr.write(r.stderr[-2000:])
                return 1
            rec = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
            rec["library_log"] = [l for l in r.stderr.splitlines() if l.startswith("[lmc] checkpoint")]
            m = re.search(r"pack ([0-9.]+) ms, copies ([0-9.]+) ms, file ([0-9.]+) ms", rec["library_log"][-2] if len(rec["library_log"]) >= 2 else "")
            if m:  # the last save
                rec["save_split_ms"] = dict(pack=float(m.group(1)), copies=float(m.group(2)), file=float(m.group(3)))
            m = re.search(r"file ([0-9.]+) ms, copies ([0-9.]+) ms, unpack ([0-9.]+) ms", rec["library_log"][-1] if rec["library_log"] else "")
            if m:
                rec["load_split_ms"] = dict(file=float(m.group(1)), copies=float(m.group(2)), unpack=float(m.group(3)))
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
