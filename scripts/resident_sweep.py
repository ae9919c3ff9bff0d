#!/usr/bin/env python3
"""Lock step against the resident schedule (lmc_set_option "resident_steps", device/step_resident.h) over the number of chains.

For every workload and N: fresh chains, lock steps until every relevant cache dim is ready (plain MLT: at once), a warm-up, then in the steady
state
  * lock step:  ms / step and chain-steps/s over --steps steps (wall time from a synchronised start to a synchronised end)
  * resident:   chain-steps/s for every K of --ks and every lanes-per-wave choice of --lanes, over the multiple of K nearest --resident-steps
                (after one untimed launch of that configuration), with the K in force after the cap and the HIP-event time of the launches
Then one `dpt_amd --chains 65536` render of a reduced torus scene, with and without --resident.

One JSON line per measurement into profiles/<name>.jsonl.  Every (workload, N) runs in a child process of its own under a time limit; the sweep
stops at the first child that fails.

usage: python scripts/resident_sweep.py --name r07_resident_sweep [--log2n 12,14,16,18,20] [--ks 8,32,128] [--lanes 64,32,16]
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TORUS = os.path.join(ROOT, "scenes", "torus", "lmc.xml")
DOOR = os.path.join(ROOT, "scenes", "veachdoor", "lmc.xml")
CLI = os.path.join(ROOT, "langevin-mcmc_amd", "dpt_amd")
WORKLOADS = {  # name: (scene, force_diffuse, max_depth, mala)
    "torus_lmc": (TORUS, 1, 6, True),  # BASELINE.json configs[1]: Lambertian, max path length 6 (the headline workload)
    "door_lmc": (DOOR, 0, 0, True),  # veach-door as shipped (maxdepth 8, glossy)
    "torus_mlt": (TORUS, 1, 6, False),  # plain MLT: no gradient cache, resident from the first step
}


def measure_one(wl, n, ks, lanes, steps, resident_steps, max_fill):
    import importlib

    import numpy as np  # noqa: F401  (the package needs it)

    p = importlib.import_module("langevin-mcmc_amd")
    scene, fd, md, mala = WORKLOADS[wl]
    ren = p.Renderer(scene, force_diffuse=fd, max_depth=md, seed_offset=0, use_gradient=1)
    if not mala:
        ren.set_option("mala", 0)
    maxd = int(ren.get_option("maxdepth"))
    relevant = sum(1 << d for d in range(2 * max(int(ren.get_option("mindepth")), 3), min(2 * maxd, 12) + 1, 2)) if mala else 0
    t0 = time.time()
    ren.init_chains(max(200000, 8 * n), n, 65536, 10 ** 6)
    init_s = time.time() - t0
    fill = 0
    while (ren.stats()["cacheReadyMask"] & relevant) != relevant and fill < max_fill:
        ren.step(16)
        fill += 16
    ready = (ren.stats()["cacheReadyMask"] & relevant) == relevant
    ren.step(16)  # warm-up in the steady state
    base = dict(workload=wl, n=n, maxdepth=maxd, init_s=round(init_s, 2), fill_steps=fill, caches_ready=ready)
    out = []

    def timed(k):
        ren.sync()
        t = time.perf_counter()
        ren.step(k)
        ren.sync()
        return time.perf_counter() - t

    dt = timed(steps)
    lock = dict(base, schedule="lock", steps=steps, ms_per_step=1e3 * dt / steps, chain_steps_per_s=n * steps / dt)
    out.append(lock)
    if not ready:
        out.append(dict(base, schedule="resident", note="caches not ready after %d fill steps: no resident measurement" % fill))
        return out
    for L in lanes:
        for K in ks:
            ren.set_option("resident_steps", K)
            ren.set_option("resident_lanes", L)
            ren.step(K)  # one untimed launch of this configuration
            s0 = ren.resident_stats()
            total = max(1, round(resident_steps / s0["k"])) * s0["k"]
            dt = timed(total)
            s1 = ren.resident_stats()
            launches = s1["launches"] - s0["launches"]
            kms = s1["kernel_ms"] - s0["kernel_ms"]
            out.append(dict(base, schedule="resident", K=K, k_in_force=s1["k"], lanes=L, steps=total, launches=launches, ms_per_launch=1e3 * dt / max(launches, 1),
                            kernel_ms=kms, ms_per_step=1e3 * dt / total, chain_steps_per_s=n * total / dt, vs_lock=(n * total / dt) / lock["chain_steps_per_s"],
                            guard=s1["guard"]))
            ren.set_option("resident_steps", 0)
    ren.close()
    return out


def reduced_torus(d, width=256, height=192, spp=512):
    xml = open(TORUS).read()
    xml = xml.replace('<integer name="height" value="768"/>', '<integer name="height" value="%d"/>' % height)
    xml = xml.replace('<integer name="width" value="1024"/>', '<integer name="width" value="%d"/>' % width)
    xml = re.sub(r'<integer name="spp"\s+value="245"/>', '<integer name="spp" value="%d"/>' % spp, xml)
    os.symlink(os.path.join(ROOT, "scenes", "torus", "data"), os.path.join(d, "data"))
    p = os.path.join(d, "lmc.xml")
    open(p, "w").write(xml)
    return p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--name", required=True)
    ap.add_argument("--log2n", default="12,14,16,18,20")
    ap.add_argument("--workloads", default=",".join(WORKLOADS))
    ap.add_argument("--ks", default="8,32,128")
    ap.add_argument("--lanes", default="64,32,16")
    ap.add_argument("--steps", type=int, default=32, help="lock steps timed")
    ap.add_argument("--resident-steps", type=int, default=128, help="resident steps timed (rounded to a multiple of K)")
    ap.add_argument("--max-fill", type=int, default=4096)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per child")
    ap.add_argument("--cli-resident", type=int, default=32)
    ap.add_argument("--no-cli", action="store_true")
    ap.add_argument("--one", help=argparse.SUPPRESS)  # child: workload:n
    a = ap.parse_args()
    ks, lanes = [int(x) for x in a.ks.split(",")], [int(x) for x in a.lanes.split(",")]
    if a.one:
        wl, n = a.one.split(":")
        for rec in measure_one(wl, int(n), ks, lanes, a.steps, a.resident_steps, a.max_fill):
            print("REC " + json.dumps(rec), flush=True)
        return 0
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    path = os.path.join(ROOT, "profiles", a.name + ".jsonl")
    with open(path, "w") as f:
        for wl in a.workloads.split(","):
            for e in a.log2n.split(","):
                cmd = [sys.executable, os.path.abspath(__file__), "--name", a.name, "--ks", a.ks, "--lanes", a.lanes, "--steps", str(a.steps),
                       "--resident-steps", str(a.resident_steps), "--max-fill", str(a.max_fill), "--one", "%s:%d" % (wl, 1 << int(e))]
                try:
                    r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=a.timeout)
                except subprocess.TimeoutExpired:
                    print("TIMEOUT: %s 2^%s" % (wl, e), flush=True)
                    return 124
                for line in r.stdout.splitlines():
                    if line.startswith("REC "):
                        f.write(line[4:] + "\n")
                        f.flush()
                        rec = json.loads(line[4:])
                        print(rec["workload"], rec["n"], rec["schedule"], rec.get("K", ""), rec.get("lanes", ""), "%.1f M/s" % (rec.get("chain_steps_per_s", 0) / 1e6),
                              flush=True)
                if r.returncode != 0:
                    print(r.stdout[-4000:], flush=True)
                    print("FAILED (exit %d): %s 2^%s" % (r.returncode, wl, e), flush=True)
                    return r.returncode if r.returncode > 0 else 1
        if not a.no_cli and os.path.exists(CLI):
            for extra in ([], ["--resident", str(a.cli_resident)]):
                with tempfile.TemporaryDirectory() as d:
                    scene = reduced_torus(d)
                    try:
                        r = subprocess.run([CLI, "--seedoffset", "5", "--chains", "65536"] + extra + [scene], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                                           text=True, timeout=a.timeout)
                    except subprocess.TimeoutExpired:
                        print("TIMEOUT: dpt_amd %s" % extra, flush=True)
                        return 124
                    if r.returncode != 0:
                        print(r.stdout[-4000:], "FAILED: dpt_amd", extra, flush=True)
                        return r.returncode if r.returncode > 0 else 1
                    el = float(re.search(r"Elapsed time:([0-9.eE+-]+)", r.stdout).group(1))
                    m = re.search(r"(\d+) mutations, ([0-9.]+) M mutations/s", r.stdout)
                    rec = dict(workload="dpt_amd_reduced_torus", scene="torus lmc.xml at 256x192, spp 512, maxdepth 8 (as shipped)", n=65536,
                               schedule="resident" if extra else "lock", K=a.cli_resident if extra else 0, elapsed_s=el, mutations=int(m.group(1)),
                               m_mutations_per_s=float(m.group(2)))
                    f.write(json.dumps(rec) + "\n")
                    f.flush()
                    print(rec, flush=True)
    print("wrote", path)
    return 0


if __name__ == "__main__":
    sys.exit(main())
