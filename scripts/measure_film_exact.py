#!/usr/bin/env python3
"""What the exact film (film_exact, INTEGRATION.md "Exact film") costs, and that the default mode costs nothing: one JSON line per measurement.

    python scripts/measure_film_exact.py --parent-lib <liblmc_hip.so built from the parent commit> [--runs 3] [--skip-default-run] >> profiles/r09_film_exact.jsonl

  ab       bench.py (the two commands: --steps 20 --warmup 5, and the default run) with the parent's library and this tree's, ALTERNATELY on one box,
           --runs each: this tree's median must lie inside the parent's own min-max
  exact    the same commands with LMC_FILM_EXACT=1 (bench.py records every LMC_* variable), next to the float numbers
  lean     the lean small-step kernel alone (lmc_kernel_timing), float against exact, 2^20 chains on the torus; refused unless a cache dim is ready, and
           the record carries the ready mask and the chain-steps the lean kernel ran in the timed interval
  merge    lmc_group_film_reduce of two contexts on one device and lmc_film_read at 1024 x 768, float against exact
Every bench.py run is a child process with a time limit; the first that fails ends the script."""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def bench(args, env_extra, limit):
    env = dict(os.environ, **env_extra)
    t0 = time.time()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + args, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=limit, cwd=ROOT)
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-4000:])
        raise SystemExit("bench.py failed (%d): %s %s" % (r.returncode, args, env_extra))
    line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    j = json.loads(line)
    return dict(value=j["value"], unit=j.get("unit"), ms_per_step=j.get("ms_per_step"), kernel_ms_per_step=j.get("kernel_ms_per_step"), lmc_env=j.get("lmc_env"), wall_s=round(time.time() - t0, 1))


def emit(**kw):
    print(json.dumps(kw), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--skip-default-run", action="store_true")
    ap.add_argument("--skip-ab", action="store_true")
    ap.add_argument("--limit", type=int, default=240, help="seconds per bench.py run")
    a = ap.parse_args()
    commands = [("steps20_warmup5", ["--steps", "20", "--warmup", "5"])] + ([] if a.skip_default_run else [("default", [])])
    if not a.skip_ab:
        for name, args in commands:
            runs = {"parent": [], "tree": [], "tree_exact": []}
            for k in range(a.runs):  # alternately, so that a drift of the box lands on both
                runs["parent"].append(bench(args, {"LMC_LIB": os.path.abspath(a.parent_lib)}, a.limit))
                runs["tree"].append(bench(args, {}, a.limit))
                runs["tree_exact"].append(bench(args, {"LMC_FILM_EXACT": "1"}, a.limit))
            pv, tv, ev = ([r["value"] for r in runs[k]] for k in ("parent", "tree", "tree_exact"))
            emit(measurement="ab", command="bench.py --gpus 1 " + " ".join(args), unit=runs["tree"][0]["unit"], parent=pv, tree=tv, tree_exact=ev, parent_min=min(pv), parent_max=max(pv),
                 tree_median=statistics.median(tv), tree_median_inside_parent_spread=min(pv) <= statistics.median(tv) <= max(pv), tree_over_parent_median=statistics.median(tv) / statistics.median(pv),
                 exact_over_float_median=statistics.median(ev) / statistics.median(tv), exact_lmc_env=runs["tree_exact"][0]["lmc_env"],
                 kernel_ms_per_step=dict(parent=runs["parent"][-1]["kernel_ms_per_step"], tree=runs["tree"][-1]["kernel_ms_per_step"], tree_exact=runs["tree_exact"][-1]["kernel_ms_per_step"]),
                 wall_s=[r["wall_s"] for k in runs for r in runs[k]])
    # ---- in this process: the lean kernel alone, the merge and the read-back
    p = importlib.import_module("langevin-mcmc_amd")
    torus = os.path.join(ROOT, "scenes", "torus", "lmc.xml")
    n = 1 << 20
    lean = {}
    for exact in (0, 1, 0, 1):
        ren = p.Renderer(torus, force_diffuse=1, max_depth=6, width=1024, height=768, seed_offset=0, use_gradient=1)
        ren.set_option("film_exact", exact)
        ren.init_chains(8 * n, n, 65536, 10 ** 6)
        ren.step(40)  # the caches fill
        ren.sync()
        mask = ren.stats()["cacheReadyMask"]
        if not mask:  # no cache is ready: the timed steps would be cache-filling gradient steps, not the lean kernel
            raise SystemExit("lean-kernel timing: no cache dim is ready after the fill steps")
        ren.set_option("timing", 1)
        lean0 = ren.kernel_timing()[2]
        ren.step(20)
        ren.sync()
        ren.step_timing()
        ms, _, lean1 = ren.kernel_timing()
        t0 = time.perf_counter()
        for _ in range(5):
            ren.film()
        read_ms = (time.perf_counter() - t0) / 5 * 1e3
        lean.setdefault("exact" if exact else "float", []).append(dict(lean_ms_per_step=ms / 20, lean_chain_steps_timed=lean1 - lean0, cache_ready_mask=mask, film_read_ms=read_ms, overflow=ren.film_overflow()))
        ren.close()
    emit(measurement="lean_kernel_and_film_read", chains=n, film=[1024, 768], steps_timed=20, **lean)
    merge = {}
    for exact in (0, 1):
        rens = [p.Renderer(torus, force_diffuse=1, max_depth=6, width=1024, height=768, seed_offset=0, use_gradient=1) for _ in range(2)]
        for r in rens:
            r.set_option("film_exact", exact)
        g = p.Group(rens)
        g.init_chains(8 * 65536, 65536, 4096, 10 ** 6)
        ms = []
        for _ in range(5):
            g.step(1)
            ms.append(g.film_reduce())
        merge["exact" if exact else "float"] = dict(group_film_reduce_ms=ms, members=2, devices=g.info()["devices"])
        for r in rens:
            r.close()
    emit(measurement="group_merge", film=[1024, 768], note="two contexts on one device unless more are visible: copies within the device, not over the links", **merge)


if __name__ == "__main__":
    main()
