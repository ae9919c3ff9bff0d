#!/usr/bin/env python3
"""The layered MLT film beside the layered mc film: each technique layer's share of the total luminance, over the layers BOTH renders
populate, on the torus at 64 x 48, force_diffuse, maxdepth 6.  MLT side: film_layers = 2, 16384 chains x 64 steps, the mean and the standard error of the
share over 8 seed offsets (2^20 apart: a chain's stream is seeded with its id plus the offset).  Reference: one bidirectional 64 spp layered mc render (mc_layers = 2, exact), itself pinned to the CPU oracle by
tests/test_gpu_mc_layers.py.  One JSON line per layer, then one summary line; a layer further than four standard errors from the mc share is marked.
Nothing is tuned to close a gap.
usage: python scripts/film_layers_vs_mc.py [--out profiles/r14_film_layers_vs_mc.jsonl]"""
import argparse
import importlib
import json
import os
import socket
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TORUS = os.path.join(ROOT, "scenes", "torus", "lmc.xml")
W, H, D, SEEDS, CHAINS, STEPS, SPP = 64, 48, 6, 8, 16384, 64, 64
SEED_STRIDE = 1 << 20  # between two seed offsets: more than the chains and the init streams of a run


def lum(img):
    return 0.212671 * img[..., 0] + 0.715160 * img[..., 1] + 0.072169 * img[..., 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_film_layers_vs_mc.jsonl"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    p = importlib.import_module("langevin-mcmc_amd")
    ref = p.Renderer(TORUS, force_diffuse=1, max_depth=D, width=W, height=H, seed_offset=0, use_gradient=0)
    ref.set_option("mc_film_exact", 1)
    ref.set_option("mc_layers", 2)
    ref.set_option("bidirectional", 1)
    ref.mc_render(SPP)
    table = ref.mc_layer_info()[1]
    mc = np.array([lum(np.float64(l)).sum() for l in ref.mc_layers_fixed()])  # a share is a ratio: the unit (2^-32, spp) cancels
    ref.close()
    mlt = np.zeros((SEEDS, len(table)))
    for s in range(SEEDS):
        # chain i seeds its stream with i + seed offset: offsets closer than the number of chains would run nearly the same population again
        ren = p.Renderer(TORUS, force_diffuse=1, max_depth=D, width=W, height=H, seed_offset=s * SEED_STRIDE, use_gradient=1)
        ren.set_option("film_exact", 1)
        ren.set_option("film_layers", 2)
        ren.init_chains(8 * CHAINS, CHAINS, 4096, STEPS, 0)
        ren.step(STEPS)
        assert ren.film_layer_info()[1] == table and ren.film_overflow() == 0
        mlt[s] = [lum(np.float64(l)).sum() for l in ren.film_layers_fixed()]
        ren.close()
    both = (mc > 0) & (mlt > 0).all(axis=0)
    mc_share = mc[both] / mc[both].sum()
    shares = mlt[:, both] / mlt[:, both].sum(axis=1, keepdims=True)
    mean, se = shares.mean(axis=0), shares.std(axis=0, ddof=1) / np.sqrt(SEEDS)
    host, lines, far = socket.gethostname(), [], []
    for (c, l), m, e, r in zip([t for t, b in zip(table, both) if b], mean, se, mc_share):
        z = (m - r) / e if e > 0 else float("inf")
        if abs(z) > 4:
            far.append([c, l])
        lines.append(json.dumps(dict(record="layer_share", camDepth=c, lightDepth=l, length=c + l - 1, mlt_share=float(m), mlt_se=float(e), mc_share=float(r), z=float(z),
                                     beyond_4_se=bool(abs(z) > 4))))
    only_mc = [list(t) for t, x, b in zip(table, mc, both) if x > 0 and not b]
    only_mlt = [list(t) for t, x, b in zip(table, (mlt > 0).any(axis=0), both) if x and not b]
    lines.append(json.dumps(dict(record="summary", width=W, height=H, maxdepth=D, seeds=SEEDS, chains=CHAINS, steps=STEPS, mc_spp=SPP, seed_stride=SEED_STRIDE, layers_compared=int(both.sum()),
                                 populated_by_mc_only=only_mc, populated_by_mlt_only_or_not_every_seed=only_mlt, beyond_4_se=far, host=host)))
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
