#!/usr/bin/env python3
"""Live-VGPR map of one kernel from `hipcc -S -gline-tables-only` output.

usage: scripts/live_vgpr_map.py FILE.s KERNEL_SUBSTRING [--top N]

Builds the kernel's control-flow graph from its labels and branches, runs a backward liveness pass over the vector registers, and
reports, per source file and (for dsmall.h) per PR_* region of SmallStepLean, the high-water mark of simultaneously live VGPRs, the
source line it falls on, and where the registers alive at that point were last written (by source line: the names of the values are
the reader's to look up).  A source line is the INNERMOST inlined location of an instruction (.loc), so the walk's lines are dscene.h's.

Approximations: a write under a partial EXEC mask counts as a full definition (a value kept for the inactive lanes through a branch-free
`if` is under-counted); calls (s_swappc) are fall-throughs that read nothing.  The allocator's own figure (kernel-resource-usage) is the
authority for the total; this map says WHERE the pressure is and what holds it.
"""
import os
import re
import sys
from collections import defaultdict

DSMALL = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "langevin-mcmc_amd", "csrc", "device", "dsmall.h")  # the PR_* marks

STORE = re.compile(r"^(global|flat|scratch|buffer)_store|^ds_(write|store)|^ds_(add|min|max|and|or|xor|inc|dec)_(u32|i32|f32|u64)$|^exp")
NO_VDST = re.compile(r"^v_cmp|^v_readlane|^v_readfirstlane|^s_|^v_nop|^buffer_wbl2|^buffer_inv|^ds_bpermute_never")
DST_ALSO_READ = re.compile(r"^v_fmac|^v_mac|^v_writelane|^v_swap|^v_dot.*acc|^v_pk_fmac|^v_mfma|^v_movrel")
REG = re.compile(r"\bv(\d+)\b|\bv\[(\d+):(\d+)\]")


def regs_of(tok):
    out = []
    for m in REG.finditer(tok):
        if m.group(1) is not None:
            out.append(int(m.group(1)))
        else:
            out.extend(range(int(m.group(2)), int(m.group(3)) + 1))
    return out


def parse(path, want):
    files, ins, labels = {}, [], {}
    cur_loc, cur_chain, inside = ("?", 0), [], False
    for raw in open(path, errors="replace"):
        line = raw.split(";")[0].strip()
        if not line:
            continue
        m = re.match(r"\.file\s+(\d+)\s+(?:\"([^\"]*)\"\s+)?\"([^\"]*)\"", line)
        if m:
            files[int(m.group(1))] = m.group(3).split("/")[-1]
            continue
        if line.endswith(":") and not line.startswith("."):
            if inside:
                break
            inside = want in line
            continue
        if not inside:
            continue
        if line.startswith(".Lfunc_end"):
            break
        m = re.match(r"\.loc\s+(\d+)\s+(\d+)", line)
        if m:
            cur_loc = (files.get(int(m.group(1)), m.group(1)), int(m.group(2)))
            # the inlining chain hipcc prints behind the directive: "; a.h:12:3 @[ b.h:40:9 @[ kernel.hip:63:13 ] ]", innermost first
            cur_chain = [(f.split("/")[-1], int(l)) for f, l in re.findall(r"([\w./+-]+):(\d+):\d+", raw.split(";", 1)[1])] if ";" in raw else []
            continue
        if line.endswith(":"):
            labels[line[:-1]] = len(ins)
            continue
        if line.startswith("."):
            continue
        parts = line.split(None, 1)
        mn = parts[0]
        ops = [o.strip() for o in parts[1].split(",")] if len(parts) > 1 else []
        defs, uses = [], []
        atomic_noret = "_atomic_" in mn and "sc0" not in line and "glc" not in line
        if STORE.search(mn) or NO_VDST.search(mn) or atomic_noret:
            for o in ops:
                uses += regs_of(o)
        else:
            if ops:
                defs = regs_of(ops[0])
                if DST_ALSO_READ.search(mn):
                    uses += defs
            for o in ops[1:]:
                uses += regs_of(o)
        target = ops[0] if mn.startswith("s_cbranch") or mn == "s_branch" else None
        ins.append({"mn": mn, "defs": defs, "uses": uses, "loc": cur_loc, "chain": cur_chain, "target": target, "text": line})
    return ins, labels


def liveness(ins, labels):
    n = len(ins)
    succ = [[] for _ in range(n)]
    for k, i in enumerate(ins):
        if i["mn"] in ("s_endpgm", "s_setpc_b64"):
            continue
        if i["mn"] == "s_branch":
            succ[k] = [labels[i["target"]]] if i["target"] in labels else []
            continue
        if k + 1 < n:
            succ[k].append(k + 1)
        if i["target"] in labels:
            succ[k].append(labels[i["target"]])
    dmask = [sum(1 << r for r in set(i["defs"])) for i in ins]
    umask = [sum(1 << r for r in set(i["uses"])) for i in ins]
    live_in = [0] * n
    live_out = [0] * n
    changed = True
    while changed:
        changed = False
        for k in range(n - 1, -1, -1):
            o = 0
            for s in succ[k]:
                if s < n:
                    o |= live_in[s]
            i_ = umask[k] | (o & ~dmask[k])
            if o != live_out[k] or i_ != live_in[k]:
                live_out[k], live_in[k] = o, i_
                changed = True
    return live_in, live_out, dmask


def regions_of_dsmall(path):
    """[(first line, last line, name)] of SmallStepLean: a region ends at the prof.Mark that names it"""
    marks = []
    for n, l in enumerate(open(path), 1):
        m = re.search(r"prof\.Mark\((PR_\w+)\)", l)
        if m and "LMC_PROF_FINE" not in l:
            marks.append((n, m.group(1)))
    return marks


def main():
    path, want = sys.argv[1], sys.argv[2]
    top = int(sys.argv[sys.argv.index("--top") + 1]) if "--top" in sys.argv else 14
    ins, labels = parse(path, want)
    live_in, live_out, dmask = liveness(ins, labels)
    press = [bin(live_out[k] | dmask[k] | live_in[k]).count("1") for k in range(len(ins))]
    # last writer (linear order) of every register, for naming what is alive at a peak
    last_def, writers = {}, []
    for k, i in enumerate(ins):
        for r in i["defs"]:
            last_def[r] = i["loc"]
        writers.append(dict(last_def))
    print(f"kernel {want}: {len(ins)} instructions, peak {max(press)} live VGPRs (highest register named: v{max(max(i['defs'] + i['uses'], default=0) for i in ins)})")

    def describe(k):
        alive = live_out[k] | live_in[k]
        by = defaultdict(int)
        for r in range(alive.bit_length()):
            if alive >> r & 1:
                f, l = writers[k].get(r, ("entry", 0))
                by[f"{f}:{l}"] += 1
        return ", ".join(f"{n}x {loc}" for loc, n in sorted(by.items(), key=lambda x: -x[1]))

    if "--dump-peak" in sys.argv:  # every register alive at the kernel's peak with the instruction that last wrote it
        k = max(range(len(ins)), key=lambda j: press[j])
        last = {}
        for j in range(k + 1):
            for r in ins[j]["defs"]:
                last[r] = j
        alive = live_out[k] | live_in[k]
        print(f"\n== alive at the peak (instruction {k}: {ins[k]['text']}, {ins[k]['loc'][0]}:{ins[k]['loc'][1]})")
        for r in range(alive.bit_length()):
            if alive >> r & 1:
                j = last.get(r)
                print(f"v{r:<4d} " + (f"[{j:6d}] {ins[j]['loc'][0]}:{ins[j]['loc'][1]:<5d} {ins[j]['text']}" if j is not None else "kernel entry"))

    by_file = defaultdict(lambda: (0, -1))
    for k, i in enumerate(ins):
        f = i["loc"][0]
        if press[k] > by_file[f][0]:
            by_file[f] = (press[k], k)
    print("\n== high-water mark by source file (innermost inlined location)")
    for f, (p, k) in sorted(by_file.items(), key=lambda x: -x[1][0])[:top]:
        print(f"{p:4d}  {f}:{ins[k]['loc'][1]}   {ins[k]['text']}")
    marks = None
    try:
        marks = regions_of_dsmall(DSMALL)
    except OSError:
        pass
    if marks:
        print("\n== SmallStepLean regions: an instruction belongs to the region of the dsmall.h line of SmallStepLean it was inlined from (the outermost such"
              "\n   line of its .loc chain; a region ends at the prof.Mark that names it); `kernel` = the code around the step (step_small_plain.hip)")
        body = next(n for n, l in enumerate(open(DSMALL), 1) if "LMC_D void SmallStepLean(" in l)
        reg_max = defaultdict(lambda: (0, -1))
        for k, i in enumerate(ins):
            lines = [l for f, l in i["chain"] if f == "dsmall.h" and l >= body]
            if lines:
                nxt = [name for (m, name) in marks if m >= lines[-1]]
                cur = nxt[0] if nxt else "after " + marks[-1][1]
            else:
                cur = "kernel"
            if press[k] > reg_max[cur][0]:
                reg_max[cur] = (press[k], k)
        for name, (p, k) in sorted(reg_max.items(), key=lambda x: -x[1][0]):
            print(f"\n{p:4d}  {name:16s} at {ins[k]['loc'][0]}:{ins[k]['loc'][1]}   {ins[k]['text']}")
            print(f"      alive, by the line that last wrote them: {describe(k)}")


if __name__ == "__main__":
    main()
