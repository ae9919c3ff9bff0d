#!/usr/bin/env python3
"""Per-kernel register / scratch / occupancy tables of two builds, side by side, from hipcc's -Rpass-analysis=kernel-resource-usage remarks.

    make -O -f langevin-mcmc_amd/csrc/Makefile EXTRA=-Rpass-analysis=kernel-resource-usage 2> build.log     (in each of the two trees)
    python scripts/kernel_resources_diff.py parent.log tree.log [--only=k_step_small,k_step,...] > profiles/<name>.txt

(-O keeps the remarks of one translation unit together when make runs jobs in parallel; a block whose fields are out of order is an error.)
A kernel that takes the film's type as its first template argument (dchain.h) is paired with the kernel of the same name and remaining arguments
in the other log: k_step<lmcd::Film, ...> with k_step<...>, k_h2_finish<lmcd::Film> with k_h2_finish; the FilmFixed forms have no partner.
Exit status 1 when a kernel of the second log uses more VGPRs or scratch, or has a lower occupancy, than the same kernel of the first."""
import re
import subprocess
import sys

FIELDS = ["TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Dynamic Stack", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill", "LDS Size [bytes/block]"]
SHOWN = ["VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "TotalSGPRs", "SGPRs Spill", "VGPRs Spill", "LDS Size [bytes/block]"]


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), stdout=subprocess.PIPE, text=True, check=True).stdout.split("\n")
        return dict(zip(names, out))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def parse(path):
    kernels, cur, want = {}, None, 0
    for line in open(path, errors="replace"):
        m = re.search(r"remark: (?:Function Name: (\S+)|\s*([A-Za-z][^:]*): (\S+))\s*\[-Rpass-analysis=kernel-resource-usage\]", line)
        if not m:
            continue
        if m.group(1):
            if cur is not None and want != len(FIELDS):
                raise SystemExit("%s: the block of %s is incomplete (interleaved output? build with make -O)" % (path, cur))
            cur, want = m.group(1), 0
            kernels[cur] = {}
            continue
        key = m.group(2).strip()
        if cur is None or want >= len(FIELDS) or key != FIELDS[want]:
            raise SystemExit("%s: field '%s' out of order in the block of %s (interleaved output? build with make -O)" % (path, key, cur))
        kernels[cur][key] = m.group(3)
        want += 1
    return kernels


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    only = None
    for a in sys.argv[1:]:
        if a.startswith("--only="):
            only = a.split("=", 1)[1].split(",")
    a, b = parse(args[0]), parse(args[1])
    dem = demangle(sorted(set(a) | set(b)))

    def key(n):  # the demangled name without the float film's type
        d = re.sub(r"<lmcd::Film>", "", dem[n])
        d = re.sub(r"<lmcd::Film, ", "<", d)
        return re.sub(r"^void ", "", d)

    a, b = {key(n): v for n, v in a.items()}, {key(n): v for n, v in b.items()}
    names = {n: n for n in set(a) | set(b)}

    def short(d):  # without the parameter list; "(anonymous namespace)::" stays, it is part of the name
        return re.sub(r"\((?!anonymous namespace\)).*", "", d)

    def base(n):
        d = names[n]
        d = re.sub(r"^void ", "", d).replace("(anonymous namespace)::", "")
        return re.split(r"[<(]", d, 1)[0].split("::")[-1]

    worse = []
    print("%-34s | %s" % ("field", "first log -> second log"))
    for n in sorted(names, key=lambda k: names[k]):
        if only and base(n) not in only:
            continue
        print("\n" + short(names[n]))
        if n not in a or n not in b:
            one = a[n] if n in a else b[n]
            print("    only in the %s log: %s" % ("first" if n in a else "second", ", ".join("%s %s" % (f, one[f]) for f in SHOWN)))
            continue
        for f in SHOWN:
            mark = "" if a[n][f] == b[n][f] else "   <-- differs"
            print("    %-30s | %6s -> %6s%s" % (f, a[n][f], b[n][f], mark))
        if int(b[n]["VGPRs"]) > int(a[n]["VGPRs"]) or int(b[n]["ScratchSize [bytes/lane]"]) > int(a[n]["ScratchSize [bytes/lane]"]) or int(b[n]["Occupancy [waves/SIMD]"]) < int(a[n]["Occupancy [waves/SIMD]"]):
            worse.append(names[n])
    print("\nkernels with more VGPRs, more scratch or fewer waves per SIMD in the second log: %d" % len(worse))
    for w in worse:
        print("    " + short(w))
    return 1 if worse else 0


if __name__ == "__main__":
    sys.exit(main())
