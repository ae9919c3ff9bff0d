"""CPU tier: the surface of the list probes (include/lmc_abi.h "probes used by the parity tests": scan, radix sort, work lists, bins, split, cache push,
relocation plan, chain slots) -- the declarations, the exports and the Python bindings.  What they compute needs a GPU: tests/test_gpu_lists.py."""
import ctypes
import os
import re

from tests import gpu_checks as gc
from tests import list_cases as lc

DECLS = {
    "lmc_scan_probe": "int n, const int *in, int *out",
    "lmc_radix_sort_probe": "int n, int n_max, const unsigned *keys, int *out_vals, unsigned *out_keys",
    "lmc_sort_by_technique_probe": "int n_chains, const unsigned char *next_kind, int n_list, const int *list, int max_entries, int *out",
    "lmc_build_lists_probe": "int N, const unsigned char *next_kind, int sort_plain, unsigned lean_dims, int want_step_kind, int *out_large, int *out_generic, "
                             "int *out_plain, int *out_counts, unsigned char *out_step_kind",
    "lmc_bins_compact_probe": "int N, const int *bin_of, const int *count, int n_list, const int *list, int grid_blocks, int *out_items, int *out_start",
    "lmc_split_list_probe": "int n_list, const int *list, int parts, int stride, int grid_blocks, int *out_sub, int *out_sub_count",
    "lmc_cache_push_probe": "int N, const int *push_dim, const float *push_data, const int *slot_of, const int *initial_counts, float *out_rows, float *out_weights, "
                            "int *out_counts, int *out_push_dim",
    "lmc_reloc_plan_probe": "int N, const unsigned char *step_kind, const int *c, const int *l, const int *flags, const unsigned *placed_key, int without_gaussian_only, "
                            "int capacity, int skipped_before, int *out_count, int *out_members, int *out_sorted",
    "lmc_chain_slots": "lmc_ctx *ctx, int *slot_of, int *chain_id",
}


def _pattern(name, args):
    body = r"\s*,\s*".join(r"\s*".join(re.escape(tok) for tok in re.findall(r"\w+|\*", a)) for a in args.split(","))
    return r"int\s+" + name + r"\s*\(\s*" + body + r"\s*\)\s*;"


def test_the_calls_are_declared_with_the_contract():
    hdr = open(os.path.join(gc.ROOT, "include", "lmc_abi.h")).read()
    for name, args in DECLS.items():
        assert re.search(_pattern(name, args), hdr), name
    assert hdr.index("probes used by the parity tests") < min(hdr.index(name + "(") for name in DECLS)
    # the constants the Python side and the references repeat
    for define, value in (("LMC_PROBE_SENTINEL", "(-0x5a5a5a5b)"), ("LMC_PROBE_BINS", str(lc.BINS)), ("LMC_PROBE_CACHE_ROWS", str(lc.CACHE_ROWS))):
        assert re.search(r"#define\s+%s\s+%s\s" % (define, re.escape(value)), hdr), define
    p = gc.pkg()
    assert p.PROBE_SENTINEL == lc.SENTINEL == -0x5A5A5A5B and p.PROBE_BINS == lc.BINS and p.PROBE_CACHE_ROWS == lc.CACHE_ROWS
    assert p.PROBE_UNTOUCHED_BITS == lc.UNTOUCHED_BITS
    for word in ("LaunchInclusiveScan", "LaunchRadixSort24", "LaunchSortByTechnique", "LaunchBuildLists", "LaunchBinsCompact", "LaunchSplitList", "LaunchCachePush",
                 "LaunchRelocPlan", "n = 0 is not a call"):
        assert word in hdr, word


def test_the_calls_are_exported():
    L = ctypes.CDLL(gc.pkg().LIB_PATH)
    for name in DECLS:
        assert hasattr(L, name), name


def test_python_bindings():
    p = gc.pkg()
    L = p.lib()
    for name, args in DECLS.items():
        assert getattr(L, name).argtypes is not None and len(getattr(L, name).argtypes) == len(args.split(",")), name
    for f in ("scan_probe", "radix_sort_probe", "sort_by_technique_probe", "build_lists_probe", "bins_compact_probe", "split_list_probe", "cache_push_probe",
              "reloc_plan_probe"):
        assert callable(getattr(p, f, None)), f
    assert callable(getattr(p.Renderer, "chain_slots", None))


def test_the_probes_live_in_their_own_host_unit():
    mk = open(os.path.join(gc.ROOT, "langevin-mcmc_amd", "csrc", "Makefile")).read()
    assert re.search(r"^HOST_HIP\s*:=.*\blist_probes\b", mk, re.M)
    src = open(os.path.join(gc.ROOT, "langevin-mcmc_amd", "csrc", "host", "list_probes.cpp")).read()
    assert "__global__" not in src and "hipLaunchKernelGGL" not in src  # host code only: the launches are the renderer's own
