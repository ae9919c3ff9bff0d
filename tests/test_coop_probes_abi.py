"""CPU tier: the surface of the work-list probes of the wave-cooperative derivative launches (include/lmc_abi.h: lmc_mala_grad_list_probe,
lmc_h2_hess_list_probe, lmc_h2_gauss_list_probe, lmc_coop_plan_probe) -- the declarations, the exports, the Python bindings, the plan (which needs no
device) and every refusal: a bad work list is turned away on the host, before the first device call, with the argument named in lmc_last_error.  What
the launches compute on a good list needs a GPU: tests/test_gpu_coop_lists.py."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import coop_cases as cc
from tests import gpu_checks as gc


def _pattern(name, args):
    body = r"\s*,\s*".join(r"\s*".join(re.escape(tok) for tok in re.findall(r"\w+|\*", a)) for a in args.split(","))
    return r"int\s+" + name + r"\s*\(\s*" + body + r"\s*\)\s*;"


_RECORD_ARGS = ("int N, const float *primary, const int *c, const int *l, const float *vert, const float *scene38, int n_list, const int *items, const int *count, "
                "const int *start, int grid_blocks, float *out")
DECLS = {
    "lmc_mala_grad_list_probe": _RECORD_ARGS,
    "lmc_h2_hess_list_probe": _RECORD_ARGS,
    "lmc_h2_gauss_list_probe": "int N, const int *dim, const float *grad, const float *hess, const int *flags, const float *offset, int stage, float sigma, int n_list, "
                               "const int *items, const int *count, const int *start, int grid_blocks, float *gauss, float *px",
    "lmc_coop_plan_probe": "int kernel, int tech, int *states_per_task, int *rec_words",
    # the two earlier probes keep their signatures: they are the new ones with everything in one bin
    "lmc_h2_hess_probe": "int c, int l, int n, const float *primary, const float *scene38, const float *vert, float *loglum, float *grad, float *hess",
    "lmc_h2_gauss_probe": "int n, int dim, const float *grad, const float *hess, float sigma, const float *offset, float *gauss, float *px",
}


def test_the_calls_are_declared_with_the_contract():
    hdr = open(os.path.join(gc.ROOT, "include", "lmc_abi.h")).read()
    for name, args in DECLS.items():
        assert re.search(_pattern(name, args), hdr), name
    assert hdr.index("probes used by the parity tests") < min(hdr.index(name + "(") for name in DECLS)
    assert re.search(r"#define\s+LMC_PROBE_VERT_WORDS\s+%d\s" % cc.VERT_WORDS, hdr)
    p = gc.pkg()
    assert p.PROBE_VERT_WORDS == cc.VERT_WORDS and p.PROBE_BINS == cc.BINS and p.PROBE_UNTOUCHED_BITS == cc.UNTOUCHED_BITS and p.COOP_KERNELS == cc.KERNELS
    for word in ("k_mala_grad", "k_h2_hess", "k_h2_gauss", "n = 0 is not a call", "0x7fc0beef", "[1, 4096]", "before any device"):
        assert word in hdr, word


def test_the_calls_are_exported():
    L = ctypes.CDLL(gc.pkg().LIB_PATH)
    for name in DECLS:
        assert hasattr(L, name), name


def test_python_bindings():
    p = gc.pkg()
    L = p.lib()
    for name in ("lmc_mala_grad_list_probe", "lmc_h2_hess_list_probe", "lmc_h2_gauss_list_probe", "lmc_coop_plan_probe"):
        assert getattr(L, name).argtypes is not None and len(getattr(L, name).argtypes) == len(DECLS[name].split(",")), name
    for f in ("mala_grad_list_probe", "h2_hess_list_probe", "h2_gauss_list_probe", "coop_plan_probe"):
        assert callable(getattr(p, f, None)), f


def test_the_probes_stay_host_code_and_share_the_kernels_plan():
    csrc = os.path.join(gc.ROOT, "langevin-mcmc_amd", "csrc")
    src = open(os.path.join(csrc, "host", "list_probes.cpp")).read()
    assert "__global__" not in src and "hipLaunchKernelGGL" not in src  # the launches are the renderer's own
    plan = open(os.path.join(csrc, "device", "dh2coop.h")).read()
    for fn, unit in (("MalaGradStatesPerTask", "gradcoop.hip"), ("H2HessStatesPerTask", "h2hess.hip"), ("H2_GAUSS_STATES_PER_TASK", "h2gauss.hip")):
        assert fn in plan and fn in src and fn in open(os.path.join(csrc, "device", unit)).read(), fn  # one definition, used by kernel and probe


def test_the_plan_probe_needs_no_device_and_states_the_documented_formulas():
    p = gc.pkg()
    for k, kernel in enumerate(cc.KERNELS):
        for t in range(cc.NTECH):
            assert p.coop_plan_probe(k, t) == (cc.ipw(kernel, t), cc.HESS_ROW if kernel == "h2_gauss" else cc.rec_words(t)), (kernel, t)
    for k, t in ((3, 0), (-1, 0), (0, 42), (1, -1)):
        with pytest.raises(RuntimeError, match="kernel" if k not in (0, 1, 2) else "tech"):
            p.coop_plan_probe(k, t)


def _record_call(name, case, **kw):
    """the raw C call (return value, message) on a case's arrays, any argument replaced by keyword"""
    L = gc.pkg().lib()
    P = gc.pkg().P
    pr, c, l, ve, sc = cc.record_inputs(case)
    a = dict(N=case.N, n_list=case.n_list, items=case.items, count=case.count, start=case.start, grid_blocks=case.grid_blocks, c=c, l=l)
    a.update(kw)
    keep = [np.ascontiguousarray(a[k], np.int32) for k in ("c", "l", "items", "count", "start")]
    out = np.zeros((case.N, 288), np.float32)
    r = getattr(L, name)(a["N"], P(pr), P(keep[0]), P(keep[1]), P(ve), P(sc), a["n_list"], P(keep[2]), P(keep[3]), P(keep[4]), a["grid_blocks"], P(out))
    return r, (L.lmc_last_error() or b"").decode()


def _gauss_call(case, **kw):
    L = gc.pkg().lib()
    P = gc.pkg().P
    d, g, h, f, o = cc.gauss_inputs(case)
    a = dict(N=case.N, n_list=case.n_list, items=case.items, count=case.count, start=case.start, grid_blocks=case.grid_blocks, dim=d, stage=1, sigma=0.01)
    a.update(kw)
    keep = [np.ascontiguousarray(a[k], np.int32) for k in ("dim", "items", "count", "start")] + [np.ascontiguousarray(x) for x in (g, h, f, o)]
    gauss, px = np.zeros((2, case.N, 544), np.float32), np.zeros(case.N, np.float32)
    r = L.lmc_h2_gauss_list_probe(a["N"], P(keep[0]), P(keep[4]), P(keep[5]), P(keep[6]), P(keep[7]), a["stage"], a["sigma"], a["n_list"], P(keep[1]), P(keep[2]), P(keep[3]),
                                  a["grid_blocks"], P(gauss), P(px))
    return r, (L.lmc_last_error() or b"").decode()


def _bad_lists(case):
    """(what, replaced arguments, the argument the message must name) for every refusal of include/lmc_abi.h"""
    full = np.flatnonzero(case.count)
    b0, b1, blast = full[0], full[1], full[-1]
    out = [("n_list = 0", dict(n_list=0), "n_list"), ("N < n_list", dict(N=case.n_list - 1), "N = "), ("grid 0", dict(grid_blocks=0), "grid_blocks"),
           ("grid 4097", dict(grid_blocks=4097), "grid_blocks")]
    it = case.items.copy()
    it[3] = case.N
    out.append(("item = N", dict(items=it.copy()), "items[3]"))
    it[3] = -1
    out.append(("item = -1", dict(items=it.copy()), "items[3]"))
    it[3] = case.items[2]
    out.append(("item twice", dict(items=it.copy()), "items[3]"))
    cnt = case.count.copy()
    cnt[b0] = -2
    out.append(("negative count", dict(count=cnt), "count[%d]" % b0))
    st = case.start.copy()
    st[b1] = case.n_list - case.count[b1] + 1
    out.append(("bin past the list", dict(start=st.copy()), "start[%d]" % b1))
    st[b1] = -1
    out.append(("negative start", dict(start=st.copy()), "start[%d]" % b1))
    st[b1] = case.start[b0]
    out.append(("overlapping bins", dict(start=st.copy()), "overlap"))
    it = case.items.copy()
    a, b = case.start[b0], case.start[blast]
    it[a], it[b] = it[b], it[a]
    out.append(("wrong technique", dict(items=it), "technique of its bin"))
    return out


@pytest.mark.parametrize("name", ["lmc_mala_grad_list_probe", "lmc_h2_hess_list_probe"])
def test_record_probes_refuse_bad_lists_before_any_device_call(name):
    """(this tier has no device: a probe that got as far as the device would fail with another message, or not return at all)"""
    case = cc.mixed_case("h2_hess" if "hess" in name else "mala_grad", 0)
    for what, kw, needle in _bad_lists(case):
        r, msg = _record_call(name, case, **kw)
        assert r != 0 and msg.startswith(name + ": ") and needle in msg and "HIP" not in msg and "device" not in msg, (what, msg)
    r, msg = _record_call(name, case, items=case.items[::-1].copy())  # a permuted list no longer matches its bins' techniques
    assert r != 0 and "(c, l) of chain" in msg
    c_bad = cc.record_inputs(case)[1].copy()
    c_bad[case.items[0]] += 1
    r, msg = _record_call(name, case, c=c_bad)
    assert r != 0 and "(c, l) of chain %d (items[0])" % case.items[0] in msg


def test_gauss_probe_refuses_bad_lists_before_any_device_call():
    case = cc.gauss_mixed_case(1)
    name = "lmc_h2_gauss_list_probe"
    for what, kw, needle in _bad_lists(case):
        r, msg = _gauss_call(case, **kw)
        assert r != 0 and msg.startswith(name + ": ") and needle in msg and "HIP" not in msg and "device" not in msg, (what, msg)
    d = cc.gauss_inputs(case)[0].copy()
    d[case.items[0]] += 2 if d[case.items[0]] < 16 else -2
    r, msg = _gauss_call(case, dim=d)
    assert r != 0 and "dim of chain %d (items[0])" % case.items[0] in msg
    d[5] = 7
    r, msg = _gauss_call(case, dim=d)
    assert r != 0 and "dim[5] = 7" in msg
    for kw, needle in ((dict(stage=2), "stage"), (dict(sigma=0.0), "sigma")):
        r, msg = _gauss_call(case, **kw)
        assert r != 0 and needle in msg


def test_the_earlier_probes_keep_the_n_zero_rule():
    L = gc.pkg().lib()
    L.lmc_h2_hess_probe.argtypes = [ctypes.c_int] * 3 + [ctypes.c_void_p] * 6
    L.lmc_h2_gauss_probe.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    z = np.zeros(1024, np.float32)
    P = gc.pkg().P
    assert L.lmc_h2_hess_probe(4, 0, 0, P(z), P(z), P(z), None, None, None) != 0 and b"n >= 1" in L.lmc_last_error()
    assert L.lmc_h2_gauss_probe(0, 6, P(z), P(z), 0.01, None, None, None) != 0 and b"n >= 1" in L.lmc_last_error()
    assert L.lmc_h2_hess_probe(2, 0, 1, P(z), P(z), P(z), None, None, None) != 0 and b"technique" in L.lmc_last_error()
