"""`-m gpu` tier: the three wave-cooperative derivative launches (k_mala_grad, k_h2_hess, k_h2_gauss) on mixed work lists -- many bins, permuted and
replicated chains, unlisted chains in between, bin populations around a task's size, grids smaller than the task count (second and later trips of the
grid-stride loop over one reused LDS staging area), one wave walking every task.  The cases and why they are the edges: tests/coop_cases.py.

What is asserted is bit equality, derived from the code and not a tolerance: a lane's arithmetic reads its own state's LDS record and nothing else (in
k_h2_gauss `run`, rp[] and the finiteness mask are per 16-lane group), so a chain's output row is the same 32-bit words wherever the list machinery
puts the chain.  Any difference is a defect of that machinery (device/dh2coop.h and the loops around it).  The anchors of the mixed launches themselves
are the bars the one-bin tests of tests/test_gpu_h2mc.py already carry (tests/h2_refs.py)."""
import functools

import numpy as np
import pytest

from tests import coop_cases as cc
from tests import gpu_checks as gc
from tests import h2_refs
from tests.test_gpu_h2mc import _h2_gauss_probe, _h2_hess_probe

pytestmark = pytest.mark.gpu
SENT = np.uint32(cc.UNTOUCHED_BITS)
RECORD_KERNELS = ("mala_grad", "h2_hess")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b):
    """uint32 words equal bit for bit, two NaNs counting as equal"""
    return (a == b) | (np.isnan(a.view(np.float32)) & np.isnan(b.view(np.float32)))


# ---- launches, each case once
_results = {}


def run(case, again=False):
    """the probe's outputs for a case as uint32: rows [N, words] (gradient, Hessian) or (gauss [2, N, 544], px [N])"""
    if case.name in _results and not again:
        return _results[case.name]
    p = gc.pkg()
    if case.kernel == "h2_gauss":
        gauss, px = p.h2_gauss_list_probe(*cc.gauss_inputs(case, getattr(case, "pool", None)), case.stage, case.sigma, case.items, case.count, case.start, case.grid_blocks)
        out = (_bits(gauss), _bits(px))
    else:
        f = p.mala_grad_list_probe if case.kernel == "mala_grad" else p.h2_hess_list_probe
        out = _bits(f(*cc.record_inputs(case), case.items, case.count, case.start, case.grid_blocks))
    if not again:
        _results[case.name] = out
    return out


def _record_layouts(kernel):
    """every layout of tests/coop_cases.py for a record kernel: the count edges and the mixed list at every grid size, both scenes"""
    out = []
    for sid in (0, 1):
        out += [cc.count_edge_case(kernel, sid, kind) for kind in cc.POPULATION_KINDS]
        m = cc.mixed_case(kernel, sid)
        out += [m.with_grid(g) for g in cc.grid_sizes(cc.total_tasks(kernel, m.count))]
    return out


def _gauss_layouts():
    out = [cc.gauss_count_edge_case(kind, stage=k % 2) for k, kind in enumerate(cc.POPULATION_KINDS)]
    for stage in (0, 1):
        m = cc.gauss_mixed_case(stage)
        out += [m.with_grid(g) for g in cc.grid_sizes(cc.total_tasks("h2_gauss", m.count))]
    return out


def _golden_groups():
    z = cc.golden()
    for sid in (0, 1):
        for t in cc.scene_techs(sid):
            idx = cc.states_of(sid, t)
            c, l = cc.tech_of(t)
            dim = cc.tech_dim(t)
            yield sid, t, c, l, dim, idx, z["primary"][idx][:, : dim + 1].copy(), z["vert"][idx][:, : 238 + 59 * (c + l - 3)].copy(), z["scenes"][sid].copy()


# ---- the baselines: every golden state once, in the simplest launch
@functools.lru_cache(None)
def per_lane_gradients():
    """lmc_grad_batch (one lane per state, dgrad.h ComputeGradient) on every golden state -> the row k_mala_grad must write: [271, 32] uint32, the sentinel
    where the launch writes nothing, and the mask of the written words"""
    rows, written = np.full((271, cc.GRAD_ROW), SENT, np.uint32), np.zeros((271, cc.GRAD_ROW), bool)
    for sid, t, c, l, dim, idx, prim, vert, sp in _golden_groups():
        ll, g = gc.pkg().grad_batch(c, l, prim.T.copy(), sp, vert.T.copy())
        rows[idx, :dim], rows[idx, 16] = _bits(g.T.copy()), _bits(ll)
        written[idx, :dim], written[idx, 16] = True, True
    return rows, written


@functools.lru_cache(None)
def one_bin_rows(kernel):
    """the work-list probe's own simplest launch (one bin, identity order, nobody unlisted, start 0) per (scene, technique): full rows [271, words]"""
    rows = np.zeros((271, cc.GRAD_ROW if kernel == "mala_grad" else cc.HESS_ROW), np.uint32)
    for sid in (0, 1):
        for t in cc.scene_techs(sid):
            case = cc.baseline_case(kernel, sid, t)
            rows[case.src] = run(case)
    return rows


@functools.lru_cache(None)
def existing_hess_probe():
    """lmc_h2_hess_probe on every golden state: logLum [271], gradient [271, 16], Hessian [271, 256] (the upper triangle, stride dim), as uint32"""
    ll, g, h = np.zeros(271, np.uint32), np.zeros((271, 16), np.uint32), np.zeros((271, 256), np.uint32)
    for sid, t, c, l, dim, idx, prim, vert, sp in _golden_groups():
        a, b, hh = _h2_hess_probe(c, l, prim, sp, vert)
        ll[idx], g[idx, :dim], h[idx, : dim * dim] = _bits(a), _bits(b), _bits(hh).reshape(len(idx), dim * dim)
    return ll, g, h


@functools.lru_cache(None)
def existing_gauss_probe():
    """lmc_h2_gauss_probe (stage 1, flags clear, one bin) on the Gaussian pool, one launch per dim -> the record every launch must write for a pool
    state: rows [P, 544] uint32 with the sentinel where the launch writes nothing, px [P]"""
    pool = cc.gauss_pool()
    P = len(pool["dim"])
    rows, px = np.full((P, cc.GAUSS_ROW), SENT, np.uint32), np.zeros(P, np.uint32)
    for d in cc.GAUSS_DIMS:
        idx = cc.gauss_states_of_dim(d)
        out, x = _h2_gauss_probe(pool["grad"][idx, :d], pool["hess"][idx, : d * d].reshape(len(idx), d, d), cc.SIGMA, pool["offset"][idx, :d])
        out = _bits(out)
        for k, i in enumerate(idx):
            rows[i, :d], rows[i, 16:18] = out[k, :d], out[k, 16:18]
            if out[k].view(np.float32)[17] == cc.H2K_DENSE:  # (an isotropic record stores no matrices)
                rows[i, 32: 32 + d * d], rows[i, 288: 288 + d * d] = out[k, 32: 32 + d * d], out[k, 288: 288 + d * d]
        px[idx] = _bits(x)
    kinds = rows[:, 17].view(np.float32)
    assert (kinds == cc.H2K_DENSE).sum() > len(kinds) // 2 and (kinds == cc.H2K_ISO_EARLYOUT).sum() > len(kinds) // 8  # both outcomes are in the pool
    return rows, px


def _assert_rows(case, got, want, what):
    """listed chains hold `want` (indexed by pool state), unlisted ones the sentinel"""
    assert (got[~case.listed] == SENT).all(), "%s: %s: a launch wrote the row of an unlisted chain" % (case.name, what)
    exp = want[case.src[case.listed]]
    bad = np.flatnonzero((got[case.listed] != exp).any(axis=1))
    assert len(bad) == 0, "%s: %s: %d of %d listed rows differ, first chain %d (bin %d, state %d)" % (
        case.name, what, len(bad), case.listed.sum(), np.flatnonzero(case.listed)[bad[0]], case.bin_of_chain()[np.flatnonzero(case.listed)[bad[0]]], case.src[case.listed][bad[0]])


# ---- the plan
@pytest.mark.parametrize("kernel", cc.KERNELS)
def test_plan_probe_returns_the_documented_states_per_task(kernel):
    p = gc.pkg()
    for t in cc.golden_techs():
        assert p.coop_plan_probe(cc.KERNELS.index(kernel), t)[0] == cc.ipw(kernel, t), t


# ---- k_mala_grad against the per-lane kernel
def test_mala_grad_rows_equal_the_per_lane_kernel_bit_for_bit():
    """Every golden state in every layout: gradient and logLum of k_mala_grad are the 32-bit words lmc_grad_batch computes for the same state (two NaNs
    count as equal); the words of a row the launch does not own, and every unlisted chain's row, keep the sentinel.  This is gradcoop.hip's own claim
    (strict arithmetic, forward components never mix)."""
    want, written = per_lane_gradients()
    seen = set()
    for case in _record_layouts("mala_grad"):
        got = run(case)
        assert (got[~case.listed] == SENT).all(), case.name
        rows, src = got[case.listed], case.src[case.listed]
        same = np.where(written[src], _same(rows, want[src]), rows == SENT)
        bad = np.flatnonzero(~same.all(axis=1))
        assert len(bad) == 0, (case.name, len(bad), "first: chain %d state %d words %s" % (np.flatnonzero(case.listed)[bad[0]], src[bad[0]], np.flatnonzero(~same[bad[0]])))
        seen |= set(src)
    assert len(seen) == 271  # every golden state took part


def test_mala_grad_mixed_launch_meets_the_golden_bar():
    """the mixed launch itself against the reference programs' mala_grad vectors, at the bar of test_golden_derivative_vectors_through_the_c_abi:
    logLum 5e-3, gradient 1e-2 relative with at most 1 % of the vectors outside"""
    z = cc.golden()
    n = bad = 0
    for sid in (0, 1):
        case = cc.mixed_case("mala_grad", sid).with_grid(3)
        rows = run(case).view(np.float32)
        for chain in np.flatnonzero(case.listed):
            i = case.src[chain]
            dim = cc.tech_dim(z["tech"][i])
            assert abs(rows[chain, 16] - z["loglum"][i]) < 5e-3
            rg = z["mala_grad"][i][:dim]
            n, bad = n + 1, bad + (np.linalg.norm(rg - rows[chain, :dim]) / max(np.linalg.norm(rg), 1e-2) > 1e-2)
    assert n >= 250 and bad <= n // 100, (bad, n)


# ---- layout independence
@pytest.mark.parametrize("kernel", RECORD_KERNELS)
def test_rows_do_not_depend_on_the_work_list(kernel):
    """A chain's whole output row in any mixed, permuted, replicated or small-grid launch is bit-equal to its state's row from the one-bin,
    identity-order launch; rows of unlisted chains keep the sentinel.  For the Hessian the one-bin launch is also the existing probe's."""
    base = one_bin_rows(kernel)
    if kernel == "h2_hess":
        z = cc.golden()
        ll, g, h = existing_hess_probe()
        for i in range(271):
            dim = cc.tech_dim(z["tech"][i])
            iu = np.triu_indices(dim)
            hess = base[i, 32: 32 + dim * dim].reshape(dim, dim)
            assert base[i, 16] == ll[i] and (base[i, :dim] == g[i, :dim]).all() and (hess[iu] == h[i, : dim * dim].reshape(dim, dim)[iu]).all(), i
            # what the launch does not own stays untouched: the gradient's tail, the words up to the Hessian, below the 2 x 2 diagonal blocks, behind the matrix
            lower = np.tril_indices(dim, -1)
            off_block = lower[0] // 2 != lower[1] // 2
            assert (base[i, dim:16] == SENT).all() and (base[i, 17:32] == SENT).all() and (base[i, 32 + dim * dim:] == SENT).all()
            assert (hess[lower[0][off_block], lower[1][off_block]] == SENT).all() and (hess[iu] != SENT).all()
    for case in _record_layouts(kernel):
        _assert_rows(case, run(case), base, kernel)


def test_mixed_hessian_launch_meets_the_golden_bar():
    """the mixed launch itself at the bar of test_step_hessian_launch_matches_reference_programs_on_golden_vectors (tests/h2_refs.py)"""
    z = cc.golden()
    checked, bad = 0, []
    for sid in (0, 1):
        case = cc.mixed_case("h2_hess", sid).with_grid(3)
        rows = run(case).view(np.float32)
        for chain in np.flatnonzero(case.listed):
            i = case.src[chain]
            dim = cc.tech_dim(z["tech"][i])
            err = h2_refs.golden_hessian_errors(z, i, dim, rows[chain, 16], rows[chain, :dim], rows[chain, 32: 32 + dim * dim].reshape(dim, dim))
            if err is None:
                continue
            checked += 1
            if max(err) > 1e-2:
                bad.append((sid, int(i)) + err)
    assert checked >= 250 and len(bad) <= checked // 100, bad


def _gauss_expected(case, want_rows, want_px):
    """both buffers and px as the launch must leave them"""
    gauss, px = np.full((2, case.N, cc.GAUSS_ROW), SENT, np.uint32), np.full(case.N, SENT, np.uint32)
    chains = np.flatnonzero(case.listed)
    buf = (((case.flags[chains] & cc.F_GSEL) != 0) != (case.stage != 0)).astype(int)  # the buffer F_GSEL XOR stage selects
    gauss[buf, chains] = want_rows[case.src[chains]]
    if case.stage:
        px[chains] = want_px[case.src[chains]]
    return gauss, px


def test_gaussian_records_do_not_depend_on_the_work_list():
    """Every layout, stage 0 and 1, F_GSEL set on about half the chains, dims 6 to 16 in one launch: a listed chain's record -- in the buffer F_GSEL XOR
    stage selects -- is bit-equal to the existing probe's one-bin launch of the same state, px (stage 1) too; the other buffer, the words of a record the
    launch does not own (an isotropic record stores no matrices), px at stage 0 and everything of an unlisted chain keep the sentinel."""
    want_rows, want_px = existing_gauss_probe()
    for case in _gauss_layouts():
        gauss, px = run(case)
        exp_g, exp_px = _gauss_expected(case, want_rows, want_px)
        for b in (0, 1):
            bad = np.flatnonzero((gauss[b] != exp_g[b]).any(axis=1))
            assert len(bad) == 0, "%s: buffer %d: %d rows differ, first chain %d (listed %s, bin %d, flags %#x, words %s)" % (
                case.name, b, len(bad), bad[0], case.listed[bad[0]], case.bin_of_chain()[bad[0]], case.flags[bad[0]], np.flatnonzero(gauss[b, bad[0]] != exp_g[b, bad[0]])[:8])
        assert (px == exp_px).all(), (case.name, np.flatnonzero(px != exp_px)[:8])


@pytest.mark.parametrize("stage", [0, 1])
def test_mixed_gaussian_launch_meets_the_eigh_bar(stage):
    """the mixed launch itself against the float64 numpy.linalg.eigh recomputation, at the bars of test_device_h2mc_gaussian_against_numpy_eigh"""
    pool = cc.gauss_pool()
    case = cc.gauss_mixed_case(stage).with_grid(3)
    gauss, px = (a.view(np.float32) for a in run(case))
    chains = np.flatnonzero(case.listed)
    buf = (((case.flags[chains] & cc.F_GSEL) != 0) != (stage != 0)).astype(int)
    n_dense = n_iso = 0
    for k, d in enumerate(cc.GAUSS_DIMS):
        sel = pool["dim"][case.src[chains]] == d
        at = case.src[chains[sel]] - k * cc.GAUSS_PER_DIM  # the states' positions among the dim's float64 originals
        H, g, o = pool["f64"][d]
        a, b = h2_refs.check_gauss_against_eigh(gauss[buf[sel], chains[sel]], px[chains[sel]] if stage else None, H[at], g[at], o[at], cc.SIGMA)
        n_dense, n_iso = n_dense + a, n_iso + b
    assert n_dense >= 250 and n_iso >= 80, (n_dense, n_iso)


# ---- the stage with no takers
@pytest.mark.parametrize("kernel", cc.KERNELS)
def test_empty_stage_writes_nothing(kernel):
    case = cc.empty_case(cc.gauss_mixed_case(1) if kernel == "h2_gauss" else cc.mixed_case(kernel, 1))
    out = run(case)  # (the probe returns 0: the binding raises otherwise)
    for a in out if kernel == "h2_gauss" else (out,):
        assert (a == SENT).all()


# ---- a non-finite state beside finite ones
@pytest.mark.parametrize("group", [0, 3])
@pytest.mark.parametrize("where", ["hess", "grad"])
def test_nonfinite_state_does_not_leak_into_its_wave_neighbours(where, group):
    """One task of four dense states, one of them with a non-finite Hessian / gradient entry, in the first or the last 16-lane group: the three finite states
    equal their solo results bit for bit, the non-finite one is the isotropic record mutation_h2mc.h:80-85 and h2mc.cpp:84-92 prescribe (mean 0,
    logDet = dim log(1 / sigma^2) -- at the bar of test_device_h2mc_gaussian_against_numpy_eigh --, kind H2K_ISO_EARLYOUT, no matrices)."""
    want_rows, want_px = existing_gauss_probe()
    case, pool, bad = cc.gauss_nonfinite_case(where, group)
    case.pool = pool
    gauss, px = run(case)
    d = cc.GAUSS_NONFINITE_DIM
    assert (gauss[0] == SENT).all()  # stage 1, flags clear: the second buffer
    for chain in range(4):
        row = gauss[1, chain]
        if chain != bad:
            assert want_rows[case.src[chain], 17].view(np.float32) == cc.H2K_DENSE
            assert (row == want_rows[case.src[chain]]).all() and px[chain] == want_px[case.src[chain]], (chain, np.flatnonzero(row != want_rows[case.src[chain]])[:8])
            continue
        f = row.view(np.float32)
        assert (f[:d] == 0).all() and f[17] == cc.H2K_ISO_EARLYOUT and abs(f[16] - d * np.log(1.0 / cc.SIGMA ** 2)) < 1e-3 * d, f[:18]
        assert (row[d:16] == SENT).all() and (row[18:] == SENT).all()
        assert np.isfinite(px[chain: chain + 1].view(np.float32)).all()


# ---- determinism
@pytest.mark.parametrize("kernel", cc.KERNELS)
def test_one_block_mixed_launch_repeats_its_bytes(kernel):
    """one wave walks every task of the mixed list, twice: identical bytes; and they are the bytes of every other grid size"""
    m = cc.gauss_mixed_case(1) if kernel == "h2_gauss" else cc.mixed_case(kernel, 1)
    one = m.with_grid(1)
    a, b = run(one), run(one, again=True)
    pairs = list(zip(a, b)) if kernel == "h2_gauss" else [(a, b)]
    assert all(x.tobytes() == y.tobytes() for x, y in pairs)
    for g in cc.grid_sizes(cc.total_tasks(kernel, m.count))[1:]:
        o = run(m.with_grid(g))
        assert all(x.tobytes() == y.tobytes() for x, y in (zip(a, o) if kernel == "h2_gauss" else [(a, o)])), g
