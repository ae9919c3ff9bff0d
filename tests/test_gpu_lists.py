"""The bookkeeping launches the step kernels run on, each on its own on the device (probes of include/lmc_abi.h, host/list_probes.cpp) against the
exact references of tests/list_cases.py: the 2048-element tiled inclusive scan, the 24-bit radix sort, the counting sort by technique, the work
lists, the stage bins, the list split, the cache-push pack, the plan of a relocation -- at sizes with remainder tiles and in the multi-tile /
multi-batch branches that no render of the suite reaches.  Then through real contexts with ragged chain counts: relocation on against off, the
slot tables a permutation at every point, the slots in key order right after a full re-sort, and the two move variants the library ships but no
other test runs (LMC_RELOC_COOP=0, LMC_RELOC_FINE=1), each in a fresh process.  Everything is an integer or a copied word: exact comparisons only.
The probe cases share one process and need no context."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import gpu_checks as gc
from tests import list_cases as lc
from tests import test_gpu_relocate as rel

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("reloc_worker", os.path.join(gc.ROOT, "tests", "helpers", "reloc_worker.py"))
worker = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(worker)


# ================================================================================================ the probes
@pytest.mark.parametrize("n", lc.SCAN_SIZES)
def test_inclusive_scan(n):
    """n = 0 is not a legal call (every caller passes at least 256 elements; the probe refuses it) and is not tested.  From 2048 * 256 + 1 elements on
    k_scan_sums runs its second batch of 256 tile sums, from 2048 * 512 + 1 its third."""
    p = gc.pkg()
    for kind in lc.SCAN_INPUTS:
        v = lc.scan_input(kind, n)
        got = p.scan_probe(v)
        want = lc.scan_ref(v)
        bad = np.flatnonzero(got != want)
        assert not len(bad), (kind, n, bad[:5], got[bad[:5]], want[bad[:5]])


@pytest.mark.parametrize("n,n_max", lc.RADIX_SIZES)
def test_radix_sort_24(n, n_max):
    """values and keys equal the stable argsort; from index n on both outputs keep the sentinel (n lives in device memory, as in the renderer)"""
    p = gc.pkg()
    for kind in lc.RADIX_KEYS:
        keys = lc.radix_keys(kind, n_max)
        vals, out = p.radix_sort_probe(keys, n)
        want_vals, want_out = lc.radix_ref(keys, n)
        bad = np.flatnonzero(vals != want_vals)
        assert not len(bad), (kind, n, n_max, bad[:5], vals[bad[:5]], want_vals[bad[:5]])
        assert np.array_equal(out, want_out), (kind, n, n_max)


@pytest.mark.parametrize("count", lc.SORT_COUNTS)
def test_sort_by_technique(count):
    """max_entries (what the (chunk, key) histogram is sized for) equal to the count and three chunks above it; the probe itself fails when an
    entry beyond the count is written"""
    p = gc.pkg()
    for single_key in (0, 1):
        next_kind, entries = lc.sort_case(count, single_key)
        for max_entries in (count, count + 3 * lc.SORT_CHUNK):
            out = p.sort_by_technique_probe(next_kind, entries, max_entries)
            lc.check_sort_by_technique(next_kind, entries, out)


@pytest.mark.parametrize("n", lc.BUILD_SIZES)
def test_build_lists(n):
    p = gc.pkg()
    for kind in lc.BUILD_KINDS:
        next_kind = lc.build_kinds(kind, n)
        for sort_plain in range(4):
            for lean in lc.BUILD_LEAN:
                got = p.build_lists_probe(next_kind, sort_plain, lean, want_step_kind=True)
                try:
                    lc.check_build_lists(next_kind, sort_plain, lean, got)
                except AssertionError as e:
                    raise AssertionError((kind, n, sort_plain, hex(lean)) + e.args) from e
            got = p.build_lists_probe(next_kind, sort_plain, 0, want_step_kind=False)  # relocation off: the launch has no stepKind array
            assert got["step_kind"] is None
            lc.check_build_lists(next_kind, sort_plain, 0, got, with_step_kind=False)


@pytest.mark.parametrize("length", lc.BINS_LENGTHS)
def test_bins_compact(length):
    p = gc.pkg()
    for kind in lc.BINS_CASES:
        bin_of, count, entries = lc.bins_case(kind, length)
        for grid in lc.BINS_GRIDS:
            items, start = p.bins_compact_probe(bin_of, count, entries, grid)
            try:
                lc.check_bins_compact(bin_of, count, entries, items, start)
            except AssertionError as e:
                raise AssertionError((kind, length, grid) + e.args) from e


@pytest.mark.parametrize("parts", lc.SPLIT_PARTS)
def test_split_list(parts):
    p = gc.pkg()
    for total in lc.split_totals(parts):
        entries = np.random.default_rng(total + parts).permutation(4000)[:total].astype(np.int32)
        stride = lc.split_stride(total, parts)
        want_sub, want_count = lc.split_ref(entries, parts, stride)
        for grid in lc.SPLIT_GRIDS:
            sub, cnt = p.split_list_probe(entries, parts, stride, grid)
            assert np.array_equal(cnt, want_count), (parts, total, grid, cnt, want_count)
            assert np.array_equal(sub, want_sub), (parts, total, grid)


@pytest.mark.parametrize("n", lc.PUSH_SIZES)
def test_cache_push(n):
    """rows bit for bit (uint32 views: the untouched words are NaNs), in chain-id order through slot_of, cut at 3000; counts saturate; push_dim cleared
    for the consumed chains only"""
    p = gc.pkg()
    for kind in lc.PUSH_CASES:
        for scrambled in (0, 1):
            push_dim, data, slot_of, init = lc.push_case(kind, n, scrambled)
            rows, w, counts, after = p.cache_push_probe(push_dim, data, slot_of, init)
            want_rows, want_w, want_counts, want_after = lc.push_ref(push_dim, data, slot_of, init)
            tag = (kind, n, scrambled)
            assert np.array_equal(counts, want_counts), tag + (counts, want_counts)
            assert np.array_equal(after, want_after), tag
            assert np.array_equal(w.view(np.uint32), want_w), tag
            bad = np.argwhere(rows.view(np.uint32) != want_rows)
            assert not len(bad), tag + (bad[:5],)


@pytest.mark.parametrize("n", lc.RELOC_SIZES)
def test_relocation_plan(n):
    """members, their stable order by key and the count, at the capacity, one below it (skipped: count[1] goes from 2 to 3, and on the repeat from 3 to 4)
    and at capacity 0"""
    p = gc.pkg()
    for kind in lc.RELOC_CASES:
        case = lc.reloc_case(kind, n)
        for wgo in ((False, True) if kind == "gauss" else (False,)):
            M = len(lc.reloc_members(case, wgo))
            for capacity, skipped_before in ((n, 0), (M, 2), (M - 1, 2), (M - 1, 3), (0, 5)):
                if capacity < 0:
                    continue
                got = p.reloc_plan_probe(case["step_kind"], case["c"], case["l"], case["flags"], case["placed_key"], wgo, capacity, skipped_before)
                want = lc.reloc_plan_ref(case, wgo, capacity, skipped_before)
                tag = (kind, n, wgo, capacity, skipped_before, M)
                assert list(got[0]) == list(want[0]), tag + (got[0], want[0])
                if M > capacity:
                    assert got[0][0] == 0 and got[0][1] == skipped_before + 1, tag
                assert np.array_equal(got[1], want[1]), tag + ("members",)
                bad = np.flatnonzero(got[2] != want[2])
                assert not len(bad), tag + ("sorted", bad[:5], got[2][bad[:5]], want[2][bad[:5]])


# ================================================================================================ through real contexts, ragged chain counts
RAGGED = (1000, 4097, 5000)  # a remainder in every tile size (64, 1024, 2048, 4096); 4097 and 5000: several relocation tiles, two radix blocks
MALA_OPTS = {"largestepprob": 0.5, "largestepscale": 1.0}
_memo = {}


def _off(n, mala):
    """the relocation-off run (tests/test_gpu_relocate.py _run), once per process"""
    if (n, mala) not in _memo:
        _memo[(n, mala)] = rel._run(False, mala, n, worker.POINTS[-1], MALA_OPTS if mala else worker.PLAIN_OPTS, checkpoints=worker.POINTS[:-1], max_depth=4 if mala else 6)
    return _memo[(n, mala)]


def _check_slots(slot_of, chain_id, n):
    assert np.array_equal(np.sort(slot_of), np.arange(n)), "slot_of is not a permutation of the slots"
    assert np.array_equal(chain_id[slot_of], np.arange(n)), "chain_id[slot_of[i]] != i"


def _check_transparent(n, mala, off, film0, on, film1, moved_needed=True):
    keys = ("steps", "largeSteps", "accepted", "resets") + (("cacheQueries", "cacheHits", "gradCalls", "cacheReadyMask") if mala else ())
    for (s0, st0, r0), (s1, st1, r1, slot_of, chain_id) in zip(off, on):
        assert r0 is None and r1 is not None and r1["relocations"] > 0 and r1["slots"] == n and r1["skipped"] == 0
        rel._same_states(s0, s1)
        for k in keys:
            assert st0[k] == st1[k], (k, st0[k], st1[k])
        assert st1["weightSum"] == pytest.approx(st0["weightSum"], rel=1e-6)
        _check_slots(slot_of, chain_id, n)
    if moved_needed:  # the chains really live elsewhere: a move that moves nothing would pass everything above
        assert (on[-1][3] != np.arange(n)).sum() > 0.9 * n
    l0, l1 = gc.lum(film0), gc.lum(film1)
    assert np.linalg.norm(l0 - l1) <= 1e-5 * np.linalg.norm(l0)


@pytest.mark.parametrize("mala", [False, True])
@pytest.mark.parametrize("n", RAGGED)
def test_ragged_relocation_is_transparent_and_a_permutation(n, mala):
    """Relocation on (per-step relocation, a full re-sort after every second step from step 0 on) against off: 12 steps of plain MLT, 12 of MALA at
    maxdepth 4, at chain counts that leave a remainder tile everywhere.  At three points: every chain in the same state, the counters equal, and the
    slot tables a permutation with chain_id the inverse of slot_of."""
    off, film0 = _off(n, mala)
    on, film1 = worker.run(n, mala, MALA_OPTS if mala else worker.PLAIN_OPTS, max_depth=4 if mala else 6)
    _check_transparent(n, mala, off, film0, on, film1)


SORTED_STEPS = 24


def _part1by1(x):
    out = np.zeros_like(x)
    for b in range(9):
        out |= ((x >> b) & 1) << (2 * b)
    return out


@pytest.mark.parametrize("n", RAGGED)
def test_slots_are_in_key_order_after_a_full_resort(n):
    """With a full re-sort after EVERY step the slots are, right after a step, in the order of the 24-bit key of relocate.hip FineKey:
        [63 - TechniqueKey(c, l) | Morton code of (screen0, screen1) * 512, 9 + 9 bits]          ascending (a stable radix sort)
    FineKey reads c and l from words 0 and 1 of the chain's contribution (summary columns 1, 2: meaningful for invalid states too) and screen0 /
    screen1 from words 1 and 2 of its current path buffer.  The summary reports those two path words among its primary samples, at columns
    16 + 2 l (l > 1) or 16 (l <= 1); its screenX / screenY (columns 10, 11) are the contribution's screen position, which for a state whose
    camera sub-path has a vertex (c >= 2) is that same pair (dpath.h: such contributions carry the path's own screenPos; c = 1 projects the light
    vertex instead).  So: the technique order is asserted for every slot, the Morton order for the valid rows with c >= 2, where columns 10, 11
    are checked to BE those path words."""
    # Every chain starts invalid and stays so until a large step of its own is accepted (a fifth of them per step here): after SORTED_STEPS steps more
    # than 90 % of the rows are valid.  The share is taken from a relocation-OFF run first, so it is a property of the set-up, not of the code under test.
    off = rel._run(False, False, n, SORTED_STEPS, worker.PLAIN_OPTS)[0][-1][0]
    usable = (off[:, 0] == 1) & (off[:, 1] >= 2)
    assert usable.sum() >= 0.9 * n, ("test set-up: too few valid rows with a camera vertex", usable.sum(), n)
    on, _ = worker.run(n, False, worker.PLAIN_OPTS, points=(SORTED_STEPS,), resort_every=1)
    s, st, rs, slot_of, chain_id = on[0]
    rel._same_states(off, s)
    _check_slots(slot_of, chain_id, n)
    c, l = s[:, 1].astype(np.int64), s[:, 2].astype(np.int64)
    tech = lc.slot_key(c, l)
    assert (np.diff(tech[chain_id]) >= 0).all(), "technique keys along the slots"
    assert rs["breaks"] == len(np.unique(tech)) - 1
    rows = (s[:, 0] == 1) & (c >= 2)
    assert np.array_equal(rows, usable)
    col = np.where(l > 1, 16 + 2 * l, 16)
    assert col[rows].max() + 1 < s.shape[1]
    idx = np.flatnonzero(rows)
    assert np.array_equal(s[idx, 10], s[idx, col[idx]]) and np.array_equal(s[idx, 11], s[idx, col[idx] + 1]), "screenX / screenY are not the path's screen0 / screen1"
    assert rows.sum() >= 0.9 * n, (rows.sum(), n)
    mx = np.clip(np.trunc(s[:, 10] * np.float32(512)).astype(np.int64), 0, 511)
    my = np.clip(np.trunc(s[:, 11] * np.float32(512)).astype(np.int64), 0, 511)
    fine = (tech << 18) | _part1by1(mx) | (_part1by1(my) << 1)
    in_slot_order = chain_id[rows[chain_id]]  # the chains of those rows, by slot: a subsequence of a sorted sequence is sorted
    bad = np.flatnonzero(np.diff(fine[in_slot_order]) < 0)
    assert not len(bad), (len(bad), bad[:5])
    assert len(np.unique(fine[in_slot_order])) > 0.5 * rows.sum()  # ... and the Morton part is not vacuous


@pytest.mark.parametrize("variant", ["LMC_RELOC_COOP=0", "LMC_RELOC_FINE=1"])
def test_shipped_move_variants(variant, tmp_path):
    """The lane-per-record move kernels (LMC_RELOC_COOP=0) and the per-step relocation by the fine key (LMC_RELOC_FINE=1): both are read from the
    environment once per process, so each runs the ragged plain-MLT render in a fresh process (tests/helpers/reloc_worker.py), one at a time."""
    name, value = variant.split("=")
    env = dict({k: v for k, v in os.environ.items() if k not in ("LMC_RELOC_COOP", "LMC_RELOC_FINE", "LMC_RELOCATE", "LMC_RESORT_EVERY", "LMC_RESORT_FIRST")}, **{name: value})
    out = str(tmp_path / "variant.npz")
    r = subprocess.run([sys.executable, os.path.join(gc.ROOT, "tests", "helpers", "reloc_worker.py"), out, ",".join(str(n) for n in RAGGED)], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:]
    d = np.load(out)
    for n in RAGGED:
        off, film0 = _off(n, False)
        on = [(d["summary_%d_%d" % (n, k)], json.loads(str(d["stats_%d_%d" % (n, k)])), json.loads(str(d["reloc_%d_%d" % (n, k)])), d["slot_of_%d_%d" % (n, k)],
               d["chain_id_%d_%d" % (n, k)]) for k in range(len(worker.POINTS))]
        _check_transparent(n, False, off, film0, on, d["film_%d" % n])
