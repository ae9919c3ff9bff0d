"""CPU tier: the references of tests/list_cases.py against brute-force loops on small random inputs, the checkers against outputs that are legal and
outputs that are subtly wrong, and each case generator's own claims.  Keeps the yardstick of tests/test_gpu_lists.py honest without a GPU."""
import numpy as np
import pytest

from tests import list_cases as lc


def test_technique_key_matches_its_definition():
    for c in range(0, 15):
        for l in range(0, 15):
            L = max(c + l - 1, 3)
            assert lc.technique_key(c, l) == min((L - 3) * 6 + min(l, 5), 63)
    keys = {int(lc.technique_key(c, l)) for c, l in lc.TECHNIQUES}
    assert len(keys) > 40 and max(keys) == 63 and min(keys) == 0  # the cases spread over the whole key range, the clamp included


# ---- scan
def test_scan_reference_and_cases():
    rng = np.random.default_rng(1)
    v = rng.integers(-50, 50, 300)
    run, brute = 0, []
    for x in v:
        run += int(x)
        brute.append(run)
    assert np.array_equal(lc.scan_ref(v), brute)
    sums_tiles = lambda n: (n + lc.SCAN_TILE - 1) // lc.SCAN_TILE  # tile sums are scanned in batches of 256
    assert [sums_tiles(n) for n in lc.SCAN_SIZES[8:]] == [256, 256, 257, 258, 514]  # one full batch; a second of 1 and 2; a third
    assert max(sums_tiles(n) for n in lc.SCAN_SIZES[:8]) == 2 and 2049 in lc.SCAN_SIZES
    for n in lc.SCAN_SIZES:
        for kind in lc.SCAN_INPUTS:
            v = lc.scan_input(kind, n)
            assert v.dtype == np.int32 and len(v) == n and v.min() >= 0 and v.max() <= 1500
            assert lc.scan_ref(v)[-1] < 2 ** 31
        t = lc.scan_input("tile_last", n)
        assert np.count_nonzero(t) == n // lc.SCAN_TILE and (np.flatnonzero(t) % lc.SCAN_TILE == lc.SCAN_TILE - 1).all()


# ---- radix sort
def test_radix_reference_and_cases():
    keys = np.random.default_rng(2).integers(0, 50, 200).astype(np.uint32)
    vals, out = lc.radix_ref(keys, 150)
    brute = sorted(range(150), key=lambda i: (int(keys[i]), i))  # stable = ties by index
    assert list(vals[:150]) == brute and list(out[:150]) == [int(keys[i]) for i in brute]
    assert (vals[150:] == lc.SENTINEL).all() and (out[150:] == lc.SENTINEL & 0xFFFFFFFF).all()
    assert {(n + lc.RS_TILE - 1) // lc.RS_TILE for n, _ in lc.RADIX_SIZES} >= {0, 1, 2, 3, 10}
    assert 256 * 10 > lc.SCAN_TILE  # 40000 keys: ten blocks, a digit histogram of two scan tiles
    for kind in lc.RADIX_KEYS:
        k = lc.radix_keys(kind, 5000)
        assert k.dtype == np.uint32 and k.max() < 1 << 24, kind
        digits = [(k >> (8 * b)) & 255 for b in range(3)]
        if kind == "all_equal":
            assert len(np.unique(k)) == 1 and np.array_equal(lc.radix_ref(k, 5000)[0], np.arange(5000))  # stability: the identity
        if kind == "two_values":
            assert len(np.unique(k)) == 2 and (k[::2] != k[1::2]).all()
        if kind == "descending":
            assert (np.diff(k.astype(np.int64)) < 0).all()
        if kind.startswith("byte"):
            b = int(kind[4])
            assert all((len(np.unique(digits[j])) == 1) == (j != b) for j in range(3)), kind
        if kind == "wave_distinct":
            assert all(len(np.unique(d[w : w + 64])) == 64 for d in digits for w in range(0, 4992, 64))
        if kind == "wave_same":
            assert all(len(np.unique(d[w : w + 64])) == 1 for d in digits for w in range(0, 4992, 64)) and k[0] != k[64]


# ---- sort by technique
def _legal_sort(next_kind, entries, rng):
    groups = {}
    for pos, e in enumerate(entries):
        groups.setdefault((int(next_kind[e]) >> 2, pos // lc.SORT_CHUNK), []).append(int(e))
    return np.array([e for g in sorted(groups) for e in rng.permutation(groups[g])], np.int64)


def test_sort_by_technique_checker():
    rng = np.random.default_rng(3)
    for count in lc.SORT_COUNTS:
        for single in (0, 1):
            nk, e = lc.sort_case(count, single)
            assert len(e) == count and len(np.unique(e)) == count and e.max(initial=0) < len(nk)
            keys = np.unique(nk[e] >> 2)
            assert len(keys) == (min(count, 1) if single else (64 if count >= 64 else len(keys)))
            out = _legal_sort(nk, e, rng)
            lc.check_sort_by_technique(nk, e, out)
            if count >= 2:
                bad = out.copy()
                bad[0] = bad[1]  # an entry twice, another lost
                with pytest.raises(AssertionError):
                    lc.check_sort_by_technique(nk, e, bad)
    nk, e = lc.sort_case(5000, 0)
    out = _legal_sort(nk, e, rng)
    k = nk[out] >> 2
    i = np.flatnonzero(k[:-1] != k[1:])[0]
    bad = out.copy()
    bad[[i, i + 1]] = bad[[i + 1, i]]  # two keys out of order
    with pytest.raises(AssertionError):
        lc.check_sort_by_technique(nk, e, bad)
    nk, e = lc.sort_case(5000, 1)  # one key: chunks 0, 1, 2 must follow each other
    out = _legal_sort(nk, e, rng)
    bad = out.copy()
    bad[[100, 3000]] = bad[[3000, 100]]
    with pytest.raises(AssertionError):
        lc.check_sort_by_technique(nk, e, bad)


# ---- build lists
def test_build_lists_reference_and_checker():
    rng = np.random.default_rng(4)
    for n in (257, 1025, 4099):
        for lean in lc.BUILD_LEAN:
            nk = lc.build_kinds("mix", n)
            k, counts = lc.build_lists_ref(nk, lean)
            for sp in range(4):
                legal = lc.build_lists_brute(nk, sp, lean, rng)
                assert np.array_equal(legal["step_kind"], k & 3) and np.array_equal(legal["counts"], counts)
                lc.check_build_lists(nk, sp, lean, legal)
                for name in ("large", "plain"):
                    cnt = int(legal["counts"][0 if name == "large" else 2])
                    bad = {f: np.array(v).copy() for f, v in legal.items()}
                    bad[name][[0, cnt - 1]] = bad[name][[cnt - 1, 0]]  # first and last entry swapped: never a legal order at these sizes
                    with pytest.raises(AssertionError):
                        lc.check_build_lists(nk, sp, lean, bad)
                bad = {f: np.array(v).copy() for f, v in legal.items()}
                bad["counts"][1] += 1
                with pytest.raises(AssertionError):
                    lc.check_build_lists(nk, sp, lean, bad)
    # sort_plain 3 is a STABLE partition: swapping two entries of one class must fail; sort_plain 1 leaves that order free
    nk = lc.build_kinds("plain_one_key", 1024)
    for sp, ok in ((1, True), (3, False), (0, False)):
        got = lc.build_lists_brute(nk, sp, 0)
        got["plain"][[3, 4]] = got["plain"][[4, 3]]
        if ok:
            lc.check_build_lists(nk, sp, 0, got)
        else:
            with pytest.raises(AssertionError):
                lc.check_build_lists(nk, sp, 0, got)


def test_build_lists_cases_claims():
    assert 4099 % 4 == 3 and 4099 > 4 * 1024  # a tail of three chains beside the uchar4 loads, five tiles
    assert (lc.build_kinds("all_large", 1024) & 3 == lc.NEXT_LARGE).all()  # 1024 in one 16-bit field of the packed counters
    assert not lc.build_kinds("all_done", 1024).any()
    p = lc.build_kinds("plain_one_key", 1024)
    assert (p & 3 == lc.NEXT_PLAIN).all() and len(np.unique(p >> 2)) == 1
    m = lc.build_kinds("mix", 4099)
    gen = m[(m & 3) == lc.NEXT_GENERIC] >> 2
    assert ((gen % 6) > 1).sum() > 100 and ((gen % 6) <= 1).sum() > 100 and {0, 1, 2, 3} == set(m & 3)
    k0, c0 = lc.build_lists_ref(m, 0)
    k1, c1 = lc.build_lists_ref(m, lc.LEAN_ALL_READY)
    k2, c2 = lc.build_lists_ref(m, lc.LEAN_ALL_READY | 1 << 31)
    assert np.array_equal(k0, m) and c1[1] == 0 and c1[2] == c0[1] + c0[2]  # all ready: every generic entry promoted
    assert c2[1] == ((gen % 6) > 1).sum() and c2[2] == c0[2] + ((gen % 6) <= 1).sum()  # bit 31: only those without a longer light sub-path
    assert (k2 >> 2 == m >> 2).all()


# ---- bins compact
def test_bins_checker_and_cases():
    rng = np.random.default_rng(5)
    for kind in lc.BINS_CASES:
        for length in lc.BINS_LENGTHS:
            bin_of, count, e = lc.bins_case(kind, length)
            assert len(e) == length and len(np.unique(e)) == length and count.sum() <= length and len(count) == lc.BINS
            b = bin_of[e]
            if kind == "one_bin":
                assert count[117] == length and count.sum() == length
            if kind == "every_bin" and length == 1000:
                assert (count > 0).all()
            if kind == "some_absent" and length >= 63:
                assert 0 < (b < 0).sum() < length and count.sum() == (b >= 0).sum()
            items = np.full(len(bin_of), lc.SENTINEL, np.int64)
            start = np.cumsum(count) - count
            for bb in range(lc.BINS):
                members = [int(x) for x in e if bin_of[x] == bb]
                items[start[bb] : start[bb] + len(members)] = rng.permutation(members) if members else []
            lc.check_bins_compact(bin_of, count, e, items, start)
            if count.sum() >= 2 and (count > 0).sum() >= 2:
                bad = items.copy()
                total = int(count.sum())
                bad[[0, total - 1]] = bad[[total - 1, 0]]  # two entries of different bins swapped
                with pytest.raises(AssertionError):
                    lc.check_bins_compact(bin_of, count, e, bad, start)
            if count.sum() >= 2:
                bad = items.copy()
                bad[0] = bad[1]
                with pytest.raises(AssertionError):
                    lc.check_bins_compact(bin_of, count, e, bad, start)


# ---- split list
def test_split_reference():
    for parts in lc.SPLIT_PARTS:
        assert {64 * parts, 64 * parts + 1} <= set(lc.split_totals(parts))
        for total in lc.split_totals(parts):
            e = np.random.default_rng(total).integers(0, 10 ** 6, total).astype(np.int32)
            stride = lc.split_stride(total, parts)
            sub, cnt = lc.split_ref(e, parts, stride)
            brute = [[] for _ in range(parts)]
            for g in range(0, total, 64):  # groups of 64 dealt round robin
                brute[(g // 64) % parts] += list(e[g : g + 64])
            for h in range(parts):
                assert cnt[h] == len(brute[h]) and list(sub[h, : cnt[h]]) == brute[h] and (sub[h, cnt[h] :] == lc.SENTINEL).all()
                assert stride >= cnt[h] + 6  # the margin behind the longest part
            assert cnt.sum() == total


# ---- cache push
def test_push_reference_and_cases():
    for n in lc.PUSH_SIZES:
        for scrambled in (0, 1):
            d, x, so, init = lc.push_case("cut_dim6", n, scrambled)
            rows, w, counts, after = lc.push_ref(d, x, so, init)
            assert (d == 6).all() and init[0] == 2990 and counts[0] == min(3000, 2990 + n) and not after.any()
            chain_slot = np.arange(n) if so is None else so
            kept = min(n, 10)
            assert np.array_equal(rows[0, 1, 2990 : 2990 + kept, :6], x.view(np.uint32)[chain_slot[:kept], 12:18])  # v1 of the first chains, in chain order
            assert np.array_equal(w[0, 2990 : 2990 + kept], x.view(np.uint32)[chain_slot[:kept], 36])
            assert (rows[0, :, : 2990] == lc.UNTOUCHED_BITS).all() and (rows[0, :, :, 6:] == lc.UNTOUCHED_BITS).all() and (rows[1:] == lc.UNTOUCHED_BITS).all()
            d, x, so, init = lc.push_case("one_tile_one_dim", n, scrambled)
            by_chain = d[chain_slot]
            assert (by_chain[:1024] == 8).all() and not by_chain[1024:].any()  # 1024 pushes of one dim in one 1024-chain tile (when there are that many)
            d, x, so, init = lc.push_case("mixed", n, scrambled)
            rows, w, counts, after = lc.push_ref(d, x, so, init)
            valid = np.isin(d, lc.CACHE_DIMS)
            assert not after[valid].any() and np.array_equal(after[~valid], d[~valid])  # cleared for the consumed chains only
            for s, dim in enumerate(lc.CACHE_DIMS):
                assert counts[s] == min(3000, init[s] + (d == dim).sum())
            if n >= 1023:
                assert valid.sum() > 100 and (~valid & (d != 0)).sum() > 100 and set(lc.CACHE_DIMS) <= set(d)
    assert all(dim % 2 or dim < 6 or dim > 12 for dim in lc.PUSH_INVALID_DIMS)


# ---- relocation plan
def test_reloc_reference_and_cases():
    for n in lc.RELOC_SIZES[:-1] + (2 * 1024 + 7,):
        for kind in lc.RELOC_CASES:
            case = lc.reloc_case(kind, n)
            key = lc.slot_key(case["c"], case["l"])
            for wgo in (False, True):
                mem = lc.reloc_members(case, wgo)
                brute = [i for i in range(n) if case["step_kind"][i] == 1 and int(key[i]) != int(case["placed_key"][i]) and not (wgo and case["flags"][i] & 2)]
                assert list(mem) == brute
                count, members, srt = lc.reloc_plan_ref(case, wgo, n, 2)
                M = len(brute)
                assert list(count) == [M, 2] and list(members[:M]) == brute and (members[M:] == lc.SENTINEL).all() and (srt[M:] == lc.SENTINEL).all()
                assert list(srt[:M]) == sorted(range(M), key=lambda p: (int(key[brute[p]]), p))
                if M:
                    assert list(lc.reloc_plan_ref(case, wgo, M - 1, 2)[0]) == [0, 3] and list(lc.reloc_plan_ref(case, wgo, 0, 3)[0]) == [0, 4]
                    assert list(lc.reloc_plan_ref(case, wgo, M, 2)[0]) == [M, 2]
            M = len(lc.reloc_members(case, False))
            if kind == "nobody":
                assert M == 0
            if kind in ("everybody", "one_key"):
                assert M == n and (case["placed_key"] == lc.NEVER_PLACED).all()
            if kind == "one_key":
                assert len(np.unique(key)) == 1
            if kind == "all_techniques" and n >= 1000:
                assert len(np.unique(key)) > 40 and 0.3 * n < M < 0.7 * n
            if kind == "gauss" and n >= 1000:
                assert 0 < len(lc.reloc_members(case, True)) < M
            if kind == "mixed_kinds" and n >= 1000:
                assert set(case["step_kind"]) == {0, 1, 2, 3} and 0 < M < 0.4 * n
    assert (lc.RELOC_SIZES[-1] + lc.RELOC_TILE - 1) // lc.RELOC_TILE == 66  # more than 64 tiles: the tile scan's second batch
