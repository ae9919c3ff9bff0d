"""References and cases for the bookkeeping launches the step kernels run on (device/kernels.hip, device/relocate.hip; probes in include/lmc_abi.h):
the tiled inclusive scan, the 24-bit radix sort, the work lists and their counting sorts, the stage bins, the list split, the cache-push pack and
the plan of a relocation.  Plain NumPy, written from the contracts in the kernels' comments, not from their loop structure.  Everything is an
integer or a copied word, so every comparison is exact.  Where the device leaves an order to LDS or global atomics, the check says what is free
and pins the rest.  tests/test_list_cases.py checks these references against brute-force loops and each generator's own claims without a GPU;
tests/test_gpu_lists.py runs the device against them."""
import numpy as np

SENTINEL = -0x5A5A5A5B  # what a probe's integer output holds where the launch wrote nothing (include/lmc_abi.h LMC_PROBE_SENTINEL)
UNTOUCHED_BITS = 0x7FC0BEEF  # ... and a float output
NEXT_DONE, NEXT_LARGE, NEXT_GENERIC, NEXT_PLAIN = 0, 1, 2, 3  # dchain.h NEXT_*
F_GAUSS = 2
SCAN_TILE, SORT_CHUNK, RELOC_TILE, RS_TILE = 2048, 2048, 1024, 4096
BINS, CACHE_ROWS, CACHE_DIMS = 336, 3000, (6, 8, 10, 12)
NEVER_PLACED = 0xFFFFFFFF


def technique_key(c, l):
    """dchain.h TechniqueKey: path length first (3 and shorter together), then the light sub-path length (5 and longer together); 6 bits"""
    c, l = np.asarray(c, np.int64), np.asarray(l, np.int64)
    return np.minimum((np.maximum(c + l - 1, 3) - 3) * 6 + np.minimum(l, 5), 63)


def slot_key(c, l):
    """relocate.hip SlotKey: longest paths first along the slots"""
    return 63 - technique_key(c, l)


# ------------------------------------------------------------------------------------------------ scan
SCAN_SIZES = (1, 7, 8, 9, 2047, 2048, 2049, 4096, 2048 * 256 - 1, 2048 * 256, 2048 * 256 + 1, 2048 * 257 + 5, 2048 * 513 + 3)
SCAN_INPUTS = ("ones", "random", "tile_last")


def scan_input(kind, n):
    """ones; random in [0, 1500] (the total of the longest case stays below 2^31); zero except the last element of every full 2048-tile"""
    if kind == "ones":
        return np.ones(n, np.int32)
    if kind == "random":
        return np.random.default_rng(n).integers(0, 1501, n).astype(np.int32)
    v = np.zeros(n, np.int32)
    last = np.arange(SCAN_TILE - 1, n, SCAN_TILE)
    v[last] = 1 + last // SCAN_TILE % 7
    return v


def scan_ref(v):
    out = np.cumsum(np.asarray(v, np.int64))
    assert len(out) and out[-1] < 2 ** 31 and out.min() >= -2 ** 31, "scan case overflows int32"
    return out


# ------------------------------------------------------------------------------------------------ radix sort
RADIX_SIZES = [(n, n) for n in (1, 63, 64, 65, 4095, 4096, 4097, 5000, 12288, 40000)] + [(5000, 8192), (0, 8192), (4096, 8192)]  # (n, n_max)
RADIX_KEYS = ("random", "all_equal", "two_values", "descending", "byte0", "byte1", "byte2", "wave_distinct", "wave_same")


def radix_keys(kind, n_max):
    """n_max keys of 24 bits.  byteB: the keys differ in byte B only; wave_distinct: every 64 consecutive keys have 64 different digits in every
    pass; wave_same: every 64 consecutive keys share one digit in every pass, neighbouring groups differ"""
    i = np.arange(n_max, dtype=np.int64)
    rng = np.random.default_rng(n_max + 17)
    if kind == "random":
        k = rng.integers(0, 1 << 24, n_max)
    elif kind == "all_equal":
        k = np.full(n_max, 0xABCDEF)
    elif kind == "two_values":
        k = np.where(i & 1, 0x000100, 0xFF00FF)
    elif kind == "descending":
        k = (1 << 24) - 1 - i * 3
    elif kind.startswith("byte"):
        b = int(kind[4])
        k = (0x5A3C96 & ~(0xFF << (8 * b))) | (rng.integers(0, 256, n_max) << (8 * b))
    elif kind == "wave_distinct":
        k = ((i * 37 + i // 64) % 64) * 0x030201 % (1 << 24)
    else:
        k = (i // 64 * 89 % 256) * 0x010101
    return k.astype(np.uint32)


def radix_ref(keys, n):
    """(vals, keys out): the stable ascending order of the first n keys; entries from n on keep the sentinel"""
    keys = np.asarray(keys, np.uint32)
    order = np.argsort(keys[:n], kind="stable")
    vals, out = np.full(len(keys), SENTINEL, np.int32), np.full(len(keys), SENTINEL & 0xFFFFFFFF, np.uint32)
    vals[:n], out[:n] = order, keys[:n][order]
    return vals, out


# ------------------------------------------------------------------------------------------------ sort by technique
SORT_COUNTS = (0, 1, 255, 256, 2047, 2048, 2049, 5000)


def sort_case(count, single_key):
    """(next_kind[n_chains], entries[count]): distinct chains in a scrambled order; keys over all 64 values or one"""
    rng = np.random.default_rng(count * 2 + single_key)
    n_chains = count + 37
    entries = rng.permutation(n_chains)[:count].astype(np.int32)
    key = np.full(n_chains, 41) if single_key else rng.integers(0, 64, n_chains)
    if not single_key and count >= 64:
        key[entries[rng.permutation(count)[:64]]] = np.arange(64)  # all 64 keys really occur
    next_kind = ((key << 2) | NEXT_GENERIC).astype(np.uint8)
    return next_kind, entries


def check_sort_by_technique(next_kind, entries, out):
    """A permutation of the entries; keys non-decreasing; inside a key the entries of 2048-chunk b before those of chunk b + 1; the order inside a
    (chunk, key) group is free (LDS atomics)."""
    entries, out = np.asarray(entries, np.int64), np.asarray(out, np.int64)
    assert len(out) == len(entries)
    assert np.array_equal(np.sort(out), np.sort(entries)), "not a permutation of the list"
    assert len(np.unique(entries)) == len(entries), "case: the chains of a list are distinct"
    chunk = np.full(len(next_kind), -1, np.int64)
    chunk[entries] = np.arange(len(entries)) // SORT_CHUNK
    rank = (np.asarray(next_kind, np.int64)[out] >> 2) * (len(entries) // SORT_CHUNK + 1) + chunk[out]
    assert (np.diff(rank) >= 0).all(), "keys, then chunks inside a key, must be non-decreasing"


# ------------------------------------------------------------------------------------------------ build lists
BUILD_SIZES = (1, 3, 255, 256, 257, 1023, 1024, 1025, 4099)
BUILD_KINDS = ("mix", "all_large", "all_done", "plain_one_key")
LEAN_ALL_READY = sum(1 << (2 * L) for L in range(3, 14))  # bit 2 L: the cache of path length L (dim 2 L) is ready and shallow
BUILD_LEAN = (0, LEAN_ALL_READY, LEAN_ALL_READY | 1 << 31)


def build_kinds(kind, n):
    rng = np.random.default_rng(n + 5)
    if kind == "all_large":
        return np.full(n, NEXT_LARGE | (7 << 2), np.uint8)
    if kind == "all_done":
        return np.zeros(n, np.uint8)
    if kind == "plain_one_key":
        return np.full(n, NEXT_PLAIN | (14 << 2), np.uint8)
    k = rng.integers(0, 4, n) | (rng.integers(0, 64, n) << 2)
    k[(k & 3) == 0] = 0  # a finished chain carries no key
    return k.astype(np.uint8)


def build_lists_ref(next_kind, lean_dims):
    """(effective next_kind, counts[3]): a generic entry whose cache became ready (lean_dims bit 2 * path length) is a plain one now -- unless bit 31
    is set (lean launch without light sub-paths) and its light sub-path index key % 6 is above 1.  step_kind = effective kind & 3."""
    k = np.asarray(next_kind, np.int64).copy()
    key = k >> 2
    ready = (lean_dims >> (2 * (3 + key // 6))) & 1
    lightless_only = (lean_dims >> 31) & 1
    promote = ((k & 3) == NEXT_GENERIC) & (ready == 1) & ~((lightless_only == 1) & (key % 6 > 1))
    k[promote] |= NEXT_PLAIN
    return k, np.array([((k & 3) == f).sum() for f in (NEXT_LARGE, NEXT_GENERIC, NEXT_PLAIN)], np.int64)


def _tile_runs(out, tile):
    """[(tile, entries of its run)], asserting that every tile occupies ONE contiguous run"""
    runs, t = [], out // tile
    cut = np.flatnonzero(np.diff(t)) + 1
    for a, b in zip(np.r_[0, cut], np.r_[cut, len(out)]):
        if b > a:
            runs.append((int(t[a]), out[a:b]))
    assert len({r[0] for r in runs}) == len(runs), "a tile's entries are split over several runs"
    return runs


def check_build_lists(next_kind, sort_plain, lean_dims, got, with_step_kind=True):
    """got: dict(large, generic, plain, counts, step_kind).  counts and step_kind exact; every list = the concatenation of per-tile segments (tile
    1024 chains, 256 for sort_plain 2), one contiguous run each, tiles in any order (a global atomic); inside a run: large and generic ascending;
    plain ascending (0), stably partitioned short class first (3), grouped by key ascending with free order inside a key (1, 2)."""
    k, counts = build_lists_ref(next_kind, lean_dims)
    n, tile = len(k), 256 if sort_plain == 2 else 1024
    assert np.array_equal(np.asarray(got["counts"], np.int64), counts), ("counts", got["counts"], counts)
    if with_step_kind:
        assert np.array_equal(np.asarray(got["step_kind"], np.int64), k & 3), "step_kind"
    for f, name in ((NEXT_LARGE, "large"), (NEXT_GENERIC, "generic"), (NEXT_PLAIN, "plain")):
        cnt, lst = int(counts[f - 1]), np.asarray(got[name], np.int64)
        assert len(lst) == n and (lst[cnt:] == SENTINEL).all(), name + ": written beyond its count"
        want = np.flatnonzero((k & 3) == f)
        seen = 0
        for t, run in _tile_runs(lst[:cnt], tile):
            exp = want[(want >= t * tile) & (want < (t + 1) * tile)]
            seen += len(run)
            if name != "plain" or sort_plain == 0:
                assert np.array_equal(run, exp), (name, t, "ascending chains of the tile")
            elif sort_plain == 3:
                long_path = (k[exp] >> 2) // 6 >= 2
                assert np.array_equal(run, np.r_[exp[~long_path], exp[long_path]]), (name, t, "stable two-class partition")
            else:
                assert np.array_equal(np.sort(run), exp) and (np.diff(k[run] >> 2) >= 0).all(), (name, t, "grouped by key")
        assert seen == cnt


def build_lists_brute(next_kind, sort_plain, lean_dims, rng=None):
    """a brute-force legal output (tiles in a shuffled order when rng is given): what check_build_lists must accept"""
    k = [int(x) for x in next_kind]
    for i, x in enumerate(k):
        key = x >> 2
        if x & 3 == NEXT_GENERIC and (lean_dims >> (2 * (3 + key // 6))) & 1 and not ((lean_dims >> 31) & 1 and key % 6 > 1):
            k[i] = x | NEXT_PLAIN
    n, tile = len(k), 256 if sort_plain == 2 else 1024
    tiles = list(range((n + tile - 1) // tile))
    got = dict(step_kind=np.array([x & 3 for x in k], np.uint8), counts=np.zeros(3, np.int32))
    for f, name in ((NEXT_LARGE, "large"), (NEXT_GENERIC, "generic"), (NEXT_PLAIN, "plain")):
        order = list(rng.permutation(tiles)) if rng is not None else tiles
        lst = []
        for t in order:
            seg = [i for i in range(t * tile, min(n, (t + 1) * tile)) if k[i] & 3 == f]
            if name == "plain" and sort_plain == 3:
                seg = [i for i in seg if (k[i] >> 2) // 6 < 2] + [i for i in seg if (k[i] >> 2) // 6 >= 2]
            elif name == "plain" and sort_plain in (1, 2):
                seg = sorted(seg if rng is None else list(rng.permutation(seg)), key=lambda i: k[i] >> 2)
            lst += seg
        got["counts"][f - 1] = len(lst)
        got[name] = np.array(lst + [SENTINEL] * (n - len(lst)), np.int32)
    return got


# ------------------------------------------------------------------------------------------------ bins compact
BINS_LENGTHS = (0, 1, 63, 64, 65, 1000)
BINS_GRIDS = (1, 3, 40)  # 40 blocks of 64: more than a list of 1000 needs
BINS_CASES = ("one_bin", "every_bin", "some_absent")


def bins_case(kind, length):
    """(bin_of[N], count[BINS], entries[length]); some_absent: a third of the list's chains have bin_of = -1 and take no part"""
    rng = np.random.default_rng(length + 3)
    n = 1200
    entries = rng.permutation(n)[:length].astype(np.int32)
    bin_of = np.full(n, -1, np.int32)
    if kind == "one_bin":
        bin_of[entries] = 117
    elif kind == "every_bin":
        bin_of[entries] = np.arange(length) * 5 % BINS
    else:
        bin_of[entries] = np.where(rng.random(length) < 1 / 3, -1, rng.integers(0, BINS, length))
    b = bin_of[entries]
    return bin_of, np.bincount(b[b >= 0], minlength=BINS).astype(np.int32), entries


def check_bins_compact(bin_of, count, entries, items, start):
    """start = exclusive prefix of count; items[start[b] : start[b] + count[b]] holds, in any order, the list's chains of bin b; nothing beyond the total"""
    count, items = np.asarray(count, np.int64), np.asarray(items, np.int64)
    ex = np.cumsum(count) - count
    assert np.array_equal(np.asarray(start, np.int64), ex), "start"
    total = int(count.sum())
    assert (items[total:] == SENTINEL).all(), "written beyond the total"
    b = np.asarray(bin_of, np.int64)[np.asarray(entries, np.int64)]
    order = np.argsort(b[b >= 0], kind="stable")
    want = np.asarray(entries, np.int64)[b >= 0][order]  # by bin; inside a bin compare as sets
    got_bin = np.repeat(np.arange(BINS), count)
    assert np.array_equal(np.asarray(bin_of, np.int64)[items[:total]], got_bin), "an entry sits in another bin's range"
    assert np.array_equal(np.sort(items[:total] + got_bin * (1 << 32)), np.sort(want + b[b >= 0][order] * (1 << 32))), "bin contents"


# ------------------------------------------------------------------------------------------------ split list
SPLIT_PARTS = (1, 2, 3, 4)
SPLIT_GRIDS = (1, 7)


def split_totals(parts):
    return (0, 1, 63, 64, 65, 127, 128, 64 * parts, 64 * parts + 1, 1000)


def split_stride(total, parts):
    """what a part can receive (ceil(groups / parts) groups of 64) plus a margin that must stay untouched"""
    return ((total + 63) // 64 + parts - 1) // parts * 64 + 70


def split_ref(entries, parts, stride):
    """Groups of 64 entries go round robin over the parts; (sub[parts, stride], sub_count[parts]), the sentinel where nothing lands"""
    e = np.asarray(entries, np.int32)
    j = np.arange(len(e))
    g = j // 64
    sub = np.full((parts, stride), SENTINEL, np.int32)
    sub[g % parts, g // parts * 64 + j % 64] = e
    return sub, np.bincount(g % parts, minlength=parts).astype(np.int32)


# ------------------------------------------------------------------------------------------------ cache push
PUSH_SIZES = (1, 1023, 1024, 1025, 5000)
PUSH_CASES = ("cut_dim6", "one_tile_one_dim", "mixed")
PUSH_INVALID_DIMS = (-2, 2, 4, 5, 7, 9, 11, 13, 14, 24)


def push_case(kind, n, scrambled):
    """(push_dim[n] by slot, push_data[n, 37], slot_of or None, initial_counts[4]).
    cut_dim6: every chain pushes dim 6 onto 2990 rows (the cut at 3000 and the saturating count); one_tile_one_dim: the first 1024 chain IDS (one
    tile of the pack) all push dim 8; mixed: the four dims, pending-free chains and invalid dims."""
    rng = np.random.default_rng(n * 3 + scrambled)
    slot_of = rng.permutation(n).astype(np.int32) if scrambled else None
    by_chain = np.zeros(n, np.int32)
    init = np.zeros(4, np.int32)
    if kind == "cut_dim6":
        by_chain[:], init[0] = 6, 2990
    elif kind == "one_tile_one_dim":
        by_chain[:1024], init[:] = 8, (5, 100, 2999, 3000)
    else:
        by_chain[:] = rng.choice(np.r_[0, 0, CACHE_DIMS, CACHE_DIMS, PUSH_INVALID_DIMS], n)
        init[:] = (0, 2500, 2999, 17)
    push_dim = np.zeros(n, np.int32)
    push_dim[slot_of if scrambled else np.arange(n)] = by_chain
    data = rng.random((n, 37), dtype=np.float32)
    return push_dim, data, slot_of, init


def push_ref(push_dim, data, slot_of, initial_counts):
    """Rows appended in chain-id order per dim (the chain's slot through slot_of), cut at 3000 rows; counts saturate at 3000; push_dim cleared for the
    consumed chains only (a dim that is odd, below 6 or above 12 is ignored and stays).  rows [4, 3, 3000, 12] / weights [4, 3000] as uint32 bits."""
    n = len(push_dim)
    rows = np.full((4, 3, CACHE_ROWS, 12), UNTOUCHED_BITS, np.uint32)
    w = np.full((4, CACHE_ROWS), UNTOUCHED_BITS, np.uint32)
    bits = np.ascontiguousarray(data, np.float32).view(np.uint32)
    after, fill = np.asarray(push_dim, np.int32).copy(), [int(x) for x in initial_counts]
    for chain in range(n):
        i = chain if slot_of is None else int(slot_of[chain])
        dim = int(push_dim[i])
        if dim < 6 or dim > 12 or dim % 2:
            continue
        s = (dim - 6) // 2
        if fill[s] < CACHE_ROWS:
            for a in range(3):
                rows[s, a, fill[s], :dim] = bits[i, 12 * a : 12 * a + dim]
            w[s, fill[s]] = bits[i, 36]
        fill[s] += 1
        after[i] = 0
    return rows, w, np.minimum(fill, CACHE_ROWS).astype(np.int32), after


# ------------------------------------------------------------------------------------------------ relocation plan
RELOC_SIZES = (1, 64, 1000, 1024, 1025, 5000, 65 * 1024 + 7)
RELOC_CASES = ("nobody", "everybody", "one_key", "all_techniques", "gauss", "mixed_kinds")
TECHNIQUES = [(c, l) for c in range(1, 15) for l in range(0, 14) if 3 <= c + l <= 14]  # path length 13 reaches the clamp at key 63


def reloc_case(kind, n):
    """dict(step_kind, c, l, flags, placed_key).  nobody: every slot already placed under its key; everybody: nothing placed yet (the first relocation);
    one_key: one technique, nothing placed; all_techniques: every (c, l), half the slots placed under their key; gauss: as all_techniques with F_GAUSS on
    a third of the chains; mixed_kinds: step kinds other than large on half of them."""
    rng = np.random.default_rng(n + len(kind))
    t = np.array(TECHNIQUES)[rng.integers(0, len(TECHNIQUES), n)]
    if kind == "one_key":
        t[:] = (3, 2)
    c, l = t[:, 0].astype(np.int32), t[:, 1].astype(np.int32)
    key = slot_key(c, l).astype(np.uint32)
    step_kind = np.full(n, NEXT_LARGE, np.uint8)
    flags = (rng.integers(0, 1024, n) & ~F_GAUSS).astype(np.int32)
    if kind == "nobody":
        placed = key.copy()
    elif kind in ("everybody", "one_key"):
        placed = np.full(n, NEVER_PLACED, np.uint32)
    else:
        placed = np.where(rng.random(n) < 0.5, key, np.where(rng.random(n) < 0.5, NEVER_PLACED, (key + 1) % 64)).astype(np.uint32)
    if kind == "gauss":
        flags |= np.where(rng.random(n) < 1 / 3, F_GAUSS, 0).astype(np.int32)
    if kind == "mixed_kinds":
        step_kind = rng.choice(np.array([NEXT_DONE, NEXT_LARGE, NEXT_LARGE, NEXT_GENERIC, NEXT_PLAIN], np.uint8), n)
    return dict(step_kind=step_kind, c=c, l=l, flags=flags, placed_key=placed)


def reloc_members(case, without_gaussian_only):
    """relocate.hip MemberKey: the slots whose chain ran a LARGE step and whose key differs from the one the slot was placed under (and, for H2MC
    renders, that hold no Gaussian), ascending"""
    m = (case["step_kind"] == NEXT_LARGE) & (slot_key(case["c"], case["l"]) != case["placed_key"])
    if without_gaussian_only:
        m &= (case["flags"] & F_GAUSS) == 0
    return np.flatnonzero(m)


def reloc_plan_ref(case, without_gaussian_only, capacity, skipped_before):
    """(count[2], members[N], sorted[N]): members ascending; sorted = the stable order of the members' keys; count[0] = the member count, or 0 with
    count[1] = skipped_before + 1 when it exceeds the capacity (the lists are built either way); the sentinel beyond the members"""
    n = len(case["c"])
    mem = reloc_members(case, without_gaussian_only)
    members, srt = np.full(n, SENTINEL, np.int32), np.full(n, SENTINEL, np.int32)
    members[: len(mem)] = mem
    srt[: len(mem)] = np.argsort(slot_key(case["c"], case["l"])[mem], kind="stable")
    count = [len(mem), skipped_before] if len(mem) <= capacity else [0, skipped_before + 1]
    return np.array(count, np.int32), members, srt
