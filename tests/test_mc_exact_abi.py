"""CPU tier: the exact mc film's surface (include/lmc_abi.h "Exact mc film": lmc_mc_accumulate / _coverage / _read_fixed / _overflow / _save / _load /
_file_info, lmc_group_mc_render, the Python bindings), the host-side bookkeeping of host/mcfilm.cpp (coverage arithmetic, launch cuts, the state
file) -- through the library and through a stand-alone sanitizer build -- and the fixed-point CPU oracle tests/helpers/mc_oracle_fx.cpp, pinned
to the float oracle of tests/test_mc_abi.py.  The device side is checked against it in tests/test_gpu_mc_exact.py."""
import ctypes
import functools
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from tests import gpu_checks as gc
from tests._orc import P
from tests.test_gpu_mc import _film_close
from tests.test_mc_abi import oracle_mc

HELPER_SRC = os.path.join(gc.ROOT, "tests", "helpers", "mc_oracle_fx.cpp")
HELPER_SO = os.path.join(gc.ROOT, "tests", "helpers", "libmc_oracle_fx.so")
MCFILM_SRC = os.path.join(gc.ROOT, "langevin-mcmc_amd", "csrc", "host", "mcfilm.cpp")
MCFILM_MAIN = os.path.join(gc.ROOT, "tests", "helpers", "mcfilm_main.cpp")

NEW_SYMBOLS = ("lmc_mc_accumulate", "lmc_mc_coverage", "lmc_mc_read_fixed", "lmc_mc_overflow", "lmc_group_mc_render", "lmc_group_mc_accumulate", "lmc_mc_save",
               "lmc_mc_load", "lmc_mc_file_info", "lmc_mc_coverage_probe", "lmc_mc_chunks_probe")


def mc_oracle_fx():
    """tests/helpers/mc_oracle_fx.cpp built like tests/test_mc_abi.py builds its helper (the oracle's flags: no contraction, -mfma)"""
    gc.oracle_lib()  # builds the oracle if needed
    deps = [HELPER_SRC, gc.ORACLE_SO]
    if not os.path.exists(HELPER_SO) or os.path.getmtime(HELPER_SO) < max(os.path.getmtime(f) for f in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-mfma",
                               "-I" + os.path.join("langevin-mcmc_amd", "csrc", "host"), HELPER_SRC, "-o", HELPER_SO,
                               "-L" + os.path.join(gc.ROOT, "oracle"), "-llmc_oracle", "-Wl,-rpath,$ORIGIN/../../oracle"], cwd=gc.ROOT)
    L = ctypes.CDLL(HELPER_SO)
    L.mc_oracle_fx_render.restype = ctypes.c_int
    L.mc_oracle_fx_render.argtypes = [ctypes.c_char_p] + [ctypes.c_int] * 8 + [ctypes.c_longlong, ctypes.c_longlong, ctypes.c_int, ctypes.c_void_p,
                                                                                ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int]
    return L


@functools.lru_cache(maxsize=None)
def _oracle_mc_fx(xml, spp, force_diffuse, max_depth, width, height, seed_offset, min_depth, bidir, streams, literal):
    L = mc_oracle_fx()
    begin, end = (0, -1) if streams is None else streams
    out = np.zeros((height, width, 3), np.int64)
    counts = np.zeros(3, np.int64)
    err = ctypes.create_string_buffer(512)
    rc = L.mc_oracle_fx_render(xml.encode(), force_diffuse, max_depth, width, height, seed_offset, min_depth, int(bidir), spp, begin, end, int(literal),
                               P(out), P(counts), err, 512)
    assert rc == 0, err.value.decode()
    out.setflags(write=False)
    return out, int(counts[0]), int(counts[1]), int(counts[2])


def oracle_mc_fx(xml, spp, force_diffuse=1, max_depth=6, width=64, height=48, seed_offset=0, min_depth=-1, bidir=True, streams=None, literal=False):
    """(words int64 [H, W, 3], unweighted, unit 2^-32; paths traced; contributions counted; contributions dropped by the range rule) of the
    fixed-point oracle.  Computed once per argument set and shared (the array is read-only)."""
    return _oracle_mc_fx(xml, int(spp), int(force_diffuse), int(max_depth), int(width), int(height), int(seed_offset), int(min_depth), bool(bidir),
                         None if streams is None else (int(streams[0]), int(streams[1])), bool(literal))


def words_to_float(words, spp):
    """lmc_mc_read's conversion"""
    return np.float32(np.float64(words) * 2.0 ** -32 / spp)


# ---------------------------------------------------------------------------------------------- surface
def test_exact_mc_entry_points_are_declared_exported_and_bound():
    hdr = open(os.path.join(gc.ROOT, "include", "lmc_abi.h")).read()
    assert re.search(r"int\s+lmc_mc_accumulate\s*\(\s*lmc_ctx\s*\*\s*ctx\s*,\s*int\s+spp\s*,\s*long long\s+stream_begin\s*,\s*long long\s+stream_end\s*\)\s*;", hdr)
    assert re.search(r"int\s+lmc_mc_coverage\s*\(\s*lmc_ctx\s*\*\s*ctx\s*,\s*long long\s*\*\s*ranges\s*,\s*int\s+cap\s*\)\s*;", hdr)
    assert re.search(r"int\s+lmc_mc_read_fixed\s*\(\s*lmc_ctx\s*\*\s*ctx\s*,\s*long long\s*\*\s*words\s*\)\s*;", hdr)
    assert re.search(r"int\s+lmc_mc_overflow\s*\(\s*lmc_ctx\s*\*\s*ctx\s*,\s*long long\s*\*\s*n\s*\)\s*;", hdr)
    assert re.search(r"int\s+lmc_group_mc_render\s*\(\s*lmc_ctx\s*\*\*\s*ctxs\s*,\s*int\s+n\s*,\s*int\s+spp\s*,\s*long long\s+stream_begin\s*,\s*long long\s+stream_end\s*\)\s*;", hdr)
    assert re.search(r"int\s+lmc_mc_save\s*\(\s*lmc_ctx\s*\*\s*ctx\s*,\s*const char\s*\*\s*path\s*\)\s*;", hdr)
    assert re.search(r"int\s+lmc_mc_load\s*\(\s*lmc_ctx\s*\*\s*ctx\s*,\s*const char\s*\*\s*path\s*\)\s*;", hdr)
    assert re.search(r"long long\s+lmc_mc_file_info\s*\(\s*const char\s*\*\s*path\s*,\s*char\s*\*\s*json\s*,\s*long long\s+cap\s*\)\s*;", hdr)
    assert '"mc_film_exact"' in hdr and '"mc_launch_streams"' in hdr and '"mc_launches"' in hdr
    p = gc.pkg()
    L = ctypes.CDLL(p.LIB_PATH)
    for fn in NEW_SYMBOLS:
        assert hasattr(L, fn), fn
        assert getattr(p.lib(), fn).argtypes is not None, fn
    for m in ("mc_accumulate", "mc_film_fixed", "mc_overflow", "mc_coverage", "mc_save", "mc_load"):
        assert callable(getattr(p.Renderer, m, None)), m
    assert callable(getattr(p.Group, "mc_render", None))
    assert callable(getattr(p, "mc_file_info", None)) and callable(getattr(p, "mc_file_words", None))


def test_dpt_amd_mc_branch_goes_through_the_group_render_and_reads_the_flags():
    src = open(os.path.join(gc.ROOT, "tools", "dpt_amd.cpp")).read()
    for s in ("lmc_group_mc_render", '"mc_film_exact"', '"--spp"', '"--max-spp"', "lmc_mc_save", "lmc_mc_load"):
        assert s in src, s


# ---------------------------------------------------------------------------------------------- coverage arithmetic, launch cuts
# (adds, total) -> (accepted, held, complement); the stand-alone sanitizer program (tests/helpers/mcfilm_main.cpp) runs the same table
COVERAGE_CASES = [
    # adjacent ranges merge, in either order of arrival, and a range that closes a gap merges both sides
    ([(0, 5), (5, 9)], 12, [True, True], [(0, 9)], [(9, 12)]),
    ([(5, 9), (0, 5)], 12, [True, True], [(0, 9)], [(9, 12)]),
    ([(0, 3), (6, 9), (3, 6)], 9, [True, True, True], [(0, 9)], []),
    # disjoint ranges stay apart, ascending whatever the order of arrival
    ([(8, 10), (0, 2), (4, 5)], 12, [True, True, True], [(0, 2), (4, 5), (8, 10)], [(2, 4), (5, 8), (10, 12)]),
    # every kind of overlap is refused and changes nothing: identical, inside, around, over the left edge, over the right edge, one id
    ([(4, 8), (4, 8), (5, 6), (3, 9), (2, 5), (7, 11), (7, 8), (4, 5)], 12, [True] + [False] * 7, [(4, 8)], [(0, 4), (8, 12)]),
    # ... across two held ranges and the gap between them
    ([(0, 2), (4, 6), (1, 5), (2, 5), (1, 4)], 8, [True, True, False, False, False], [(0, 2), (4, 6)], [(2, 4), (6, 8)]),
    # an empty range is accepted and adds nothing; a reversed or negative one is refused
    ([(3, 3), (5, 4), (-1, 2), (0, 1)], 4, [True, False, False, True], [(0, 1)], [(1, 4)]),
    # the complement is cut at total; a film that holds everything lacks nothing; an empty film lacks everything
    ([(2, 20)], 10, [True], [(2, 20)], [(0, 2)]),
    ([(0, 24)], 24, [True], [(0, 24)], []),
    ([], 7, [], [], [(0, 7)]),
]


@pytest.mark.parametrize("case", range(len(COVERAGE_CASES)))
def test_coverage_arithmetic(case):
    adds, total, accepted, held, comp = COVERAGE_CASES[case]
    got = gc.pkg().mc_coverage_probe(adds, total)
    assert got == (accepted, held, comp), got


# (begin, end, nTiles, cap) -> launches
CHUNK_CASES = [
    ((0, 48, 12, 262144), [(0, 48)]),                                       # under the cap: one launch
    ((0, 48, 12, 5), [(0, 5), (5, 10), (10, 12), (12, 17), (17, 22), (22, 24), (24, 29), (29, 34), (34, 36), (36, 41), (41, 46), (46, 48)]),  # a cap below nTiles
    ((0, 48, 12, 30), [(0, 24), (24, 48)]),                                 # cuts fall on multiples of nTiles
    ((7, 48, 12, 30), [(7, 36), (36, 48)]),
    ((17, 17, 12, 5), []),
    ((0, 786432, 3072, 262144), [(0, 261120), (261120, 522240), (522240, 783360), (783360, 786432)]),  # 1024 x 768 at 256 spp
    ((0, 196608, 3072, 262144), [(0, 196608)]),                             # ... at 64 spp: one launch
]


@pytest.mark.parametrize("case", range(len(CHUNK_CASES)))
def test_launch_cuts(case):
    args, want = CHUNK_CASES[case]
    got = gc.pkg().mc_chunks_probe(*args)
    assert got == want, got
    assert all(e - b <= args[3] for b, e in got) and (not got or (got[0][0], got[-1][1]) == args[:2])
    assert all(a[1] == b[0] for a, b in zip(got, got[1:]))


# ---------------------------------------------------------------------------------------------- the state file
def _hand_built_file(path, width=5, height=3, ranges=((0, 2), (3, 4)), spp=4, magic=b"LMCMCFX\n", version=1):
    """a state file written here, field by field, from the layout in include/lmc_abi.h"""
    words = (np.arange(width * height * 3, dtype=np.int64) - 7) * (1 << 33) + 5
    n_tiles = ((width + 15) // 16) * ((height + 15) // 16)
    raw = magic + struct.pack("<II", version, len(ranges)) + struct.pack("<Q", 0x0123456789ABCDEF)
    raw += struct.pack("<8i", 1, width, height, -1, 6, 7, 1, 0)
    raw += struct.pack("<5q", n_tiles, spp, 60, 41, 2)
    for b, e in ranges:
        raw += struct.pack("<2q", b, e)
    raw += words.astype("<i8").tobytes()
    with open(path, "wb") as f:
        f.write(raw)
    return words.reshape(height, width, 3), raw


def test_state_file_round_trip_through_a_hand_built_file(tmp_path):
    p = gc.pkg()
    path = str(tmp_path / "film.mcfx")
    words, raw = _hand_built_file(path)
    info = p.mc_file_info(path)
    assert info["version"] == 1 and info["scene_hash"] == "0123456789abcdef" and info["force_diffuse"] == 1
    assert (info["width"], info["height"], info["mindepth"], info["maxdepth"], info["seedoffset"], info["bidirectional"]) == (5, 3, -1, 6, 7, 1)
    assert (info["n_tiles"], info["spp"], info["paths"], info["contributions"], info["overflow"]) == (1, 4, 60, 41, 2)
    assert info["coverage"] == [[0, 2], [3, 4]] and info["streams_held"] == 3
    assert info["film_words"] == 45 and info["words_offset"] == 96 + 32 and info["total_bytes"] == len(raw)
    got = p.mc_file_words(path)
    assert got.dtype == np.int64 and got.shape == (3, 5, 3) and np.array_equal(got, words)


def test_state_file_refusals_name_the_reason(tmp_path):
    p = gc.pkg()
    path = str(tmp_path / "film.mcfx")
    _, raw = _hand_built_file(path)
    for cut in (len(raw) - 1, 96 + 32 + 8, 96 + 10, 40, 9):  # inside the words, the ranges, the fixed part
        with open(path, "wb") as f:
            f.write(raw[:cut])
        with pytest.raises(RuntimeError, match="short file"):
            p.mc_file_info(path)
    _hand_built_file(path, magic=b"LMCCKPT\n")
    with pytest.raises(RuntimeError, match="wrong magic"):
        p.mc_file_info(path)
    _hand_built_file(path, version=2)
    with pytest.raises(RuntimeError, match="wrong version"):
        p.mc_file_info(path)
    _hand_built_file(path, ranges=((0, 2), (2, 4)))  # not merged
    with pytest.raises(RuntimeError, match="coverage"):
        p.mc_file_info(path)
    with pytest.raises(RuntimeError, match="cannot open"):
        p.mc_file_info(str(tmp_path / "absent.mcfx"))


def test_mcfilm_stand_alone_under_the_sanitizers(tmp_path):
    """host/mcfilm.cpp with a main of its own (tests/helpers/mcfilm_main.cpp), built with -fsanitize=address,undefined: the coverage table above, the
    launch cuts, a write / read round trip of the state file and its refusals"""
    exe = str(tmp_path / "mcfilm_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           "-I" + os.path.dirname(MCFILM_SRC), MCFILM_MAIN, MCFILM_SRC, "-o", exe], cwd=gc.ROOT)
    lines = []
    for adds, total, accepted, held, comp in COVERAGE_CASES:
        flat = lambda rs: " ".join("%d %d" % r for r in rs)
        lines.append("coverage %d %d %s | %s | %d %s | %d %s" % (total, len(adds), flat(adds), " ".join(str(int(a)) for a in accepted), len(held), flat(held), len(comp), flat(comp)))
    for args, want in CHUNK_CASES:
        lines.append("chunks %d %d %d %d | %d %s" % (args + (len(want), " ".join("%d %d" % r for r in want))))
    lines.append("file " + str(tmp_path / "san.mcfx"))
    r = subprocess.run([exe], input="\n".join(lines) + "\n", stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    assert r.stdout.rstrip().endswith("ok %d cases" % len(lines)), r.stdout


# ---------------------------------------------------------------------------------------------- the fixed-point oracle
def test_fixed_point_oracle_agrees_with_the_float_oracle():
    """its words converted as lmc_mc_read converts them pass the film bar against oracle_mc's float film, and the counts are the same"""
    for bidir, seed_offset, spp in ((True, 0, 2), (False, 7, 3)):
        w, pw, nw, dropped = oracle_mc_fx(gc.TORUS, spp, seed_offset=seed_offset, bidir=bidir)
        o, po, no = oracle_mc(gc.TORUS, spp, seed_offset=seed_offset, bidir=bidir)
        assert pw == po == 64 * 48 * spp and nw == no and nw > 0 and dropped == 0, (pw, po, nw, no, dropped)
        _film_close(words_to_float(w, spp), o)


def test_fixed_point_oracle_literal_loop_at_one_sample():
    """spp = 1, seedoffset 0: the stream layout is the reference's loop -- word for word"""
    for bidir in (True, False):
        a = oracle_mc_fx(gc.TORUS, 1, bidir=bidir)
        b = oracle_mc_fx(gc.TORUS, 1, bidir=bidir, literal=True)
        assert a[1:] == b[1:] and np.array_equal(a[0], b[0]) and a[0].any(), bidir


def test_fixed_point_oracle_ranges_sum_to_the_whole_word_for_word():
    nTiles = 4 * 3
    full = oracle_mc_fx(gc.TORUS, 2, seed_offset=7)
    a = oracle_mc_fx(gc.TORUS, 2, seed_offset=7, streams=(0, 9))
    b = oracle_mc_fx(gc.TORUS, 2, seed_offset=7, streams=(9, 2 * nTiles))
    assert a[1] + b[1] == full[1] == 2 * 64 * 48 and a[2] + b[2] == full[2] and a[3] == b[3] == full[3] == 0
    assert np.array_equal(a[0] + b[0], full[0]) and a[0].any() and b[0].any()
