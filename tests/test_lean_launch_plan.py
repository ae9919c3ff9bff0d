"""CPU tier: the LDS plan of the lean small-step launch (device/dsmall.h LeanStackWords / LeanLdsWordsPerThread) through the exported probe
lmc_lean_plan_probe (include/lmc_abi.h), which runs host arithmetic only.

A thread's stack region holds the tree's stack need rounded up to a multiple of 4, and never fewer than 2 * PSS_MAX_LENGTH = 24 words: between
traversals the region stages the stored Gaussian / the moment vectors of a state of up to 12 dimensions, filled in groups of four.  Behind it come
2 * MAXD = 24 words (proposal offsets, new primary-sample vector).  The host's stack need is an upper bound for the walks the kernels run (accel.cpp Collapse, dscene.h LdsStackT::Push), so nothing is added above it.

Why the numbers matter: the Lambertian lightless instantiations are compiled for three waves per SIMD = three blocks of 256 per CU, and a CU has
160 KB of LDS: 3 x (256 x 52 x 4 + 1 280 static bytes of the jump and logf tables) = 163 584 <= 163 840 for the torus (stack need 25 .. 28), where the
former rounding (multiple of 8, at least 32: 56 words) stopped at eleven waves.  (Launched in one-wave blocks, the default, every wave pays the static
bytes: eleven blocks per CU with 52 words, ten with 56.)

NOT here: a guard that `words x N x 4` fits 32 bits (304-word path record, N just below and just above the limit).  The lean kernel still forms
64-bit per-lane addresses; addressing by a scalar base plus a 32-bit lane offset was not built, so there is no guard to test.  A change that
introduces such offsets has to bring the guard, its probe and these cases with it."""
import ctypes

import pytest

from tests import gpu_checks as gc

MD2, MAXPSS = 24, 24  # dsmall.h: 2 * MD; dpath.h: MAXPSS = 2 * MAXD
CU_LDS_BYTES, STATIC_LDS_BYTES = 163840, 1280  # gfx950; drng.h: 64 jump constants of 16 B + 16 logf table rows of 16 B

# stack need -> stack words of a thread
CASES = [(0, 24), (23, 24), (24, 24), (25, 28), (27, 28), (28, 28), (37, 40), (40, 40)]


def _probe(need, block=256):
    L = gc.pkg().lib()
    L.lmc_lean_plan_probe.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_longlong)]
    L.lmc_lean_plan_probe.restype = ctypes.c_int
    sw, wpt, nbytes = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_longlong(-1)
    rc = L.lmc_lean_plan_probe(need, block, ctypes.byref(sw), ctypes.byref(wpt), ctypes.byref(nbytes))
    return rc, sw.value, wpt.value, nbytes.value


@pytest.mark.parametrize("need,stack_words", CASES)
def test_stack_words_and_lds_words_per_thread(need, stack_words):
    rc, sw, wpt, nbytes = _probe(need)
    assert rc == 0
    assert sw == stack_words
    assert sw >= need and sw >= MD2 and sw % 4 == 0 and (sw - need < 4 or sw == MD2)
    assert wpt == stack_words + MAXPSS
    assert nbytes == 256 * (stack_words + MAXPSS) * 4


def test_the_torus_plan_leaves_room_for_three_blocks_per_cu():
    for need in (25, 26, 27, 28):
        rc, sw, wpt, nbytes = _probe(need)
        assert (rc, sw, wpt, nbytes) == (0, 28, 52, 53248)
        assert 3 * (nbytes + STATIC_LDS_BYTES) <= CU_LDS_BYTES
    # the door scene (need 37) keeps the 40 entries of BVH_LDS_STACK
    assert _probe(37)[1:] == (40, 64, 65536)


def test_block_size_scales_the_bytes_and_bad_arguments_are_refused():
    assert _probe(28, 64)[3] == 64 * 52 * 4
    assert _probe(-1)[0] != 0
    assert _probe(28, 32)[0] != 0  # the launch needs blocks of at least 64 threads (drng.h RequireJumpLdsBlock)
