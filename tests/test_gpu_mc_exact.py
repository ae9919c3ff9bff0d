"""`-m gpu` tier: the exact mc film (lmc_set_option "mc_film_exact"; device/mc.hip k_mc over FilmFixed, host/mcfilm.cpp) word for word against the
fixed-point CPU oracle (tests/helpers/mc_oracle_fx.cpp), across cuts into calls, launches, members and files, at the edges of the wave reduction,
under the range rule, and through dpt_amd.  Films and sample counts are those of tests/test_gpu_mc.py."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import gpu_checks as gc
from tests.test_gpu_mc import CLI, SCENES, VEACH, _film_close, _mc_scene
from tests.test_mc_abi import oracle_mc
from tests.test_mc_exact_abi import oracle_mc_fx, words_to_float

pytestmark = pytest.mark.gpu
N_TILES = 4 * 3  # of the 64 x 48 film


def _renderer(name, seed_offset, bidir, exact=True, width=None, height=None, xml=None):
    sxml, fd, md, W, H = SCENES[name]
    ren = gc.pkg().Renderer(xml or sxml, force_diffuse=fd, max_depth=md, width=width or W, height=height or H, seed_offset=seed_offset, use_gradient=0)
    ren.set_option("bidirectional", 1 if bidir else 0)
    ren.set_option("mc_film_exact", 1 if exact else 0)
    assert ren.get_option("mc_film_exact") == (1 if exact else 0)
    return ren


def _oracle(name, spp, seed_offset, bidir, min_depth, width=None, height=None, xml=None, streams=None):
    sxml, fd, md, W, H = SCENES[name]
    return oracle_mc_fx(xml or sxml, spp, force_diffuse=fd, max_depth=md, width=width or W, height=height or H, seed_offset=seed_offset, min_depth=min_depth, bidir=bidir,
                        streams=streams)


def _differing(g, o):
    """how a failing word-for-word comparison reads: the number of differing words and the first differing pixel"""
    bad = np.argwhere(g != o)
    return "%d of %d words differ, first at pixel (x=%d, y=%d) channel %d: %d vs %d" % (len(bad), g.size, bad[0][1], bad[0][0], bad[0][2], g[tuple(bad[0])], o[tuple(bad[0])]) if len(bad) else ""


def _check_against_the_oracle(name, spp, seed_offset, bidir, width=None, height=None):
    sxml, fd, md, W, H = SCENES[name]
    W, H = width or W, height or H
    ren = _renderer(name, seed_offset, bidir, width=W, height=H)
    min_depth = int(ren.get_option("mindepth"))
    ren.mc_render(spp)
    g, (gp, gn), gov, cov = ren.mc_film_fixed(), ren.mc_stats(), ren.mc_overflow(), ren.mc_coverage()
    ren.close()
    o, op, on, odrop = _oracle(name, spp, seed_offset, bidir, min_depth, width=W, height=H)
    print("%s bidir=%d seed=%d spp=%d %dx%d: paths %d / %d, contributions %d / %d, overflow %d / %d" % (name, bidir, seed_offset, spp, W, H, gp, op, gn, on, gov, odrop))
    assert gp == op == W * H * spp, (gp, op)
    assert gn == on, (name, bidir, seed_offset, gn, on)
    assert gov == odrop == 0
    assert cov == [(0, ((W + 15) // 16) * ((H + 15) // 16) * spp)]
    assert o.any() and np.array_equal(g, o), _differing(g, o)


# ---- 1. word for word against the fixed-point oracle
@pytest.mark.parametrize("name", list(SCENES))
@pytest.mark.parametrize("bidir", [True, False])
def test_exact_mc_film_equals_the_fixed_point_oracle(name, bidir):
    for seed_offset, spp in ((0, 2), (7, 3)):
        _check_against_the_oracle(name, spp, seed_offset, bidir)


# ---- 2. read conversion
@pytest.mark.parametrize("bidir", [True, False])
def test_exact_mc_read_is_the_stated_conversion_and_close_to_the_float_film(bidir):
    spp = 3
    ren = _renderer("torus_materials", 7, bidir)
    img = ren.mc_render(spp)
    words = ren.mc_film_fixed()
    ren.set_option("mc_film_exact", 0)  # takes effect at the next mc_render
    assert np.array_equal(ren.mc_film_fixed(), words)
    flt = ren.mc_render(spp)
    with pytest.raises(RuntimeError, match="float mode"):
        ren.mc_film_fixed()
    assert ren.mc_overflow() == 0 and ren.mc_coverage() == []
    ren.close()
    want = words_to_float(words, spp)
    assert img.dtype == np.float32 and np.array_equal(img.view(np.uint32), want.view(np.uint32))
    _film_close(img, flt)


# ---- 3. cuts do not show
@pytest.fixture(scope="module")
def lambert_whole():
    """torus Lambertian, seed offset 7, 4 spp, one launch: (words, stats), shared and read-only"""
    ren = _renderer("torus_lambert", 7, True)
    ren.mc_render(4)
    words, stats = ren.mc_film_fixed(), ren.mc_stats()
    assert ren.get_option("mc_launches") == 1 and ren.mc_overflow() == 0
    ren.close()
    words.setflags(write=False)
    assert words.any() and stats[0] == 64 * 48 * 4
    return words, stats


def test_stream_ranges_sum_to_the_whole_word_for_word(lambert_whole):
    words, stats = lambert_whole
    ren = _renderer("torus_lambert", 7, True)
    ren.mc_render(4, streams=(0, 17))
    a, sa, ca = ren.mc_film_fixed(), ren.mc_stats(), ren.mc_coverage()
    ren.mc_render(4, streams=(17, -1))
    b, sb, cb = ren.mc_film_fixed(), ren.mc_stats(), ren.mc_coverage()
    ren.close()
    assert ca == [(0, 17)] and cb == [(17, 4 * N_TILES)]
    assert (sa[0] + sb[0], sa[1] + sb[1]) == stats
    assert a.any() and b.any() and np.array_equal(a + b, words), _differing(a + b, words)


def test_render_then_accumulate_equals_the_whole(lambert_whole):
    words, stats = lambert_whole
    ren = _renderer("torus_lambert", 7, True)
    ren.mc_render(4, streams=(0, 17))
    part = ren.mc_film_fixed()
    img = ren.mc_accumulate(4, streams=(17, -1))
    g = ren.mc_film_fixed()
    assert ren.mc_stats() == stats and ren.mc_coverage() == [(0, 4 * N_TILES)]
    ren.close()
    assert not np.array_equal(part, words) and np.array_equal(g, words), _differing(g, words)
    assert np.array_equal(img.view(np.uint32), words_to_float(words, 4).view(np.uint32))


def test_more_samples_are_added_to_a_finished_render(lambert_whole):
    """2 spp, then the sample indices 2 and 3: the 4 spp render"""
    words, stats = lambert_whole
    ren = _renderer("torus_lambert", 7, True)
    two = ren.mc_render(2)
    w2 = ren.mc_film_fixed()
    assert np.array_equal(two.view(np.uint32), words_to_float(w2, 2).view(np.uint32))
    four = ren.mc_accumulate(4, streams=(2 * N_TILES, 4 * N_TILES))
    g = ren.mc_film_fixed()
    assert ren.mc_stats() == stats and ren.mc_coverage() == [(0, 4 * N_TILES)]
    ren.close()
    assert np.array_equal(g, words), _differing(g, words)
    assert np.array_equal(four.view(np.uint32), words_to_float(words, 4).view(np.uint32))


def test_launch_cuts_do_not_show(lambert_whole):
    """5 stream ids per launch, no multiple of nTiles = 12"""
    words, stats = lambert_whole
    ren = _renderer("torus_lambert", 7, True)
    ren.set_option("mc_launch_streams", 5)
    assert ren.get_option("mc_launch_streams") == 5
    ren.mc_render(4)
    g, launches = ren.mc_film_fixed(), ren.get_option("mc_launches")
    assert ren.mc_stats() == stats and ren.mc_coverage() == [(0, 4 * N_TILES)] and ren.mc_overflow() == 0
    ren.close()
    assert launches == len(gc.pkg().mc_chunks_probe(0, 4 * N_TILES, N_TILES, 5)) > 1
    assert np.array_equal(g, words), _differing(g, words)


def test_an_overlapping_accumulate_is_refused_and_changes_nothing(lambert_whole):
    ren = _renderer("torus_lambert", 7, True)
    ren.mc_render(4, streams=(5, 17))
    before, stats = ren.mc_film_fixed(), ren.mc_stats()
    for streams in ((0, 6), (16, 20), (5, 17), (8, 9), (0, -1)):
        with pytest.raises(RuntimeError, match="overlaps"):
            ren.mc_accumulate(4, streams=streams)
        assert np.array_equal(ren.mc_film_fixed(), before) and ren.mc_stats() == stats and ren.mc_coverage() == [(5, 17)]
    with pytest.raises(RuntimeError, match="beyond"):  # the film holds ids of sample index 1: not a 1 spp film
        ren.mc_accumulate(1, streams=(0, 5))
    ren.mc_accumulate(4, streams=(0, 5))  # the context stays usable
    ren.mc_accumulate(4, streams=(17, -1))
    g = ren.mc_film_fixed()
    ren.close()
    assert np.array_equal(g, lambert_whole[0])
    flt = _renderer("torus_lambert", 7, True, exact=False)
    with pytest.raises(RuntimeError, match="float mode"):
        flt.mc_accumulate(4)
    flt.close()


# ---- 4. the wave reduction at its edges
@pytest.mark.parametrize("width,height,spp", [
    (16, 16, 64),  # one tile: all 64 lanes of a wave share one pixel
    (64, 48, 1),   # every lane of a wave on a different tile
    (64, 48, 3),   # 21 same-pixel groups per wave, four reduction rounds: the rest take the per-lane atomics
    (24, 20, 2),   # partial tiles
])
@pytest.mark.parametrize("bidir", [True, False])
def test_wave_reduction_edges(width, height, spp, bidir):
    _check_against_the_oracle("torus_lambert", spp, 7, bidir, width=width, height=height)


# ---- 5. the range rule
def _bright_door(tmp_path):
    """veach-door with the emitter's radiance scaled up until the fixed-point ORACLE drops some, not all, contributions by the range rule"""
    src = open(VEACH).read()
    line = '<rgb name="radiance" value="1420 1552 1642"/>'
    assert src.count(line) == 1
    sxml, fd, md, W, H = SCENES["veachdoor"]
    os.symlink(os.path.join(os.path.dirname(VEACH), "data"), tmp_path / "data")
    for k, factor in enumerate((1e8, 1e9, 1e7, 1e10, 1e6)):  # (1e8: 16 of 1895 bidirectional, 66 of 483 unidirectional contributions dropped)
        p = tmp_path / ("door_x%d.xml" % k)
        p.write_text(src.replace(line, '<rgb name="radiance" value="%r %r %r"/>' % (1420 * factor, 1552 * factor, 1642 * factor)))
        drops = [oracle_mc_fx(str(p), 2, force_diffuse=fd, max_depth=md, width=W, height=H, seed_offset=7, bidir=b)[2:] for b in (True, False)]
        if all(0 < dropped < counted for counted, dropped in drops):
            return str(p), factor
    raise AssertionError("no factor makes the oracle drop some but not all contributions")


def test_range_rule_drops_whole_contributions_like_the_oracle(tmp_path):
    xml, factor = _bright_door(tmp_path)
    for bidir in (True, False):
        ren = _renderer("veachdoor", 7, bidir, xml=xml)
        min_depth = int(ren.get_option("mindepth"))
        o, op, on, odrop = _oracle("veachdoor", 2, 7, bidir, min_depth, xml=xml)
        print("radiance x %g, bidir=%d: oracle %d contributions, %d dropped" % (factor, bidir, on, odrop))
        assert 0 < odrop < on, (odrop, on)
        ren.mc_render(2)
        g, (gp, gn), gov = ren.mc_film_fixed(), ren.mc_stats(), ren.mc_overflow()
        ren.close()
        assert (gp, gn, gov) == (op, on, odrop), (gp, gn, gov, op, on, odrop)
        assert np.array_equal(g, o), _differing(g, o)


# ---- 6. groups
@pytest.mark.parametrize("members", [2, 3])
def test_group_render_leaves_the_whole_on_member_zero(members, lambert_whole):
    words, stats = lambert_whole
    p = gc.pkg()
    rens = [_renderer("torus_lambert", 7, True) for _ in range(members)]
    img = p.Group(rens).mc_render(4)
    g = rens[0].mc_film_fixed()
    assert rens[0].mc_stats() == stats and rens[0].mc_coverage() == [(0, 4 * N_TILES)] and rens[0].mc_overflow() == 0
    for r in rens[1:]:
        assert not r.mc_film_fixed().any() and r.mc_stats() == (0, 0) and r.mc_coverage() == []
    for r in rens:
        r.close()
    assert np.array_equal(g, words), _differing(g, words)
    assert np.array_equal(img.view(np.uint32), words_to_float(words, 4).view(np.uint32))


def test_group_of_mixed_modes_is_refused_and_the_members_stay_usable(lambert_whole):
    p = gc.pkg()
    rens = [_renderer("torus_lambert", 7, True), _renderer("torus_lambert", 7, True, exact=False)]
    rens[0].mc_render(4, streams=(0, 17))
    before = rens[0].mc_film_fixed()
    with pytest.raises(RuntimeError, match="differ in mc_film_exact"):
        p.Group(rens).mc_render(4)
    assert np.array_equal(rens[0].mc_film_fixed(), before) and rens[0].mc_coverage() == [(0, 17)]  # nothing was rendered
    rens[0].mc_accumulate(4, streams=(17, -1))
    assert np.array_equal(rens[0].mc_film_fixed(), lambert_whole[0])
    flt = rens[1].mc_render(4)
    _film_close(flt, words_to_float(lambert_whole[0], 4))
    for r in rens:
        r.close()


def test_float_group_render_is_the_host_sum_in_member_order():
    """float mode: member 0's film is shard 0 + shard 1 + shard 2 added in that order, the sum dpt_amd's host loop made"""
    p = gc.pkg()
    rens = [_renderer("torus_lambert", 7, True, exact=False) for _ in range(3)]
    img = p.Group(rens).mc_render(4)
    stats = rens[0].mc_stats()
    for r in rens:
        r.close()
    whole, op, on = oracle_mc(gc.TORUS, 4, seed_offset=7)
    assert stats == (op, on)
    _film_close(img, whole)


# ---- 7. save and load
def test_save_load_and_continue(tmp_path, lambert_whole):
    words, stats = lambert_whole
    p = gc.pkg()
    path = str(tmp_path / "half.mcfx")
    a = _renderer("torus_lambert", 7, True)
    a.mc_render(4, streams=(0, 2 * N_TILES))
    half, half_stats = a.mc_film_fixed(), a.mc_stats()
    a.mc_save(path)
    a.close()
    assert not os.path.exists(path + ".tmp")
    info = p.mc_file_info(path)
    assert (info["width"], info["height"], info["seedoffset"], info["bidirectional"], info["n_tiles"], info["spp"]) == (64, 48, 7, 1, N_TILES, 4)
    assert (info["paths"], info["contributions"], info["overflow"]) == half_stats + (0,) and info["coverage"] == [[0, 2 * N_TILES]]
    assert np.array_equal(p.mc_file_words(path), half)
    b = _renderer("torus_lambert", 7, True)
    b.mc_load(path)
    assert np.array_equal(b.mc_film_fixed(), half) and b.mc_stats() == half_stats and b.mc_coverage() == [(0, 2 * N_TILES)]
    with pytest.raises(RuntimeError, match="overlaps"):
        b.mc_accumulate(4, streams=(0, -1))
    b.mc_accumulate(4, streams=(2 * N_TILES, -1))
    g = b.mc_film_fixed()
    assert b.mc_stats() == stats and b.mc_coverage() == [(0, 4 * N_TILES)]
    b.close()
    assert np.array_equal(g, words), _differing(g, words)


def test_load_refuses_a_file_of_another_render_and_names_the_field(tmp_path, lambert_whole):
    path = str(tmp_path / "film.mcfx")
    a = _renderer("torus_lambert", 7, True)
    a.mc_render(4)
    a.mc_save(path)
    a.close()
    for field, kw in (("width", dict(width=48, height=48)), ("height", dict(width=64, height=32)), ("seedoffset", dict(seed_offset=0)), ("bidirectional", dict(bidir=False))):
        b = _renderer("torus_lambert", kw.pop("seed_offset", 7), kw.pop("bidir", True), **kw)
        b.mc_render(1, streams=(0, 3))
        before = b.mc_film_fixed()
        with pytest.raises(RuntimeError, match="differs in " + field):
            b.mc_load(path)
        assert np.array_equal(b.mc_film_fixed(), before) and b.mc_coverage() == [(0, 3)]  # the context is as it was
        b.close()
    flt = _renderer("torus_lambert", 7, True, exact=False)
    with pytest.raises(RuntimeError, match="float mode"):
        flt.mc_load(path)
    with pytest.raises(RuntimeError, match="no exact mc film"):
        flt.mc_save(str(tmp_path / "none.mcfx"))
    flt.close()


# ---- 8. float mode guard
def test_float_mode_is_one_launch_and_passes_the_existing_bar():
    xml, fd, md, W, H = SCENES["torus_materials"]
    ren = gc.pkg().Renderer(xml, force_diffuse=fd, max_depth=md, width=W, height=H, seed_offset=7, use_gradient=0)
    assert ren.get_option("mc_film_exact") == 0 and ren.get_option("mc_launch_streams") == 262144
    min_depth = int(ren.get_option("mindepth"))
    g = ren.mc_render(3)
    gp, gn = ren.mc_stats()
    assert ren.get_option("mc_launches") == 1
    ren.close()
    o, op, on = oracle_mc(xml, 3, force_diffuse=fd, max_depth=md, width=W, height=H, seed_offset=7, min_depth=min_depth, bidir=True)
    assert (gp, gn) == (op, on)
    _film_close(g, o)


# ---- 9. dpt_amd
def _cli(args, tmp_path, expect=0):
    for f in os.listdir(tmp_path):
        if f.endswith(".exr"):
            os.remove(tmp_path / f)
    r = subprocess.run([CLI] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == expect, r.stdout
    if expect != 0:
        return r.stdout, None
    assert r.stdout.rstrip().endswith("Done!"), r.stdout
    exrs = [f for f in os.listdir(tmp_path) if re.fullmatch(r"lmc_timeuse_[0-9]+\.[0-9]{6}s\.exr", f)]
    assert len(exrs) == 1, os.listdir(tmp_path)
    return r.stdout, open(tmp_path / exrs[0], "rb").read()


def test_dpt_amd_exact_mc_film_is_the_same_for_any_devices_and_legs(tmp_path):
    p = gc.pkg()
    scene = _mc_scene(tmp_path, extra=[('<boolean name="mala"           value="true"/>', '<boolean name="mala" value="false"/>')])
    A, B, C, C2 = (str(tmp_path / n) for n in ("a.mcfx", "b.mcfx", "c.mcfx", "c2.mcfx"))
    out_a, exr_a = _cli(["--exact-film", "--checkpoint", A, scene], tmp_path)
    assert "Exact film: 64-bit fixed-point accumulation" in out_a
    out_b, exr_b = _cli(["--exact-film", "--devices", "0,0,0", "--checkpoint", B, scene], tmp_path)
    assert "sharded over 3 devices" in out_b
    out_c, exr_c = _cli(["--exact-film", "--max-spp", "2", "--checkpoint", C, scene], tmp_path)
    assert p.mc_file_info(C)["spp"] == 2 and p.mc_file_info(C)["coverage"] == [[0, 2 * N_TILES]]
    out_c2, exr_c2 = _cli(["--resume", C, "--checkpoint", C2, scene], tmp_path)
    assert "Exact film" in out_c2  # the mode comes from the file
    wa = p.mc_file_words(A)
    assert wa.any() and np.array_equal(p.mc_file_words(B), wa) and np.array_equal(p.mc_file_words(C2), wa)
    assert not np.array_equal(p.mc_file_words(C), wa)
    for path in (A, B, C2):
        info = p.mc_file_info(path)
        assert info["spp"] == 4 and info["coverage"] == [[0, 4 * N_TILES]] and info["paths"] == 64 * 48 * 4, info
    assert exr_a == exr_b == exr_c2 and exr_c != exr_a
    # the library's own render of the scene: the same words
    ren = p.Renderer(scene, seed_offset=0, use_gradient=0)
    ren.set_option("mc_film_exact", 1)
    ren.mc_render(4)
    assert np.array_equal(ren.mc_film_fixed(), wa)
    ren.close()
    # --spp overrides the scene's count
    D = str(tmp_path / "d.mcfx")
    _cli(["--exact-film", "--spp", "2", "--checkpoint", D, scene], tmp_path)
    assert np.array_equal(p.mc_file_words(D), p.mc_file_words(C))
    # checkpoints need the exact film
    out, _ = _cli(["--checkpoint", str(tmp_path / "e.mcfx"), scene], tmp_path, expect=2)
    assert "--exact-film" in out and not os.path.exists(tmp_path / "e.mcfx")
