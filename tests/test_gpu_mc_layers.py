"""`-m gpu` tier: the layered mc film (lmc_set_option "mc_layers"; device/mc.hip k_mc over FilmLayers / FilmFixedLayers, host/mcrender.cpp) layer for layer
against the layered fixed-point CPU oracle (tests/helpers/mc_oracle_layers_fx.cpp), its sum against the unlayered film of the same context, across cuts
into calls and launches, at the edges of the wave reduction, under the range rule, in float mode, at its refusals and through dpt_amd.  Films and
sample counts are those of tests/test_gpu_mc.py."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import gpu_checks as gc
from tests.test_gpu_mc import CLI, VEACH, _film_close, _mc_scene
from tests.test_gpu_mc_exact import _differing
from tests.test_mc_exact_abi import words_to_float
from tests.test_mc_layers_abi import LENGTH, SAMPLES, SCENES, TECHNIQUE, layer_count, layer_table, scene_oracle

pytestmark = pytest.mark.gpu
N_TILES = 4 * 3  # of the 64 x 48 film


def _renderer(name, seed_offset, bidir, mode, exact=True, width=None, height=None, xml=None):
    sxml, fd, md, W, H, D = SCENES[name]
    ren = gc.pkg().Renderer(xml or sxml, force_diffuse=fd, max_depth=md, width=width or W, height=height or H, seed_offset=seed_offset, use_gradient=0)
    assert ren.get_option("mc_layers") == 0 and ren.mc_layer_info() == (0, [])  # off by default
    ren.set_option("bidirectional", 1 if bidir else 0)
    ren.set_option("mc_film_exact", 1 if exact else 0)
    ren.set_option("mc_layers", mode)
    assert ren.get_option("mc_layers") == mode and ren.get_option("maxdepth") == D
    return ren


def _layers_equal(g, o):
    """word for word, layer for layer; layers that are empty in the oracle are all-zero on the device"""
    assert g.shape == o.shape and g.dtype == np.int64, (g.shape, o.shape)
    for k in range(len(o)):
        assert np.array_equal(g[k], o[k]), "layer %d: %s" % (k, _differing(g[k], o[k]))
        if not o[k].any():
            assert not g[k].any(), k


def _check_against_the_oracle(name, mode, spp, seed_offset, bidir, width=None, height=None):
    """exact mode: every layer word for word, the counters, overflow (0) and coverage; in the same render the sum identities: the layers sum to the film
    of the context, to an unlayered render made afterwards on it, with the same stats, and lmc_mc_read_layer is the stated conversion bit for bit"""
    sxml, fd, md, W, H, D = SCENES[name]
    W, H = width or W, height or H
    ren = _renderer(name, seed_offset, bidir, mode, width=W, height=H)
    min_depth = int(ren.get_option("mindepth"))
    img = ren.mc_render(spp)
    info = ren.mc_layer_info()
    g, total, (gp, gn), gov, cov = ren.mc_layers_fixed(), ren.mc_film_fixed(), ren.mc_stats(), ren.mc_overflow(), ren.mc_coverage()
    o, op, on, odrop, outside = scene_oracle(name, mode, spp, seed_offset, bidir, min_depth, width=W, height=H)
    filled = [k for k in range(len(o)) if o[k].any()]
    floats = {k: ren.mc_layer(k) for k in filled[:2] + filled[-1:] + [0]}
    ren.set_option("mc_layers", 0)  # takes effect at the next mc_render
    assert ren.mc_layer_info() == info
    plain_img = ren.mc_render(spp)
    plain, plain_stats = ren.mc_film_fixed(), ren.mc_stats()
    assert ren.mc_layer_info() == (0, [])
    with pytest.raises(RuntimeError, match="no layered mc film"):
        ren.mc_layer_fixed(0)
    ren.close()
    print("%s mode=%d bidir=%d seed=%d spp=%d %dx%d: paths %d / %d, contributions %d / %d, overflow %d / %d, %d of %d layers filled" %
          (name, mode, bidir, seed_offset, spp, W, H, gp, op, gn, on, gov, odrop, len(filled), len(o)))
    assert info == (mode, layer_table(mode, D)) and len(g) == layer_count(mode, D)
    assert gp == op == W * H * spp, (gp, op)
    assert gn == on, (name, bidir, seed_offset, gn, on)
    assert gov == odrop == 0 and outside == 0
    assert cov == [(0, ((W + 15) // 16) * ((H + 15) // 16) * spp)]
    assert filled
    _layers_equal(g, o)
    assert np.array_equal(g.sum(0), total), _differing(g.sum(0), total)
    assert np.array_equal(total, plain), _differing(total, plain)
    assert plain_stats == (gp, gn)
    assert np.array_equal(img.view(np.uint32), plain_img.view(np.uint32))
    for k, f in floats.items():
        assert f.dtype == np.float32 and np.array_equal(f.view(np.uint32), words_to_float(g[k], spp).view(np.uint32)), k


# ---- 1. + 2. every layer word for word against the layered oracle, and the sum identities
@pytest.mark.parametrize("name", list(SCENES))
@pytest.mark.parametrize("bidir", [True, False])
def test_length_layers_equal_the_layered_oracle(name, bidir):
    for seed_offset, spp in SAMPLES:
        _check_against_the_oracle(name, LENGTH, spp, seed_offset, bidir)


@pytest.mark.parametrize("name,bidir", [("veachdoor", True), ("torus_materials", True), ("torus_lambert", False)])
def test_technique_layers_equal_the_layered_oracle(name, bidir):
    for seed_offset, spp in SAMPLES:
        _check_against_the_oracle(name, TECHNIQUE, spp, seed_offset, bidir)


# ---- 3. the reduction's edges
@pytest.mark.parametrize("width,height,spp", [
    (16, 16, 64),  # one tile: all 64 lanes of a wave share one pixel and change layer together
    (64, 48, 1),   # every lane of a wave on a different tile
    (64, 48, 3),   # 21 same-pixel groups per wave, four reduction rounds: the rest take the per-lane atomics
    (24, 20, 2),   # partial tiles
])
@pytest.mark.parametrize("bidir", [True, False])
def test_wave_reduction_edges_by_length(width, height, spp, bidir):
    _check_against_the_oracle("torus_lambert", LENGTH, spp, 7, bidir, width=width, height=height)


def test_wave_reduction_edges_by_technique():
    _check_against_the_oracle("torus_lambert", TECHNIQUE, 64, 7, True, width=16, height=16)


# ---- 4. cuts do not show
@pytest.fixture(scope="module")
def lambert_whole():
    """torus Lambertian, seed offset 7, 4 spp, by length, one launch: (layers, stats), shared and read-only"""
    ren = _renderer("torus_lambert", 7, True, LENGTH)
    ren.mc_render(4)
    layers, stats = ren.mc_layers_fixed(), ren.mc_stats()
    assert ren.get_option("mc_launches") == 1 and ren.mc_overflow() == 0
    ren.close()
    layers.setflags(write=False)
    assert sum(l.any() for l in layers) >= 5 and stats[0] == 64 * 48 * 4
    return layers, stats


def test_stream_ranges_in_two_calls_equal_the_whole(lambert_whole):
    layers, stats = lambert_whole
    ren = _renderer("torus_lambert", 7, True, LENGTH)
    ren.mc_render(4, streams=(0, 17))
    a, sa = ren.mc_layers_fixed(), ren.mc_stats()
    ren.mc_render(4, streams=(17, -1))
    b, sb = ren.mc_layers_fixed(), ren.mc_stats()
    assert a.any() and b.any() and (sa[0] + sb[0], sa[1] + sb[1]) == stats
    _layers_equal(a + b, layers)
    ren.mc_render(4, streams=(0, 17))
    ren.mc_accumulate(4, streams=(17, -1))
    g, total = ren.mc_layers_fixed(), ren.mc_film_fixed()
    assert ren.mc_stats() == stats and ren.mc_coverage() == [(0, 4 * N_TILES)]
    ren.close()
    _layers_equal(g, layers)
    assert np.array_equal(total, layers.sum(0))


def test_launch_cuts_do_not_show(lambert_whole):
    """5 stream ids per launch, no multiple of nTiles = 12"""
    layers, stats = lambert_whole
    ren = _renderer("torus_lambert", 7, True, LENGTH)
    ren.set_option("mc_launch_streams", 5)
    ren.mc_render(4)
    g, launches = ren.mc_layers_fixed(), ren.get_option("mc_launches")
    assert ren.mc_stats() == stats and ren.mc_coverage() == [(0, 4 * N_TILES)] and ren.mc_overflow() == 0
    ren.close()
    assert launches == len(gc.pkg().mc_chunks_probe(0, 4 * N_TILES, N_TILES, 5)) > 1
    _layers_equal(g, layers)


def test_more_samples_are_added_layer_by_layer_and_another_mode_is_refused(lambert_whole):
    """2 spp, then the sample indices 2 and 3: the 4 spp render; an accumulate with another mc_layers value is refused and changes nothing"""
    layers, stats = lambert_whole
    ren = _renderer("torus_lambert", 7, True, LENGTH)
    ren.mc_render(2)
    before, before_total, before_stats = ren.mc_layers_fixed(), ren.mc_film_fixed(), ren.mc_stats()
    for other in (TECHNIQUE, 0):
        ren.set_option("mc_layers", other)
        with pytest.raises(RuntimeError, match=r"mc_layers = 1.*mc_layers = %d" % other):
            ren.mc_accumulate(4, streams=(2 * N_TILES, 4 * N_TILES))
        assert ren.mc_layer_info()[0] == LENGTH and np.array_equal(ren.mc_layers_fixed(), before) and np.array_equal(ren.mc_film_fixed(), before_total)
        assert ren.mc_stats() == before_stats and ren.mc_coverage() == [(0, 2 * N_TILES)]
    ren.set_option("mc_layers", LENGTH)
    four = ren.mc_accumulate(4, streams=(2 * N_TILES, 4 * N_TILES))
    g = ren.mc_layers_fixed()
    assert ren.mc_stats() == stats and ren.mc_coverage() == [(0, 4 * N_TILES)]
    ren.close()
    assert not np.array_equal(before, layers)
    _layers_equal(g, layers)
    assert np.array_equal(four.view(np.uint32), words_to_float(layers.sum(0), 4).view(np.uint32))


# ---- 5. the range rule
def _bright_door(tmp_path):
    """tests/test_gpu_mc_exact.py's construction over the layered oracle: veach-door with the emitter's radiance scaled up until the oracle drops some,
    not all, contributions by the range rule"""
    src = open(VEACH).read()
    line = '<rgb name="radiance" value="1420 1552 1642"/>'
    assert src.count(line) == 1
    os.symlink(os.path.join(os.path.dirname(VEACH), "data"), tmp_path / "data")
    for k, factor in enumerate((1e8, 1e9, 1e7, 1e10, 1e6)):
        p = tmp_path / ("door_x%d.xml" % k)
        p.write_text(src.replace(line, '<rgb name="radiance" value="%r %r %r"/>' % (1420 * factor, 1552 * factor, 1642 * factor)))
        drops = [scene_oracle("veachdoor", LENGTH, 2, 7, b, xml=str(p))[2:4] for b in (True, False)]
        if all(0 < dropped < counted for counted, dropped in drops):
            return str(p), factor
    raise AssertionError("no factor makes the layered oracle drop some but not all contributions")


def test_range_rule_drops_a_contribution_from_its_own_layer_only(tmp_path):
    xml, factor = _bright_door(tmp_path)
    for bidir in (True, False):
        ren = _renderer("veachdoor", 7, bidir, LENGTH, xml=xml)
        min_depth = int(ren.get_option("mindepth"))
        o, op, on, odrop, outside = scene_oracle("veachdoor", LENGTH, 2, 7, bidir, min_depth, xml=xml)
        print("radiance x %g, bidir=%d: oracle %d contributions, %d dropped" % (factor, bidir, on, odrop))
        assert 0 < odrop < on and outside == 0, (odrop, on)
        ren.mc_render(2)
        g, total, (gp, gn), gov = ren.mc_layers_fixed(), ren.mc_film_fixed(), ren.mc_stats(), ren.mc_overflow()
        ren.close()
        assert (gp, gn, gov) == (op, on, odrop), (gp, gn, gov, op, on, odrop)
        _layers_equal(g, o)  # every layer equal: what the oracle dropped is missing from its own layer, and from no other
        assert np.array_equal(total, o.sum(0))


# ---- 6. float mode
@pytest.mark.parametrize("name,bidir,mode", [("veachdoor", True, TECHNIQUE), ("torus_materials", True, LENGTH), ("torus_lambert", False, TECHNIQUE)])
def test_float_layers(name, bidir, mode):
    seed_offset, spp = SAMPLES[1]
    ren = _renderer(name, seed_offset, bidir, mode, exact=False)
    min_depth = int(ren.get_option("mindepth"))
    img = ren.mc_render(spp)
    layers, film, stats = ren.mc_layers(), ren.mc_film(), ren.mc_stats()
    with pytest.raises(RuntimeError, match="float mode"):
        ren.mc_layer_fixed(0)
    ren.set_option("mc_layers", 0)
    plain = ren.mc_render(spp)
    assert ren.mc_stats() == stats
    ren.close()
    o, op, on, odrop, outside = scene_oracle(name, mode, spp, seed_offset, bidir, min_depth)
    assert stats == (op, on) and layers.dtype == np.float32 and layers.shape == o.shape
    filled = 0
    for k in range(len(o)):
        if o[k].any():
            _film_close(layers[k], words_to_float(o[k], spp))
            filled += 1
        else:
            assert not layers[k].any(), k  # exactly zero
    assert filled >= 2
    want = np.zeros_like(film)
    for k in range(len(layers)):  # float adds in increasing layer index
        want = want + layers[k]
    assert np.array_equal(film.view(np.uint32), want.view(np.uint32)) and np.array_equal(img.view(np.uint32), film.view(np.uint32))
    _film_close(film, plain)


# ---- 7. refusals
def test_refusals_name_mc_layers_and_leave_the_contexts_usable(tmp_path):
    p = gc.pkg()
    rens = [_renderer("torus_lambert", 7, True, LENGTH) for _ in range(2)]
    rens[0].mc_render(4)
    layers, total = rens[0].mc_layers_fixed(), rens[0].mc_film_fixed()
    path = str(tmp_path / "layered.mcfx")
    with pytest.raises(RuntimeError, match="mc_layers"):
        rens[0].mc_save(path)
    assert not os.path.exists(path) and not os.path.exists(path + ".tmp")
    with pytest.raises(RuntimeError, match="mc_layers"):
        p.Group(rens).mc_render(4)
    with pytest.raises(RuntimeError, match="mc_layers"):
        p.Group(rens).mc_accumulate(4)
    for bad in (-1, len(layers), 1000):
        with pytest.raises(RuntimeError, match="layer %d outside" % bad):
            rens[0].mc_layer_fixed(bad)
        with pytest.raises(RuntimeError, match="layer %d outside" % bad):
            rens[0].mc_layer(bad)
    with pytest.raises(RuntimeError, match="mc_layers"):
        rens[0].set_option("mc_layers", 3)
    assert np.array_equal(rens[0].mc_layers_fixed(), layers) and not rens[1].mc_coverage()  # nothing was rendered or changed
    for r in rens:
        r.set_option("mc_layers", 0)
    img = p.Group(rens).mc_render(4)
    assert np.array_equal(rens[0].mc_film_fixed(), total) and rens[0].mc_layer_info() == (0, [])
    assert np.array_equal(img.view(np.uint32), words_to_float(total, 4).view(np.uint32))
    rens[0].mc_save(path)
    rens[1].set_option("mc_layers", TECHNIQUE)
    with pytest.raises(RuntimeError, match="mc_layers"):
        rens[1].mc_load(path)
    rens[1].set_option("mc_layers", 0)
    rens[1].mc_load(path)
    assert np.array_equal(rens[1].mc_film_fixed(), total)
    for r in rens:
        r.close()


# ---- 8. dpt_amd
def test_dpt_amd_writes_the_non_empty_layers_beside_the_image(tmp_path):
    scene = _mc_scene(tmp_path)
    p = gc.pkg()
    ren = p.Renderer(scene, seed_offset=0, use_gradient=0)
    ren.set_option("mc_layers", LENGTH)
    ren.mc_render(4)
    layers, lengths = ren.mc_layers(), [L for L, _ in ren.mc_layer_info()[1]]
    ren.close()
    r = subprocess.run([CLI, "--mc-layers", "length", scene], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("Done!"), r.stdout
    exrs = [f for f in os.listdir(tmp_path) if f.endswith(".exr")]
    main = [f for f in exrs if re.fullmatch(r"lmc_timeuse_[0-9]+\.[0-9]{6}s\.exr", f)]
    assert len(main) == 1, exrs
    want = {main[0][:-4] + "_L%02d.exr" % L for L, l in zip(lengths, layers) if l.any()}
    assert len(want) >= 5 and set(exrs) - {main[0]} == want, (sorted(exrs), sorted(want))
    img = p.read_image(str(tmp_path / main[0]))
    total = sum(p.read_image(str(tmp_path / f)) for f in sorted(want))
    assert img.shape == (48, 64, 3) and img.max() > 0
    assert np.allclose(total, img, rtol=2e-3, atol=1e-4 * img.max()), np.abs(total - img).max()  # half floats
    # the flag on an mcmc scene: refused, the integrator named
    r = subprocess.run([CLI, "--mc-layers", "technique", gc.TORUS], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode != 0 and "integrator=mcmc" in r.stdout and "--mc-layers" in r.stdout, r.stdout
