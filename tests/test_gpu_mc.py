"""`-m gpu` tier: the "mc" integrator (lmc_mc_render, device/mc.hip; PathTrace, pathtrace.cpp:14-78) against its CPU oracle
(tests/helpers/mc_oracle.cpp), against the reference's own loop and images, sharded, through dpt_amd, and beside the estimators that were
there before it."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import gpu_checks as gc
from tests.test_mc_abi import oracle_mc

pytestmark = pytest.mark.gpu
CLI = os.path.join(gc.ROOT, "langevin-mcmc_amd", "dpt_amd")
VEACH = os.path.join(gc.ROOT, "scenes", "veachdoor", "lmc.xml")

# (scene, force_diffuse, max_depth override, width, height)
SCENES = {
    "torus_lambert": (gc.TORUS, 1, 6, 64, 48),
    "torus_materials": (gc.TORUS, 0, 8, 64, 48),
    "veachdoor": (VEACH, 0, 0, 80, 45),
}


def _film_close(g, o):
    """the same image up to the order of the float adds (the splats are atomics): the chain tests' film bar, and per pixel"""
    assert o.sum() > 0 and np.isfinite(g).all()
    assert np.linalg.norm(g - o) <= 1e-5 * np.linalg.norm(o), np.linalg.norm(g - o) / np.linalg.norm(o)
    assert np.allclose(g, o, rtol=1e-4, atol=1e-6 * o.max()), np.abs(g - o).max()


def _renderer(name, seed_offset, bidir):
    xml, fd, md, W, H = SCENES[name]
    ren = gc.pkg().Renderer(xml, force_diffuse=fd, max_depth=md, width=W, height=H, seed_offset=seed_offset, use_gradient=0)
    ren.set_option("bidirectional", 1 if bidir else 0)
    return ren


@pytest.mark.parametrize("name", list(SCENES))
@pytest.mark.parametrize("bidir", [True, False])
def test_mc_render_matches_the_oracle(name, bidir):
    xml, fd, md, W, H = SCENES[name]
    for seed_offset, spp in ((0, 2), (7, 3)):
        ren = _renderer(name, seed_offset, bidir)
        assert ren.get_option("bidirectional") == (1 if bidir else 0)
        min_depth = int(ren.get_option("mindepth"))
        g = ren.mc_render(spp)
        gp, gn = ren.mc_stats()
        ren.close()
        o, op, on = oracle_mc(xml, spp, force_diffuse=fd, max_depth=md, width=W, height=H, seed_offset=seed_offset, min_depth=min_depth, bidir=bidir)
        assert gp == op == W * H * spp, (gp, op)
        assert gn == on, (name, bidir, seed_offset, gn, on)
        _film_close(g, o)


@pytest.mark.parametrize("bidir", [True, False])
def test_mc_render_is_the_reference_loop_at_one_sample(bidir):
    """spp = 1, seedoffset 0: the reference's PathTrace loop as written (one RNG(tileIndex) per tile)"""
    ren = _renderer("torus_materials", 0, bidir)
    g = ren.mc_render(1)
    gp, gn = ren.mc_stats()
    ren.close()
    xml, fd, md, W, H = SCENES["torus_materials"]
    o, op, on = oracle_mc(xml, 1, force_diffuse=fd, max_depth=md, width=W, height=H, seed_offset=0, bidir=bidir, literal=True)
    assert gp == op and gn == on, (gp, op, gn, on)
    _film_close(g, o)


def test_mc_stream_ranges_sum_to_the_whole_render():
    ren = _renderer("torus_lambert", 7, True)
    spp, nTiles = 4, 4 * 3
    full = ren.mc_render(spp)
    full_stats = ren.mc_stats()
    a = ren.mc_render(spp, streams=(0, 17))
    sa = ren.mc_stats()
    b = ren.mc_render(spp, streams=(17, -1))
    sb = ren.mc_stats()
    ren.close()
    assert sa[0] + sb[0] == full_stats[0] == 64 * 48 * spp and sa[1] + sb[1] == full_stats[1]
    _film_close(a + b, full)
    assert nTiles * spp > 17


def _mc_scene(tmp_path, width=64, height=48, spp=4, extra=None):
    """scenes/torus/lmc.xml with integrator = mc and a small film"""
    xml = open(gc.TORUS).read()
    xml = xml.replace('<string  name="integrator"     value="mcmc"/>', '<string name="integrator" value="mc"/>')
    xml = xml.replace('<integer name="height" value="768"/>', '<integer name="height" value="%d"/>' % height)
    xml = xml.replace('<integer name="width" value="1024"/>', '<integer name="width" value="%d"/>' % width)
    xml = re.sub(r'<integer name="spp"\s+value="245"/>', '<integer name="spp" value="%d"/>' % spp, xml)
    if extra:
        for a, b in extra:
            assert a in xml, a
            xml = xml.replace(a, b)
    assert 'value="mc"' in xml and 'value="%d"' % width in xml and 'name="spp" value="%d"' % spp in xml
    if not os.path.exists(tmp_path / "data"):
        os.symlink(os.path.join(gc.ROOT, "scenes", "torus", "data"), tmp_path / "data")
    p = tmp_path / "mc.xml"
    p.write_text(xml)
    return str(p)


def _run_cli(args, tmp_path):
    for f in os.listdir(tmp_path):
        if f.endswith(".exr"):
            os.remove(tmp_path / f)
    r = subprocess.run([CLI] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout
    assert re.search(r"Elapsed time:[0-9.eE+-]+", r.stdout), r.stdout
    assert r.stdout.rstrip().endswith("Done!"), r.stdout
    exrs = [f for f in os.listdir(tmp_path) if re.fullmatch(r"lmc_timeuse_[0-9]+\.[0-9]{6}s\.exr", f)]
    assert len(exrs) == 1, os.listdir(tmp_path)
    return r.stdout, gc.pkg().read_image(str(tmp_path / exrs[0]))


def test_dpt_amd_renders_an_mc_scene(tmp_path):
    """an mc scene with the reference's defaults mala = h2mc = false (the combination an mcmc scene is refused with)"""
    scene = _mc_scene(tmp_path, extra=[('<boolean name="mala"           value="true"/>', '<boolean name="mala" value="false"/>')])
    p = gc.pkg()
    ren = p.Renderer(scene, seed_offset=0, use_gradient=0)
    assert ren.get_option("integrator_mc") == 1 and ren.get_option("bidirectional") == 1
    assert ren.get_option("mala") == 0 and ren.get_option("h2mc") == 0
    want = ren.mc_render(4)
    ren.close()
    shipped = p.Renderer(gc.TORUS, width=64, height=48, use_gradient=0)
    assert shipped.get_option("integrator_mc") == 0
    shipped.close()
    out, img = _run_cli([scene], tmp_path)
    assert img.shape == (48, 64, 3) and np.isfinite(img).all()
    # the EXR holds half floats
    half = want.astype(np.float16).astype(np.float32)
    assert np.allclose(img, half, rtol=2e-3, atol=1e-4 * want.max()), np.abs(img - half).max()
    # two shards on one device: the same image
    out2, img2 = _run_cli(["--devices", "0,0", "--chains", "1024", scene], tmp_path)
    assert "ignored by integrator=mc" in out2 and "sharded over 2 devices" in out2
    assert np.allclose(img2, img, rtol=2e-3, atol=1e-4 * want.max())


def test_dpt_amd_mc_scene_with_mala_runs_path_trace(tmp_path):
    """integrator = mc wins over mala = true (main.cpp:92-96; the shipped file's value): PathTrace, not MLT -- no "Average brightness:" line,
    the mc image"""
    scene = _mc_scene(tmp_path)
    ren = gc.pkg().Renderer(scene, seed_offset=0, use_gradient=0)
    assert ren.get_option("mala") == 1
    want = ren.mc_render(4)
    ren.close()
    out, img = _run_cli([scene], tmp_path)
    assert "Average brightness" not in out
    assert np.allclose(img, want.astype(np.float16).astype(np.float32), rtol=2e-3, atol=1e-4 * want.max())


def _lum(x):
    return x.astype(np.float64) @ np.array([0.212671, 0.715160, 0.072169])


def _relmse(a, b):  # bench.py truth_crosscheck
    return float(((a - b) ** 2 / (b ** 2 + 0.01)).mean())


# At 16384 spp (2.5 s) the render's own noise is about the size of the difference between the reference's LMC and H2MC renders (relMSE 0.0055):
# measured relMSE 0.0094 (seedoffset 0) / 0.0104 (seedoffset 1) against the shipped render, 0.0135 between the two, 0.126 / 0.032 at 1024 / 4096 spp
# (a 1 / spp fall: noise, no bias); mean ratio 1.015 at every count -- the shipped render's own normaliser, the offset bench.py's truth_crosscheck
# sees with lmc_bidir_mc (profiles/r07_mc_vs_reference.jsonl).  The bars are twice the measured deviation, as the project sets its bars.
MC_VS_REF_SPP = 16384
MC_VS_REF_RELMSE_BAR = 2 * 0.0104
MC_VS_REF_MEAN_BAR = 2 * 0.0151


def test_mc_render_against_the_reference_image():
    """the shipped torus scene (full materials, maxdepth 8) through the mc integrator at 256 x 192 against the reference's own render of it
    (tests/golden/torus_ref_images_256x192.npz, 245 spp LMC, box-downsampled 4x)"""
    ref = np.load(os.path.join(gc.ROOT, "tests", "golden", "torus_ref_images_256x192.npz"))
    lr = _lum(ref["lmc"])
    ren = gc.pkg().Renderer(gc.TORUS, width=256, height=192, seed_offset=0, use_gradient=0)
    img = _lum(ren.mc_render(MC_VS_REF_SPP))
    ren.close()
    ratio, rel = float(img.mean() / lr.mean()), _relmse(img, lr)
    print("mc vs reference: mean ratio %.4f relMSE %.5f (lmc vs h2mc renders: %.5f)" % (ratio, rel, _relmse(_lum(ref["h2mc"]), lr)))
    assert abs(ratio - 1) < MC_VS_REF_MEAN_BAR and rel < MC_VS_REF_RELMSE_BAR, (ratio, rel)


def test_other_estimators_unchanged_by_an_mc_render():
    """lmc_bidir_mc, lmc_path_trace, lmc_direct_lighting and the chains' film: the same before and after an lmc_mc_render on the context"""
    p = gc.pkg()
    ren = p.Renderer(gc.TORUS, force_diffuse=1, max_depth=6, width=64, height=48, seed_offset=0, use_gradient=0)
    ren.init_chains(20000, 1024, 256, 8)
    ren.step(4)
    ren.sync()
    before = [ren.bidir_mc(16), ren.path_trace(8), ren.direct_lighting(8), ren.film()]
    ren.mc_render(4)
    chain_film = ren.film()
    after = [ren.bidir_mc(16), ren.path_trace(8), ren.direct_lighting(8)]
    ren.close()
    assert np.array_equal(chain_film, before[3])
    for a, b in zip(after, before[:3]):
        assert b.sum() > 0 and np.allclose(a, b, rtol=1e-5, atol=1e-7 * b.max())
