"""The environment map on the CPU (include/spath_hip.h "environment lighting"): the numpy statement of the octahedral
mapping and of the importance tables (tests/env_model.py) against what it must mean, and the scene.py helpers.  The device side is held to
the same model at tolerance 0 in tests/test_hip_environment.py."""
import hashlib
import json
import os
import struct

import numpy as np
import pytest

import env_model as em
import path_model
from hip_checks import mixed_table
from path_model import F
from spath_amd import capi, scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRAWS = 2_000_000
# the share of uniform (texel, r3, r4) draws whose direction env_lookup gives to another texel, measured over DRAWS draws with seed 1:
# n = 64: 7 draws, 3.5e-6 (seeds 2, 3: 9 and 5); n = 2, 3: none.  The bar is 8 x the measured share rounded up to a power of two (DESIGN.md
# section 5.10's rule): 2.8e-5 -> 2^-15 at n = 64; where nothing was measured, 8 x the measurement's resolution 1 / DRAWS -> 2^-17.  n = 1
# has one texel: every direction is clamped into it
SHARE_BAR = {1: 0.0, 2: 2.0 ** -17, 3: 2.0 ** -17, 64: 2.0 ** -15}


def test_symbols_and_selftest_shapes():
    for name in ("sphip_set_environment", "sphip_set_environment_device", "sphip_selftest_env_dump"):
        assert name in capi.SYMBOLS
    assert capi.Context.SELFTEST_OUT[9] == ("float32", 4) and capi.Context.SELFTEST_OUT[10] == ("float32", 6)


def test_lookup_by_hand():
    """4 x 4: +y is the centre (the texel right of and above the middle, a = b = +0), the axes +-x and +-z the middles of the square's
    sides, -y the corners; the answer does not depend on the length of d; a zero, an infinite or a NaN direction has no texel"""
    d = np.array([[0, 1, 0], [1, 0, 0], [-1, 0, 0], [0, 0, 1], [0, 0, -1],
                  [0.1, -1, 0.1], [-0.1, -1, 0.1], [0.1, -1, -0.1], [-0.1, -1, -0.1],
                  [0, 0, 0], [np.nan, 1, 0], [np.inf, 0, 0], [1, -0.0, 0.25]], F)
    i, j, r3, ok = em.lookup(d, 4)
    assert ok.tolist() == [True] * 9 + [False] * 3 + [True]
    assert list(zip(i.tolist(), j.tolist()))[:9] == [(2, 2), (3, 2), (0, 2), (2, 3), (2, 0), (3, 3), (0, 3), (3, 0), (0, 0)]
    assert (i[12], j[12]) == (3, 2)                           # d.y = -0 is the upper half: (a, b) = (0.8, 0.2)
    assert r3[0] == 1 and r3[1] == 1 and not r3[9:12].any()
    for k in (-20, 20):
        for got, want in zip(em.lookup(d * F(2.0 ** k), 4), (i, j, r3, ok)):
            assert np.array_equal(got, want)
    # the diagonal folds: the face centres of the octahedron, |p|^3 = 3^-1.5 on every one
    f = np.array([[sx, sy, sz] for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)], F)
    i, j, r3, ok = em.lookup(f, 4)
    assert ok.all() and np.allclose(r3, 3.0 ** -1.5, rtol=1e-6)
    assert list(zip(i.tolist(), j.tolist())) == [(2, 2), (2, 1), (3, 3), (3, 0), (1, 2), (1, 1), (0, 3), (0, 0)]


def test_place_and_lookup_agree_with_the_geometry():
    """the centre of every texel: place() gives a unit direction that lookup() returns to the same texel, equal (to f32 rounding) to
    scene.octahedral_directions, and r3 is the same on both ways"""
    n = 16
    jj, ii = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    wd, r3 = em.place(ii.ravel(), jj.ravel(), np.full(n * n, 0.5), np.full(n * n, 0.5), n)
    assert np.allclose(wd, scene.octahedral_directions(n).reshape(-1, 3), atol=1e-6)
    assert np.allclose(em._dot3(wd, wd), 1, atol=1e-6)
    i, j, r3b, ok = em.lookup(wd, n)
    assert ok.all() and np.array_equal(i, ii.ravel()) and np.array_equal(j, jj.ravel())
    assert np.allclose(r3, r3b, rtol=1e-5)


def test_the_jacobian_covers_the_sphere():
    """da db = r3 d omega: the texels' solid angles (4 / n^2) / |g_c|^3 add up to 4 pi.  Midpoint rule at h = 2 / 256: the error is
    h^2 / 24 = 2.5e-6 times the integrand's second derivatives, which stay below 100 (the integrand is between 1 and 3^1.5, smooth on each
    of the eight faces): 1e-3 relative"""
    n = 256
    tx = np.zeros((n, n, 3), F)
    tx[..., 0] = 1
    tab = em.tables(tx)
    omega = tab["wt"] * (4.0 / (n * n))
    assert abs(omega.sum() / (4 * np.pi) - 1) < 1e-3
    assert abs(tab["Phi"] / (4 * np.pi) - 1) < 1e-3      # Phi: the map's power per unit area for radiance summing to 1


def test_tables_are_sequential_sums():
    rng = np.random.default_rng(5)
    for n in (1, 2, 3, 5):
        tx = rng.random((n, n, 3)).astype(F)
        tab = em.tables(tx)
        run = 0.0
        for j in range(n):
            s = 0.0
            for i in range(n):
                s = s + tab["wt"][j, i]
                assert tab["rc"][j, i] == s
            run = run + s
            assert tab["marg"][j] == run
        assert tab["T"] == run


def test_tpdf_is_a_density():
    """tpdf is the selection probability w_env / W times a density per unit (a, b) area: its integral over the square is w_env / W up to
    the f32 rounding of each texel (2^-24 relative, 2^-23 allowed for the double sums beside it)"""
    t, m = scene.open_clutter(100)
    tab = em.tables(scene.sky_environment(64))
    sp = em.scene_part(tab, t, m)
    assert 0 < sp["w_env"] < sp["W"]
    sel = sp["w_env"] / sp["W"]
    assert abs(sp["tpdf"].astype(np.float64).sum() * (4.0 / 64 ** 2) / sel - 1) < 2.0 ** -23
    black = em.tables(np.zeros((3, 3, 3), F))
    sp0 = em.scene_part(black, t, m)
    assert black["T"] == 0 and sp0["w_env"] == 0 and sp0["W"] == scene.light_table(t, m)[3] and not sp0["tpdf"].any()


def test_one_lit_texel_takes_every_sample():
    """a map black but for texel (3, 2) of 5 x 5: black rows and leading black texels are never chosen, r8 = r9 = 0 included"""
    tx = np.zeros((5, 5, 3), F)
    tx[2, 3] = (1, 2, 3)
    tab = em.tables(tx)
    rng = np.random.default_rng(11)
    u = rng.random((4, 10_000))
    u[:, 0] = 0.0
    u[0:2, 1] = np.nextafter(1.0, 0.0)
    i, j, wd, _ = em.sample(tab, *u)
    assert (i == 3).all() and (j == 2).all()
    li, lj, _, ok = em.lookup(wd, 5)
    assert ok.all() and (li == 3).all() and (lj == 2).all()


def test_samples_follow_the_map():
    """the share of samples per texel is wt / T: chi-square over the 9 texels of a 3 x 3 map with 10^5 draws, 8 degrees of freedom; the
    bar 40 is the 1 - 3e-6 quantile"""
    rng = np.random.default_rng(2)
    tab = em.tables(rng.random((3, 3, 3)).astype(F))
    i, j, _, _ = em.sample(tab, *rng.random((4, 100_000)))
    cnt = np.bincount(j * 3 + i, minlength=9).astype(np.float64)
    exp = (tab["wt"] / tab["T"]).ravel() * 100_000
    assert ((cnt - exp) ** 2 / exp).sum() < 40


@pytest.mark.parametrize("n", [1, 2, 3, 64])
def test_sample_then_lookup_names_the_same_texel(n):
    share = em.roundtrip_share(n, DRAWS, 1)
    print(f"n = {n}: {share * DRAWS:.0f} of {DRAWS} draws come back to another texel ({share:.2e}); bar {SHARE_BAR[n]:.2e}")
    assert share <= SHARE_BAR[n]


def test_model_digests():
    """the model's own bits, pinned: the tables of the sky map at n = 64 under open_clutter(100), and 1000 samples from them"""
    t, m = scene.open_clutter(100)
    tab = em.tables(scene.sky_environment(64))
    sp = em.scene_part(tab, t, m)
    i, j, wd, r3 = em.sample(tab, *np.random.default_rng(3).random((4, 1000)))
    h = hashlib.sha256()
    for a in (tab["wt"], tab["rc"], tab["marg"], sp["tpdf"], np.array([tab["T"], sp["w_env"], sp["W"]]), i, j, wd, r3):
        h.update(np.ascontiguousarray(a).tobytes())
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "env_model_digests.json")))
    assert h.hexdigest() == want["sky64_open_clutter_100"]


def test_scene_helpers(tmp_path):
    sky = scene.sky_environment(64)
    assert sky.dtype == F and sky.shape == (64, 64, 3) and np.isfinite(sky).all() and (sky >= 0).all()
    sun = sky.sum(-1) > 50
    assert 0 < sun.sum() < 64                                  # a few texels
    d = scene.octahedral_directions(64)[sun]
    sd = np.array([0.3, 0.8, 0.5]) / np.linalg.norm([0.3, 0.8, 0.5])
    assert (d @ sd >= np.cos(0.1)).all()
    assert np.array_equal(sky[0, 0], np.array([0.15, 0.12, 0.1], F))            # a corner looks down: the ground
    p = tmp_path / "env.bin"
    scene.write_environment(p, sky)
    raw = p.read_bytes()
    assert raw[:4] == b"SPEN" and struct.unpack("<I", raw[4:8])[0] == 64 and raw[8:] == sky.tobytes()
    with pytest.raises(ValueError):
        scene.write_environment(p, np.zeros((4, 5, 3), F))
    with pytest.raises(ValueError):
        scene.sky_environment(4, sky_radiance=(-1, 0, 0))
    # a lat-long image: a constant stays one; an upper half lights the centre diamond, the zenith row the centre
    assert np.allclose(scene.environment_from_latlong(np.full((8, 16, 3), 0.25), 8), 0.25)
    img = np.zeros((16, 32, 3))
    img[:8] = 1.0
    e = scene.environment_from_latlong(img, 8)
    up = scene.octahedral_directions(8)[..., 1]
    assert (e[up > 0.3] == 1).all() and (e[up < -0.3] == 0).all()
    # azimuth: a patch around +x (column w / 4 by the docstring: atan2(1, 0) = pi / 2 -> u = 1 / 4) lands where lookup sends +x
    img = np.zeros((16, 32, 3))
    img[6:10, 6:10] = 1.0
    e = scene.environment_from_latlong(img, 8)
    i, j, _, _ = em.lookup(np.array([[1, 0.02, 0.02]], F), 8)
    assert e[j[0], i[0], 0] == 1 and e.sum() < 8 * 3


# ---------------------------------------------------------------------------------------------------------------- the path model
def _rays():
    from spath_amd import view
    cam = view.Camera(48, 32)
    cam.set_delta_mov((0.1, -0.2, 0.3))
    cam.set_delta_rot((0.05, 0.1, 0.0))
    return np.ascontiguousarray(cam.get_viewport(), dtype=F)


@pytest.mark.parametrize("est", ["plain", "mis"])
@pytest.mark.parametrize("tables", [False, True])
def test_black_map_is_no_map(tables, est):
    """an all-zero map (which executes the specular and the dielectric step against tables of zeros and every environment step against
    a map without an entry) changes nothing: the bits, images and scans, of the call without a map"""
    t, m, s, vn, _ = em.replay_scene("open", tables, mixed_table)
    r = _rays()
    want = path_model.render(r, t, m, 4, 3, est, s, vn)
    got = path_model.render(r, t, m, 4, 3, est, s, vn, env=np.zeros((3, 3, 3), F))
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)) and got[2] == want[2]


@pytest.mark.parametrize("est", ["plain", "mis"])
@pytest.mark.parametrize("tables", [False, True])
@pytest.mark.parametrize("mp", ["n3", "sky64"])
@pytest.mark.parametrize("name", ["glass", "open"])
def test_path_digests_and_coverage(name, mp, tables, est):
    """the replay cases of tests/test_hip_environment.py: every rule fires, and the model's images are pinned"""
    t, m, s, vn, g = em.replay_scene(name, tables, mixed_table)
    img, mean, scans, info = path_model.render(_rays(), t, m, 4, 3, est, s, vn, g, em.replay_maps()[mp])
    em.covered(info, name, tables, est)
    h = hashlib.sha256(mean.tobytes() + img.tobytes() + struct.pack("<Q", scans)).hexdigest()
    key = f"path_{name}_{mp}_{'tables' if tables else 'bare'}_{est}"
    if os.environ.get("SPATH_PRINT_DIGESTS"):
        print("DIGEST", key, h)
        return
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "env_model_digests.json")))
    assert h == want[key]
