"""Lamps in the path model (tests/lamp_model.py), on the CPU: path_model's walker with the lamps' light sample in
place draws every kind of lamp and reaches its guards, alone, beside emitters and under an environment map; and a sun lamp lights a
scene as one texel of a map does wherever the camera's hit sees the whole texel or none of it (hip_checks.z_grid's bounds) -- and
not in the texel's penumbra, which test_sun_is_one_texel_away_from_shadow_edges measures."""
import numpy as np
import pytest

import env_model
import hip_checks as hc
import lamp_model as lm
import path_model
from oracle import oracle as O
from path_model import F
from spath_amd import scene

SPP, SEED = 4, 3


def case(name):
    lamps = scene.lamp_table(scene.point_lamp((1.0, 1.5, -1.5), (6.0, 5.0, 4.0)),
                             scene.spot_lamp((-2.0, 2.2, -2.0), (0.5, -1.0, -0.3), (40.0, 36.0, 30.0), 25, 50))
    env = None
    if name == "sky+sun":
        t, m = scene.open_clutter(100)
        env = env_model.replay_maps()["sky64"]
        lamps = scene.lamp_table(scene.sun_lamp((0.3, -0.8, -0.5), (3.0, 2.8, 2.4)))
    else:
        t, m = scene.closed_room(300)
        if name == "lamps_only":
            m = m.copy()
            m[:, 3:6] = 0
    return t, m, env, lamps


@pytest.mark.parametrize("name", ["room", "lamps_only", "sky+sun"])
def test_walker_draws_lamps(name):
    """the lamps are drawn, give samples and are cut by their guards; the image differs from the one without lamps; a room without
    emitters has a non-empty table and renders"""
    t, m, env, lamps = case(name)
    counts = {}
    rgba, mean, scans, info = lm.render(hc.rays(), t, m, SPP, SEED, "mis", lamps, env=env, counts=counts)
    assert counts["lamp_draws"] > 1000 and counts["sample"] > 500 and counts["cos_x"] > 0, counts
    if name == "sky+sun":
        assert counts["lamp_sun"] == counts["lamp_draws"], counts
    else:
        assert counts["lamp_point"] > 0 and counts["lamp_spot"] > 0 and counts["falloff"] > 0, counts
    plain = path_model.render(hc.rays(), t, m, SPP, SEED, "mis", env=env)
    assert not np.array_equal(mean, plain[1]) and scans > 0 and np.isfinite(mean).all()
    if name == "lamps_only":
        assert scene.light_table(t, m)[0].size == 0 and not plain[1].any() and mean.any()
    # black lamps add no entry: the model's render is path_model's, bit for bit
    z = lamps.copy()
    z[:, 4:7] = 0
    off = lm.render(hc.rays(), t, m, SPP, SEED, "mis", z, env=env)
    assert np.array_equal(off[1], plain[1]) and off[2] == plain[2]


def test_lamps_need_mis():
    t, m, env, lamps = case("room")
    for est in ("plain", "nee"):
        with pytest.raises(ValueError):
            lm.samples(hc.rays(), t, m, SEED, 0, 1, est, lamps)


def _one_texel(n=1024, i=666, j=386, Le=(3.2e5, 2.9e5, 2.4e5)):
    """a map that is black but for texel (i, j), and the sun lamp of the same light: a = minus the texel's centre direction,
    c = Le x the texel's solid angle, in float64 from the map model's own weights (wt = Lsum / r3 per texel, times da db = 4 / n^2)"""
    env = np.zeros((n, n, 3), F)
    env[j, i] = Le
    tab = env_model.tables(env)
    lsum = float(np.asarray(Le, F).astype(np.float64).sum())
    omega = tab["wt"][j, i] / lsum * (4.0 / (float(n) * n))
    a, b = -1.0 + (2.0 * i + 1.0) / n, -1.0 + (2.0 * j + 1.0) / n
    y = 1.0 - abs(a) - abs(b)
    assert y > 0.2 and abs(tab["Phi"] - lsum * omega) < 1e-12 * tab["Phi"]
    d = np.array([a, y, b]) / np.sqrt(a * a + y * y + b * b)
    assert np.hypot(d[0], d[2]) > 0.4                             # well away from the vertical
    li, lj, _, ok = env_model.lookup(d[None].astype(F), n)
    assert ok[0] and (li[0], lj[0]) == (i, j)                     # the sun's direction is the texel's, in the map model's own lookup
    return env, scene.lamp_table(scene.sun_lamp(-d, np.asarray(Le, F).astype(np.float64) * omega))


def _penumbra_pixels(rays, t, n, i, j):
    """the pixels whose camera hit sees texel (i, j) of an n x n map partly: the shadow rays from the hit towards the texel's centre and
    its four corners do not all agree -> bool [npix].  Decided by geometry alone, before anything is rendered"""
    idx, dist = O.closest_hits(rays, t, np.full(rays.shape[0], -1, np.int32))
    x = (rays[:, :3] + rays[:, 3:] * dist[:, None]).astype(F)
    k = np.full(rays.shape[0], 1)
    occ = []
    for ra, rb in ((0.5, 0.5), (0, 0), (0, 1), (1, 0), (1, 1)):
        wd, _ = env_model.place(i * k, j * k, ra * k, rb * k, n)
        occ.append(O.closest_hits(np.concatenate([x, wd], 1).astype(F), t, idx.astype(np.int32))[0] >= 0)
    occ = np.stack(occ)
    return (idx >= 0) & (occ.any(0) != occ.all(0))


def test_sun_is_one_texel_away_from_shadow_edges():
    """open_clutter(100) lit by a sun lamp and by a map whose only non-zero texel (n = 1024) is that sun, both under NEE|MIS in the
    numpy models, 16 seeds x 8 spp at 32 x 32, under hip_checks.z_grid's bounds (|z| < 4 for the image, < 5 per cell) -- over the
    pixels whose camera hit sees the whole texel or none of it.

    Why the mask, and what it says about the issue's expectation test.  The two lightings are NOT one image pixel by pixel.  The
    primary ray of a pixel is fixed (no camera samples), so its first hit is one point; where that point lies in the texel's penumbra
    the map lights it partly and the lamp fully or not at all: a difference of order one at that pixel, not a second-order bias.  The
    penumbra is as wide as the texel, so the number of such pixels falls as 1 / n and never reaches zero at a map size the library
    takes (n <= 2048): 10 of 866 camera hits at n = 1024 here.  Both renders share their seeds, hence their paths, so the noise of
    their difference is small and a handful of such pixels decides z.  Measured with these models, unmasked (z(image); cells beyond
    5): n = 256: 2 spp -3.70, none; 8 spp -3.74, four cells of 5.5 to 9.2; 32 spp -8.33, cells to +17.9 and -17.2.  n = 1024: 2 spp
    -0.80, none; 8 spp +0.65, cells -9.10 and +9.30; 32 spp +0.74, cells -17.4 and +27.4.  n = 2048: 2 spp +1.09, none; 8 spp +2.99,
    cells +7.85 and +5.05; 32 spp +4.66, cells +8.23 and +19.2.  So a pass at few samples shows nothing, and the unmasked comparison
    the issue asks of the GPU (n = 256, 16 x 256 spp) cannot hold at any n.  With the penumbra pixels left out (they are chosen by
    geometry: five shadow rays per camera hit, before anything is rendered) z stays flat as the samples grow, n = 1024: 2 spp -0.50
    (largest cell 1.74), 8 spp +0.76 (2.50), 32 spp -0.42 (3.07).  That is the statement this test holds: away from the shadow edges of
    the camera's own hits the (2 / pi) / sxz factor of lamp_light makes a lamp the limit of the texel; at deeper bounces the hit
    point is itself random and the penumbra is the second-order term it was taken for."""
    n, i, j = 1024, 666, 386
    t, m = scene.open_clutter(100)
    env, lamps = _one_texel(n, i, j)
    w = h = 32
    rays = hc.rays(w, h)
    edge = _penumbra_pixels(rays, t, n, i, j)
    assert 0 < edge.sum() <= 0.02 * edge.size, edge.sum()
    seeds = range(500, 516)
    a = np.stack([lm.render(rays, t, m, 8, s, "mis", lamps)[1].astype(np.float64) for s in seeds])
    b = np.stack([path_model.render(rays, t, m, 8, s, "mis", env=env)[1].astype(np.float64) for s in seeds])
    u = path_model.render(rays, t, m, 8, 500, "mis")[1]
    assert not np.array_equal(u, a[0].astype(F)) and not np.array_equal(u, b[0].astype(F))
    # the disagreement sits in the penumbra pixels: some differ by a good part of the sun's light there
    dd = (a - b).mean(0).sum(-1)
    assert np.abs(dd[edge]).max() > 0.1, np.abs(dd[edge]).max()
    a[:, edge] = 0
    b[:, edge] = 0
    hc.z_grid(a, b, h, w, "model, penumbra pixels left out: sun lamp vs one texel at n = 1024, seeds 500..515", alike_is_zero=True)
