"""Textures (include/spath_hip.h: SPHIP_FLAG_TEXTURE with sphip_set_texture and sphip_set_uv): per-triangle
UVs and one bilinear RGB atlas on the context.  The albedo of a hit, rho * c, replaces the material's reflectance in the unwind's brdf
and in the hit's light sample, nowhere else.

The arithmetic is stated operation by operation in the header and restated in numpy (tests/texture_model.py).  STATED TOLERANCE: 0 --
the selftest, images, means and scan counts bit for bit.  The integrator is held to the one existing path model (tests/path_model.py)
through exact equivalences: where the four texels of a footprint are equal the sample is that texel bit for bit, so a render whose
triangles each see one tile of the atlas is the untextured render of the materials times the tiles' colours; the variation inside a
triangle is held by a first-hit closed form under a white 1 x 1 map.  The statistical bar is the project's (hip_checks.z_grid).

CPU part: the flag and the symbols; the model on constant footprints, under wrap, at the edges and against float64; the scene.py
helpers.  GPU part: the selftest; the tile equivalence for variants 1 and 16, both estimators; the first-hit closed form for variants
1, 8 and 16 in both shapes; zero UVs = no flag; the compositions; one expectation; the error contract; the front ends."""
import ctypes as C
import os

import numpy as np
import pytest

import env_model
import hip_checks as hc
import path_model
import texture_model as tm
from hip_checks import E_INVALID, E_STATE, ESTIMATORS, NEE_MIS, REPLAY_SEED, SPP, H, W, _torch_first, shape  # noqa: F401  (fixtures)
from oracle import oracle as O
from path_model import F, INV_P, INV_PI, _bits, _dot, _philox, _unit_vec
from spath_amd import capi, scene, view

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEX = capi.FLAG_TEXTURE
SPEC, GLOSSY, SMOOTH, GLASS, ENV = capi.FLAG_SPECULAR, capi.FLAG_GLOSSY, capi.FLAG_SMOOTH, capi.FLAG_DIELECTRIC, capi.FLAG_ENVIRONMENT
_MODEL = {}

# six colours, one per 8 x 8 tile of the 24 x 16 atlas of the tile equivalence
TILE_COLOURS = np.array([[0.9, 0.35, 0.2], [0.25, 0.8, 0.3], [0.3, 0.4, 0.95], [0.85, 0.8, 0.15], [0.6, 0.2, 0.7], [0.5, 0.55, 0.6]], F)
TILE_ATLAS = tm.tile_atlas(TILE_COLOURS, 8, 3)


# ---------------------------------------------------------------------------------------------------------------- scenes
def tile_uv(n):
    """triangle i sees tile i % 6 alone: three distinct UVs in the tile's central 4 x 4 texels, moved by whole repeats (s by i % 3 - 1,
    t by i % 2) so that the wrap runs too"""
    i = np.arange(n)
    k = i % 6
    c0, r0 = (k % 3) * 8.0, (k // 3) * 8.0
    uv = np.zeros((n, 6))
    for v, (a, b) in enumerate(((2.25, 2.5), (5.75, 2.25), (3.5, 5.75))):
        uv[:, 2 * v] = (c0 + a) / 24.0 + (i % 3 - 1)
        uv[:, 2 * v + 1] = (r0 + b) / 16.0 + (i % 2)
    return uv.astype(F)


def _random_rough(n, seed):
    return np.array([0, 0.05, 0.3, 1], F)[np.random.default_rng(seed).integers(0, 4, n)]


def case(name):
    """the scenes of the tile equivalence -> dict(t, m, s, vn, g, env, rough, uv): the plain room; the room with a mixed specular table
    and alpha in {0, 0.05, 0.3, 1}; the room with a smooth sphere, partly glass; the open clutter under the sky"""
    s = vn = g = env = rough = None
    if name == "room":
        t, m = scene.closed_room(300)
    elif name == "spec+rough":
        t, m = scene.closed_room(300)
        s = hc.mixed_table(t, m)
        rough = _random_rough(t.shape[0], 5)
    elif name == "glass+vn":                                  # the room's clutter is too small to be met: a smooth sphere in front
        t0, m0 = scene.closed_room(300)                       # of the camera, two of every three of its triangles glass
        ts, ms = scene.icosphere(1, (0.0, -0.2, -1.0), 0.5, (0.8, 0.7, 0.6, 0, 0, 0))
        t, m = np.concatenate([t0, ts]), np.concatenate([m0, ms])
        which = np.arange(300, t.shape[0])
        g = scene.dielectric_table(t, 1.5, (0.9, 0.95, 1.0), which=which[which % 3 != 0])
        vn = scene.vertex_normals(t, which=which)
    elif name == "env":
        t, m = scene.open_clutter(100)
        env = env_model.replay_maps()["sky64"]
    else:
        raise KeyError(name)
    return {"t": t, "m": m, "s": s, "vn": vn, "g": g, "env": env, "rough": rough, "uv": tile_uv(t.shape[0])}


CASES = ("room", "spec+rough", "glass+vn", "env")


def _flags(k):
    return hc.table_flags(k["s"], k["vn"], k["g"], k["env"], k["rough"])


def _ctx(k, devs=None, atlas=TILE_ATLAS, uv=True):
    c = hc.ctx(k["t"], k["m"], k["s"], k["vn"], devs, k["g"], k["env"], k["rough"])
    if atlas is not None:
        c.set_texture(atlas)
    if uv:
        c.set_uv(k["uv"])
    return c


def tiled_mats(k):
    """the materials whose untextured render the tile equivalence expects: rho times the colour of the triangle's tile, an f32 product"""
    m2 = k["m"].copy()
    m2[:, :3] = (k["m"][:, :3] * TILE_COLOURS[np.arange(m2.shape[0]) % 6]).astype(F)
    return m2


def _model(name, est):
    """the existing path model on the tiled materials, no texture step: computed once per case"""
    if (name, est) not in _MODEL:
        k = case(name)
        _MODEL[name, est] = path_model.render(hc.rays(), k["t"], tiled_mats(k), SPP, REPLAY_SEED, est, k["s"], k["vn"], k["g"], k["env"], k["rough"])
    return _MODEL[name, est]


def plane_scene():
    """a planar 8 x 8-cell quad of 128 triangles in y = -1 under the camera, one planar UV mapping of about 2.5 repeats that reaches
    below s = 0, a 7 x 5 random atlas -> (t, m, uv, atlas)"""
    xs, zs = np.linspace(-3.0, 3.0, 9), np.linspace(-2.0, 6.0, 9)
    v = []
    for a in range(8):
        for b in range(8):
            p00, p10, p11, p01 = (xs[a], -1, zs[b]), (xs[a + 1], -1, zs[b]), (xs[a + 1], -1, zs[b + 1]), (xs[a], -1, zs[b + 1])
            v += [list(p00) + list(p10) + list(p11), list(p00) + list(p11) + list(p01)]
    t = np.zeros((128, 12), F)
    t[:, :9] = np.asarray(v, F)
    t = scene.flat_normals(t)
    m = np.zeros((128, 6), F)
    m[:, 0:3] = (0.8, 0.7, 0.6)
    uv = scene.planar_uv(t, origin=(0.5, 0.0, -2.0), s_axis=(2.5 / 6.0, 0, 0), t_axis=(0, 0, 2.5 / 8.0))
    atlas = np.random.default_rng(11).random((5, 7, 3)).astype(F)
    return t, m, uv, atlas


def _random_hits(n, seed):
    """rays that hit random triangles at random barycentric points -> (o, d, tv)"""
    rng = np.random.default_rng(seed)
    tv = rng.uniform(-2, 2, (n, 9)).astype(F)
    b = rng.dirichlet((1, 1, 1), n)
    p = b[:, 0:1] * tv[:, 0:3] + b[:, 1:2] * tv[:, 3:6] + b[:, 2:3] * tv[:, 6:9]
    o = rng.uniform(-4, 4, (n, 3))
    d = p - o
    d /= np.linalg.norm(d, axis=1)[:, None]
    return o.astype(F), d.astype(F), tv


# ---------------------------------------------------------------------------------------------------------------- CPU part
def test_flag_value_and_symbols():
    assert capi.FLAG_TEXTURE == 0x4000000
    assert capi.FLAG_TEXTURE & (capi.FLAG_NEE | capi.FLAG_MIS | capi.FLAG_ACCEL | capi.FLAG_PRIMARY_REUSE | capi.FLAG_CAMERA_SAMPLES | SPEC | SMOOTH |
                                GLASS | ENV | GLOSSY | 0xFF | 0xFF0000) == 0
    names = {"sphip_set_texture", "sphip_set_texture_device", "sphip_set_uv", "sphip_set_uv_device"}
    assert names <= set(capi.SYMBOLS)
    hdr = open(os.path.join(ROOT, "include", "spath_hip.h")).read()
    assert "SPHIP_FLAG_TEXTURE = 0x4000000" in hdr
    assert all(f"int {n}(" in hdr for n in names)
    lib = C.CDLL(capi.LIB_PATH)
    assert all(hasattr(lib, n) for n in names)
    assert capi.load().sphip_abi_version() == 3


def test_model_constant_footprint_is_the_texel():
    """any (s, t) at least 2 texels inside a tile returns the tile's colour bit for bit, whole repeats away too"""
    rng = np.random.default_rng(1)
    for k in range(6):
        c0, r0 = (k % 3) * 8.0, (k // 3) * 8.0
        s = ((c0 + rng.uniform(2, 6, 4000)) / 24.0 + rng.integers(-3, 4, 4000)).astype(F)
        t = ((r0 + rng.uniform(2, 6, 4000)) / 16.0 + rng.integers(-3, 4, 4000)).astype(F)
        c = tm.sample(TILE_ATLAS, s, t)
        assert np.array_equal(_bits(c), _bits(np.broadcast_to(TILE_COLOURS[k], c.shape)))


def _accuracy_bar(tw, th, rng_texels):
    """the f32 statement against float64 bilinear from the same f32 (s, t), per channel, for texels in [0, R].  Along an axis of n
    texels the coordinate carries the rounding of fs = s - floorf(s) (a negative s: 2^-25 at most, n times that in texels), of the
    product fs * n and of the difference with 0.5 (2^-24 n each at most: half an ulp of a value below n), and fx = x - x0 rounds only
    for x < 0 (2^-25): the coordinate is off by less than 3 * 2^-24 n texels, and the sample by that times the largest step between
    neighbouring texels, R at most, on each axis.  The three lerps add three roundings each (a difference, a product, a sum) of values
    within [-R, R]: 9 * 2^-24 R.  Together (3 (tw + th) + 9) 2^-24 R: a few ulps of the texel range per texel of the atlas' sides"""
    return (3 * (tw + th) + 9) * 2.0 ** -24 * rng_texels


def test_model_accuracy_against_float64():
    """MEASURED, in ulps of the texel range R = 1 (2^-24), over 200000 draws each with s, t uniform in [-2, 3) and texels uniform in
    [0, 1): 0.0 at 1 x 1, 4.7 at 5 x 3, 8.6 at 7 x 5, 24.4 at 24 x 16, 122.5 at 256 x 64, against derived bars of 15, 33, 45, 129 and
    969: the error grows with the atlas' sides as derived, and stays 4 to 8 times below the worst case"""
    rng = np.random.default_rng(2)
    for tw, th in ((1, 1), (5, 3), (24, 16), (7, 5), (256, 64)):
        atlas = rng.random((th, tw, 3)).astype(F)
        s, t = rng.uniform(-2, 3, 200000).astype(F), rng.uniform(-2, 3, 200000).astype(F)
        err = np.abs(tm.sample(atlas, s, t).astype(np.float64) - tm.bilinear64(atlas, s, t)).max()
        bar = _accuracy_bar(tw, th, 1.0)
        print(f"{tw} x {th}: max |c32 - c64| = {err:.3e} = {err * 2 ** 24:.1f} ulp(1), bar {bar:.3e} = {bar * 2 ** 24:.0f} ulp(1)")
        assert err <= bar, (tw, th, err, bar)


def test_model_wrap():
    """s and s + k sample alike up to the rounding of the sum: fl(s + k) is off by at most 2^-24 (|k| + 1) (half an ulp below 2^ceil),
    so by 2^-24 (|k| + 1) n texels on an axis of n, and the sample by that times the texel range; bounded against float64 at the
    unmoved (s, t) with the accuracy bar on top"""
    rng = np.random.default_rng(3)
    tw, th = 24, 16
    atlas = rng.random((th, tw, 3)).astype(F)
    s, t = rng.random(50000).astype(F), rng.random(50000).astype(F)
    want = tm.bilinear64(atlas, s, t)
    for k in (-3, -2, -1, 1, 2, 3):
        got = tm.sample(atlas, (s + F(k)).astype(F), (t + F(k)).astype(F)).astype(np.float64)
        bar = _accuracy_bar(tw, th, 1.0) + 2.0 ** -24 * (abs(k) + 1) * (tw + th)
        err = np.abs(got - want).max()
        print(f"k = {k}: max |c(s + k) - c64(s)| = {err:.3e}, bar {bar:.3e}")
        assert err <= bar, (k, err, bar)
    # whole repeats of a dyadic coordinate are exact: the same bits
    sd = (rng.integers(0, 1024, 5000) / 1024.0).astype(F)
    for k in (-2, 1, 5):
        assert np.array_equal(_bits(tm.sample(atlas, sd + F(k), sd)), _bits(tm.sample(atlas, sd, sd)))


def test_model_edge_cases():
    # s = -1e-9: s - floorf(s) rounds up to 1, the select makes it 0: column tw - 1 / 0 with weight 0.5
    for tw in (1, 3, 5, 24, 4096):
        i0, i1, fx, fs = tm.axis(np.array([-1e-9], F), tw)
        assert fs[0] == 0 and i0[0] == tw - 1 and i1[0] == 0 and fx[0] == F(0.5)
    rng = np.random.default_rng(4)
    for tw in (1, 3, 5, 24, 4096):
        s = np.concatenate([rng.uniform(-4, 4, 999000), rng.uniform(-1e-6, 1e-6, 500), np.nextafter(F(1), F(0)) + np.zeros(250),
                            rng.integers(-8, 8, 250) - 2.0 ** -25]).astype(F)
        i0, i1, fx, fs = tm.axis(s, tw)
        assert s.size == 10 ** 6 and i0.min() >= 0 and i0.max() <= tw - 1 and i1.min() >= 0 and i1.max() <= tw - 1
        assert (fx >= 0).all() and (fx < 1).all() and (fs >= 0).all() and (fs < 1).all()
    # a non-finite coordinate leaves the hit untextured, and so does a row of zeros (of either sign)
    uvr = np.ones((4, 6), F)
    uvr[3] = (0, -0.0, 0, 0, -0.0, 0)
    tx = tm.textured(uvr, np.array([0.5, np.nan, np.inf, 0.0], F), np.array([0.5, 0.5, 0.5, 0.0], F))
    assert tx.tolist() == [True, False, False, False]
    o, d, tv = _random_hits(4, 5)
    d[1] = 0                                            # a degenerate ray: u, v are not finite
    rho = np.full((4, 3), 0.5, F)
    alb = tm.tex_albedo(TILE_ATLAS, o, d, tv, uvr, rho)
    assert np.array_equal(alb[1], rho[1]) and np.array_equal(alb[3], rho[3]) and not np.array_equal(alb[0], rho[0])


def test_scene_helpers(tmp_path):
    t, m = scene.default_scene()
    n = t.shape[0]
    ck = scene.checker_texture(8, 4, 2, (1, 0.5, 0.25), (0, 0, 0))
    assert ck.shape == (4, 8, 3) and ck.dtype == F
    assert np.array_equal(ck[0, 0], np.array([1, 0.5, 0.25], F)) and not ck[0, 2].any() and not ck[2, 0].any() and ck[2, 2].any()
    with pytest.raises(ValueError):
        scene.checker_texture(0, 4)
    with pytest.raises(ValueError):
        scene.checker_texture(4, 4, a=(-1, 0, 0))
    uv = scene.uv_table(t, (0, 0, 1, 0, 0, 1), which=[1, 2])
    assert uv.shape == (n, 6) and uv.dtype == F and not uv[0].any() and not uv[3:].any() and uv[1].tolist() == [0, 0, 1, 0, 0, 1]
    with pytest.raises(ValueError):
        scene.uv_table(t, (0, 0, np.nan, 0, 0, 1))
    pu = scene.planar_uv(t, origin=(1, 0, 2), s_axis=(0.5, 0, 0), t_axis=(0, 0, 0.25))
    assert pu.shape == (n, 6) and pu.dtype == F
    want = np.stack([(t[:, 0::3][:, :3].astype(np.float64) - 1) * 0.5, (t[:, 2::3][:, :3].astype(np.float64) - 2) * 0.25], 2).reshape(n, 6)
    assert np.array_equal(pu, want.astype(F))
    assert not scene.planar_uv(t, which=[0])[1:].any()
    scene.write_texture(str(tmp_path / "a.tex"), ck)
    raw = open(tmp_path / "a.tex", "rb").read()
    assert np.frombuffer(raw[:8], np.uint32).tolist() == [8, 4] and raw[8:] == ck.tobytes()
    scene.write_uv(str(tmp_path / "a.uv"), uv)
    assert open(tmp_path / "a.uv", "rb").read() == uv.tobytes()
    c = object.__new__(capi.Context)                     # the checks that need no device
    c._n_tris = n
    with pytest.raises(ValueError, match="one UV row per triangle"):
        capi.Context.set_uv(c, uv[:3])
    with pytest.raises(ValueError, match=r"\(th, tw, 3\)"):
        capi.Context.set_texture(c, np.zeros((4, 4), F))


PLANE_SEEDS = (1, 2, 3, 4)
_PLANE = {}


def _plane_expected(seed):
    """the closed form of test_first_hit_closed_form for one seed, from the oracle's closest hits and device math and the texture model
    -> (want [npix, 3], keep [npix]); computed once per seed"""
    if seed in _PLANE:
        return _PLANE[seed]
    t, m, uv, atlas = plane_scene()
    r = hc.rays()
    if "hits" not in _PLANE:
        idx, dist = O.closest_hits(r, t)
        a = np.flatnonzero(idx >= 0)
        ia = idx[a].astype(np.int64)
        o, d = r[a, :3], r[a, 3:]
        _PLANE["hits"] = (a, ia, path_model.turned_normal(t, ia, d), (o + d * dist[a][:, None]).astype(F),
                          tm.tex_albedo(atlas, o, d, t[ia, 0:9], uv[ia], m[ia, 0:3]))
    a, ia, nrm, x, alb = _PLANE["hits"]
    r1, r2 = _philox(seed, a.astype(np.uint32), np.zeros(a.size, np.uint32), 0)
    nd = _unit_vec(nrm, r1, r2)
    ct = _dot(nd, nrm)
    bi, _ = O.closest_hits(np.concatenate([x, nd], 1), t, ia.astype(np.int32))
    want = np.ones((r.shape[0], 3), F)
    want[a] = F(0) + ((((alb * INV_PI) * F(1)) * ct[:, None]) * INV_P).astype(F)      # E_0 = 0 and the sum start from +0
    keep = np.ones(r.shape[0], bool)
    keep[a[bi >= 0]] = False
    _PLANE[seed] = (want, keep)
    return _PLANE[seed]


def test_first_hit_closed_form_oracle_side():
    """the camera of the closed form sees the plane in a good part of the frame, the mapping spans repeats and reaches below s = 0, the
    albedo varies inside the triangles, and the pixels left out (the bounce ray hits the plane again in the oracle) are at most 2 % of
    the hit pixels: none are expected for a plane"""
    t, m, uv, atlas = plane_scene()
    r = hc.rays()
    left = sum(int((~_plane_expected(seed)[1]).sum()) for seed in PLANE_SEEDS)
    a, ia, _, _, alb = _PLANE["hits"]
    s, tt, _, tx = tm.tex_lookup(atlas, r[a, :3], r[a, 3:], t[ia, 0:9], uv[ia])
    print("hit pixels", a.size, "of", r.shape[0], "; left out", left, "of", len(PLANE_SEEDS) * a.size, "; s in", s.min(), s.max(), "t in", tt.min(), tt.max())
    assert 0.2 * r.shape[0] < a.size < 0.8 * r.shape[0]
    assert tx.all() and (s < 0).sum() > 20 and s.max() - s.min() > 1.5 and tt.max() - tt.min() > 1.0
    assert np.unique(_bits(alb), axis=0).shape[0] > a.size // 2 and np.unique(ia).size > 20
    assert left <= 0.02 * len(PLANE_SEEDS) * a.size


# ---------------------------------------------------------------------------------------------------------------- GPU part
@pytest.mark.gpu
@pytest.mark.parametrize("size", [(1, 1), (5, 3), (24, 16)])
def test_selftest_tex(size):
    """what 12, the device function the kernels call, against the model bit for bit: 4096 random hits, UVs that reach outside [0, 1]
    and below 0, rows of zeros, and rows and rays that give a NaN or an infinite coordinate"""
    tw, th = size
    n = 4096
    rng = np.random.default_rng(20 + tw)
    atlas = rng.random((th, tw, 3)).astype(F)
    o, d, tv = _random_hits(n, 21)
    uvr = rng.uniform(-3, 4, (n, 6)).astype(F)
    uvr[0:256] = 0
    uvr[256:272, 1] = -0.0
    uvr[256:272, 0] = 0
    uvr[256:272, 2:] = 0                                # all six compare equal to zero
    uvr[512:576, 2] = np.inf                            # rows the host setter would refuse (the device setter takes them): s is inf or NaN
    uvr[576:640, 5] = np.nan
    d[640:704] = 0                                      # degenerate rays: u, v are not finite
    uvr[704:768] = (rng.integers(-2, 3, (64, 6))).astype(F)          # whole numbers: fs = 0 at the vertices
    s, t, c, tx = tm.tex_lookup(atlas, o, d, tv, uvr)
    assert (~tx[0:272]).all() and (~tx[512:704]).all() and tx[704:].all()
    assert (s[tx] < 0).sum() > 100 and (s[tx] > 1).sum() > 100
    cx = capi.Context(0)
    cx.set_texture(atlas)
    got = cx.selftest(12, np.concatenate([o, d, tv, uvr], 1).astype(F), n).reshape(n, 6)
    cx.set_texture(None)
    with pytest.raises(RuntimeError, match=E_STATE):
        cx.selftest(12, np.zeros(21, F), 1)
    cx.close()
    want = np.concatenate([s[:, None], t[:, None], c, tx.astype(F)[:, None]], 1).astype(F)
    nan = np.isnan(want)
    assert not nan[:, 2:].any()
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(_bits(got)[~nan], _bits(want)[~nan])


@pytest.mark.gpu
@pytest.mark.parametrize("est", sorted(ESTIMATORS))
@pytest.mark.parametrize("variant", [1, 16])
@pytest.mark.parametrize("name", CASES)
def test_tile_equivalence_model_bit_exact(name, variant, est):
    """every triangle sees one tile of the atlas: the textured render of the materials is the path model's untextured render of the
    materials times the tiles' colours, RGBA8, means and scans bit for bit: the albedo reaches the unwind, both light samples and every
    depth slot"""
    k = case(name)
    want_img, want_mean, want_scans, _ = _model(name, est)
    c = _ctx(k)
    r = hc.rays()
    f = _flags(k) | ESTIMATORS[est] | variant
    img, mean = c.render(r, W, H, SPP, seed=REPLAY_SEED, flags=f | TEX, want_accum=True)
    st = c.stats()
    plain = c.render(r, W, H, SPP, seed=REPLAY_SEED, flags=f, want_accum=True)
    c.close()
    assert st["kernel_variant"] == variant
    assert np.array_equal(_bits(mean), _bits(want_mean))
    assert np.array_equal(img, want_img)
    assert st["scans_executed"] == want_scans
    assert not hc.same(plain, (img, mean))                # the texture matters


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [1, capi.FLAG_ACCEL, 16])
def test_first_hit_closed_form(shape, variant):
    """the variation inside a triangle: the textured plane under a white 1 x 1 map, plain estimator, 1 spp over 4 seeds.  A pixel whose
    bounce ray leaves the scene is (((albedo * INV_PI) * 1) * ct) * INV_P with the model's albedo at the camera's hit, bit for bit,
    and (1, 1, 1) on a primary miss; pixels whose bounce ray hits anything in the oracle are left out (_plane_expected)"""
    t, m, uv, atlas = plane_scene()
    r = hc.rays()
    c = hc.ctx(t, m, env=np.ones((1, 1, 3), F))
    c.set_texture(atlas)
    c.set_uv(uv)
    for seed in PLANE_SEEDS:
        want, keep = _plane_expected(seed)
        mean = c.render(r, W, H, 1, seed=seed, flags=TEX | ENV | variant, want_accum=True)[1]
        assert c.stats()["kernel_variant"] == (8 if variant == capi.FLAG_ACCEL else variant)
        assert np.array_equal(_bits(mean[keep]), _bits(want[keep])), seed
    if variant == 16:
        assert hc._tiles(c)[1] == shape
    c.close()


def _zero_tables(t, m, tables):
    """(s, vn, g, env, rough) of test_zero_uv_is_no_flag's table sets over the bad room"""
    _, _, s, vn = hc.smooth_case("bad_room", True)
    if tables == "none":
        return None, None, None, None, None
    if tables == "spec+rough":
        return s, None, None, None, _random_rough(t.shape[0], 7)
    return s, vn, scene.dielectric_table(t, which=np.arange(14, 40)), env_model.replay_maps()["n3"], None


@pytest.mark.gpu
@pytest.mark.parametrize("est", sorted(ESTIMATORS))
@pytest.mark.parametrize("tables", ["none", "spec+rough", "spec+glass+vn+env"])
@pytest.mark.parametrize("variant", [1, capi.FLAG_ACCEL, 16])
def test_zero_uv_is_no_flag(variant, tables, est):
    """a UV table of zeros and any atlas: the flagged render is the unflagged one bit for bit, scans included, from rays and, with and
    without camera samples, from a camera; and real UVs matter"""
    t, m = scene.closed_room(200)
    s, vn, g, env, rough = _zero_tables(t, m, tables)
    c = hc.ctx(t, m, s, vn, None, g, env, rough)
    c.set_texture(TILE_ATLAS)
    c.set_uv(np.zeros((t.shape[0], 6), F))
    f = hc.table_flags(s, vn, g, env, rough) | ESTIMATORS[est] | variant
    hc.check_zero_table_is_no_flag(c, f, TEX)
    c.set_uv(tile_uv(t.shape[0]))
    r = hc.rays()
    assert not hc.same(c.render(r, W, H, SPP, seed=6, flags=f | TEX, want_accum=True), c.render(r, W, H, SPP, seed=6, flags=f, want_accum=True))
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("glossy", [False, True])
def test_zero_uv_is_no_flag_camera_samples_256(monkeypatch, glossy):
    """the instantiation whose glossy twin once came out wrong with an inlined helper: NEE|MIS, vertex normals
    and camera samples, variant 16 in its 256-thread shape, a table of zeros, over 8 seeds"""
    monkeypatch.setenv("SPATH_HIP_CYLM_SHAPE", "256")
    t, m, s, vn = hc.smooth_case("bad_room", True)
    c = hc.ctx(t, m, s, vn, rough=np.zeros(t.shape[0], F) if glossy else None)
    c.set_texture(TILE_ATLAS)
    c.set_uv(np.zeros((t.shape[0], 6), F))
    cam = view.Camera(40, 26)
    cam.set_delta_mov([0.1, 0.2, 0.3])
    f = NEE_MIS | SPEC | SMOOTH | (GLOSSY if glossy else 0) | capi.FLAG_CAMERA_SAMPLES | 16
    for seed in range(8):
        want = c.render_camera(cam, SPP, seed=seed, flags=f, want_accum=True)
        ws = c.stats()["scans_executed"]
        got = c.render_camera(cam, SPP, seed=seed, flags=f | TEX, want_accum=True)
        assert hc.same(got, want) and c.stats()["scans_executed"] == ws, seed
    assert hc._tiles(c)[1] == 256
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("est", sorted(ESTIMATORS))
@pytest.mark.parametrize("name", ["spec+rough", "glass+vn"])
def test_both_block_shapes(shape, name, est):
    """variant 16 in its 256- and its 512-thread shape: the tile equivalence, a progressive and an adaptive split, primary-hit reuse,
    camera samples, and zero UVs = no flag; the tile size of the stream says which shape ran"""
    k = case(name)
    c = _ctx(k)
    hc.check_both_block_shapes(c, shape, ESTIMATORS[est] | 16 | _flags(k), TEX, _model(name, est)[:3], lambda c: c.set_uv(np.zeros_like(k["uv"])))
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("est", sorted(ESTIMATORS))
@pytest.mark.parametrize("variant", [16, capi.FLAG_ACCEL, 1])
def test_progressive_adaptive_denoise(variant, est):
    k = case("glass+vn")
    f = _flags(k) | ESTIMATORS[est] | variant
    c = _ctx(k)
    hc.check_progressive_adaptive_denoise(c, f | TEX)
    g1 = c.accum_gbuffer()
    c.accum_begin(rays=hc.rays(), w=W, h=H, seed=9, flags=f, adaptive=(0.3, 0.05, 4))
    c.accum_step(4)
    assert c.accum_gbuffer().tobytes() == g1.tobytes()      # the G-buffer stays the material's
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("est", sorted(ESTIMATORS))
@pytest.mark.parametrize("variant", [1, capi.FLAG_ACCEL, 16])
def test_camera_samples_and_device_setters(variant, est):
    """camera samples with the flag are the chain of one-sample accumulations over sphip_camera_rays_device's rays; the atlas and the
    UVs come from device pointers here and give the host setters' render"""
    import torch
    k = case("spec+rough")
    f = _flags(k) | ESTIMATORS[est] | variant | TEX
    c = _ctx(k)
    want = c.render(hc.rays(), W, H, SPP, seed=5, flags=f, want_accum=True)
    c.close()
    c = _ctx(k, atlas=None, uv=False)
    hc.set_device_table(c.set_uv_device, k["uv"])
    d = torch.from_numpy(TILE_ATLAS).to("cuda")
    c.set_texture_device(d.data_ptr(), TILE_ATLAS.shape[1], TILE_ATLAS.shape[0], torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    del d
    assert hc.same(c.render(hc.rays(), W, H, SPP, seed=5, flags=f, want_accum=True), want)
    hc.check_camera_samples(c, f)
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("est", sorted(ESTIMATORS))
@pytest.mark.parametrize("name", ["room", "env"])
def test_reuse_chunks_multi_device(name, est):
    """primary-hit reuse, sample chunks, variant 1 and multi-device contexts ({0,0} and {0,0,0}, one-shot and in two steps) give the
    single context's render; either setter ends a multi-device accumulation"""
    k = case(name)
    r = hc.rays()
    f = _flags(k) | ESTIMATORS[est] | TEX
    c = _ctx(k)
    want = c.render(r, W, H, SPP, seed=4, flags=f, want_accum=True)
    assert not hc.same(want, c.render(r, W, H, SPP, seed=4, flags=f & ~TEX, want_accum=True))
    for extra in (capi.FLAG_PRIMARY_REUSE, capi.flag_chunks(1), capi.flag_chunks(4), capi.flag_chunks(3) | capi.FLAG_PRIMARY_REUSE, 1, 1 | capi.FLAG_PRIMARY_REUSE):
        assert hc.same(c.render(r, W, H, SPP, seed=4, flags=f | extra, want_accum=True), want), extra
    c.close()
    for devs in ([0, 0], [0, 0, 0]):
        mc = _ctx(k, devs)
        got = mc.render(r, W, H, SPP, seed=4, flags=f, want_accum=True)
        mc.accum_begin(rays=r, w=W, h=H, seed=4, flags=f)
        mc.accum_step(1)
        img, mean, _ = mc.accum_step(SPP - 1, want_mean=True)
        assert hc.same(got, want), devs
        assert hc.same((img, mean), want), devs
        for again in (lambda: mc.set_uv(k["uv"]), lambda: mc.set_texture(TILE_ATLAS)):
            again()                                       # ends the accumulation
            with pytest.raises(RuntimeError, match=E_STATE):
                mc.accum_step(1)
            mc.accum_begin(rays=r, w=W, h=H, seed=4, flags=f)
            img, mean, _ = mc.accum_step(SPP, want_mean=True)
            assert hc.same((img, mean), want), devs
        mc.close()


@pytest.mark.gpu
def test_unbiased_plain_vs_mis():
    """plain and NEE|MIS estimate one image of the room whose every triangle carries three repeats of a two-colour checker
    (hip_checks.z_grid: |z| < 4 for the image, < 5 per cell, 16 seeds x 256 spp at 32 x 32)"""
    t, m = scene.closed_room(200)
    atlas = scene.checker_texture(8, 8, 2, (0.95, 0.9, 0.8), (0.15, 0.25, 0.5))
    uv = scene.uv_table(t, (0, 0, 3, 0, 0, 3))
    w = h = 32
    rays = hc.rays(w, h)
    seeds = list(range(100, 116))
    c = hc.ctx(t, m)
    c.set_texture(atlas)
    c.set_uv(uv)
    a = hc.seeds_means(c, rays, w, h, 256, TEX | NEE_MIS, seeds)
    b = hc.seeds_means(c, rays, w, h, 256, TEX, seeds)
    u = hc.seeds_means(c, rays, w, h, 256, 0, seeds[:1])
    c.close()
    assert not np.array_equal(u[0], b[0])
    hc.z_grid(a, b, h, w, "textured room: MIS vs plain, seeds 100..115")


@pytest.mark.gpu
def test_error_contract():
    k = case("room")
    t, m, uv = k["t"], k["m"], k["uv"]
    rays = hc.rays()
    c = hc.ctx(t, m)
    L = capi.load()

    def refused(code, fn, text=None):
        with pytest.raises(RuntimeError, match=code) as e:
            fn()
        assert L.sphip_last_error(c._h), "sphip_last_error is set"
        assert text is None or text in str(e.value), str(e.value)
        c.render(rays, W, H, 1, seed=1)                    # the context stays usable

    refused(E_STATE, lambda: c.render(rays, W, H, 2, seed=1, flags=TEX), "sphip_set_uv")            # neither: the UV table is asked for first
    refused(E_STATE, lambda: c.accum_begin(rays=rays, w=W, h=H, seed=1, flags=TEX), "sphip_set_uv")
    c.set_texture(TILE_ATLAS)
    refused(E_STATE, lambda: c.render(rays, W, H, 2, seed=1, flags=TEX), "sphip_set_uv")            # the atlas alone
    c.set_texture(None)
    c.set_uv(uv)
    refused(E_STATE, lambda: c.render(rays, W, H, 2, seed=1, flags=TEX), "sphip_set_texture")       # the UVs alone
    refused(E_STATE, lambda: c.accum_begin(rays=rays, w=W, h=H, seed=1, flags=TEX), "sphip_set_texture")
    c.set_texture(TILE_ATLAS)
    good = c.render(rays, W, H, 2, seed=1, flags=TEX, want_accum=True)
    unflagged = c.render(rays, W, H, 2, seed=1, want_accum=True)                                  # without the flag both are ignored
    assert not hc.same(good, unflagged)
    refused(E_INVALID, lambda: c.render(rays, W, H, 1, seed=1, mode=capi.MODE_FLAT, flags=TEX))     # flag with FLAT
    refused(E_INVALID, lambda: c.render(rays, W, H, 2, seed=1, flags=TEX | capi.FLAG_NEE))          # flag with NEE alone
    refused(E_INVALID, lambda: c.accum_begin(rays=rays, w=W, h=H, seed=1, flags=TEX | capi.FLAG_NEE))
    for v in (2, 15, 9):                                                                          # the A/B scans, a retired variant
        refused(E_INVALID, lambda: c.render(rays, W, H, 2, seed=1, flags=TEX | v))
        refused(E_INVALID, lambda: c.accum_begin(rays=rays, w=W, h=H, seed=1, flags=TEX | v))
    import torch                                                                                  # hit queries ignore the flag
    d_rays = torch.from_numpy(rays).to("cuda")
    hits = []
    for f in (0, TEX, TEX | capi.FLAG_NEE, TEX | 2):
        d_idx = torch.full((W * H,), -7, dtype=torch.int32, device="cuda")
        d_dist = torch.zeros(W * H, dtype=torch.float32, device="cuda")
        c.closest_hit_device(d_rays.data_ptr(), W * H, d_idx.data_ptr(), d_dist.data_ptr(), flags=f, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        hits.append((d_idx.cpu().numpy(), d_dist.cpu().numpy()))
    assert all(np.array_equal(h[0], hits[0][0]) and np.array_equal(_bits(h[1]), _bits(hits[0][1])) for h in hits) and (hits[0][0] >= 0).any()
    # bad texels, a bad size, non-finite UVs: the message names the first offender and what was set stays
    for bad in (-0.5, np.nan, np.inf):
        ab = TILE_ATLAS.copy()
        ab[3, 5, 1] = bad
        ab[9, 2, 0] = bad
        with pytest.raises(RuntimeError, match=E_INVALID) as e:
            c.set_texture(ab)
        assert "texel (5, 3) has component 1 " in str(e.value), str(e.value)
        assert hc.same(c.render(rays, W, H, 2, seed=1, flags=TEX, want_accum=True), good)
    for tw, th in ((0, 4), (4, 0), (4097, 1), (1, 4097)):
        with pytest.raises(RuntimeError, match=E_INVALID):
            c._check(L.sphip_set_texture(c._h, TILE_ATLAS.ctypes.data, tw, th), "sphip_set_texture")
        with pytest.raises(RuntimeError, match=E_INVALID):                                         # the device form refuses the size too, and clears
            c.set_texture_device(d_rays.data_ptr(), tw, th)
        refused(E_STATE, lambda: c.render(rays, W, H, 2, seed=1, flags=TEX), "sphip_set_texture")
        c.set_texture(TILE_ATLAS)
    assert hc.same(c.render(rays, W, H, 2, seed=1, flags=TEX, want_accum=True), good)
    for bad in (np.nan, np.inf, -np.inf):
        ub = uv.copy()
        ub[40, 3] = bad
        ub[60, 0] = bad
        with pytest.raises(RuntimeError, match=E_INVALID) as e:
            c.set_uv(ub)
        assert "triangle 40 " in str(e.value), str(e.value)
        assert hc.same(c.render(rays, W, H, 2, seed=1, flags=TEX, want_accum=True), good)
    # set_scene clears the UVs and keeps the atlas
    c.set_scene(t, m)
    refused(E_STATE, lambda: c.render(rays, W, H, 2, seed=1, flags=TEX), "sphip_set_uv")
    c.set_uv(uv)
    assert hc.same(c.render(rays, W, H, 2, seed=1, flags=TEX, want_accum=True), good)
    c.set_uv(None)
    refused(E_STATE, lambda: c.render(rays, W, H, 2, seed=1, flags=TEX), "sphip_set_uv")            # NULL cleared it
    assert hc.same(c.render(rays, W, H, 2, seed=1, want_accum=True), unflagged)
    c.set_uv(uv)
    # either setter ends an accumulation, in the same way and with the same code as set_scene does
    c.accum_begin(rays=rays, w=W, h=H, seed=1, flags=TEX)
    c.accum_step(2)
    c.set_scene(t, m)
    with pytest.raises(RuntimeError, match=E_STATE) as by_scene:
        c.accum_step(2)
    c.set_uv(uv)
    for again in (lambda: c.set_uv(uv), lambda: c.set_texture(TILE_ATLAS)):
        c.accum_begin(rays=rays, w=W, h=H, seed=1, flags=TEX)
        c.accum_step(2)
        again()
        with pytest.raises(RuntimeError, match=E_STATE) as by_setter:
            c.accum_step(2)
        assert str(by_setter.value) == str(by_scene.value)
    assert hc.same(c.render(rays, W, H, 2, seed=1, flags=TEX, want_accum=True), good)
    c.close()
    # UVs before a scene are refused; the atlas needs none
    c = capi.Context(0)
    with pytest.raises(RuntimeError, match=E_STATE):
        c.set_uv(uv)
    with pytest.raises(RuntimeError, match=E_STATE):
        c.set_uv_device(0)
    assert L.sphip_last_error(c._h)
    c.set_texture(TILE_ATLAS)
    c.set_scene(t, m)
    c.set_uv(uv)
    assert hc.same(c.render(rays, W, H, 2, seed=1, flags=TEX, want_accum=True), good)
    c.close()
    # the device-pointer forms on a multi-device context
    mc = capi.Context.multi([0, 0])
    mc.set_scene(t, m)
    with pytest.raises(RuntimeError, match=E_STATE):
        mc.set_uv_device(0)
    with pytest.raises(RuntimeError, match=E_STATE):
        mc.set_texture_device(0, 1, 1)
    assert L.sphip_last_error(mc._h)
    with pytest.raises(RuntimeError, match=E_STATE):
        mc.render(rays, W, H, 2, seed=1, flags=TEX)
    ub = uv.copy()
    ub[2, 1] = np.nan
    with pytest.raises(RuntimeError, match=E_INVALID):
        mc.set_uv(ub)
    mc.set_uv(uv)
    mc.set_texture(TILE_ATLAS)
    assert hc.same(mc.render(rays, W, H, 2, seed=1, flags=TEX, want_accum=True), good)
    mc.close()


@pytest.mark.gpu
def test_cli_and_adapter(tmp_path):
    """spath_cli --tex FILE --uv FILE goes through hip_renderer::set_texture and set_uv and gives the capi image, one-shot,
    progressive, with --mis, with --spec beside it and on the camera path; the flat pass is unchanged; one option without the other, a
    UV file of the wrong size, a missing file and --nee alone are refused; the Python renderer mirrors the adapter"""
    import subprocess
    cli = os.path.join(ROOT, "spath_amd", "host", "build", "spath_cli")
    k = case("spec+rough")
    t, m, s, uv = k["t"], k["m"], k["s"], k["uv"]
    sp, ss, st_, su = (str(tmp_path / x) for x in ("s.bin", "s.spec", "s.tex", "s.uv"))
    scene.write_scene(sp, t, m)
    scene.write_specular(ss, s)
    scene.write_texture(st_, TILE_ATLAS)
    scene.write_uv(su, uv)
    w, h = 40, 24
    cam = view.Camera(w, h)
    rays = np.ascontiguousarray(cam.get_viewport(), dtype=F)
    c = hc.ctx(t, m, s)
    c.set_texture(TILE_ATLAS)
    c.set_uv(uv)
    tx = c.render(rays, w, h, 8, seed=9, flags=TEX)
    tx_mis = c.render(rays, w, h, 8, seed=9, flags=TEX | NEE_MIS)
    tx_spec = c.render(rays, w, h, 8, seed=9, flags=TEX | SPEC)
    tx_aa = c.render_camera(cam, 8, seed=9, flags=TEX | capi.FLAG_CAMERA_SAMPLES)
    plain = c.render(rays, w, h, 8, seed=9)
    flat = c.render(rays, w, h, 1, mode=capi.MODE_FLAT)
    c.close()
    assert len({tx.tobytes(), tx_mis.tobytes(), tx_spec.tobytes(), tx_aa.tobytes(), plain.tobytes()}) == 5
    base = [cli, "--scene", sp, "--w", str(w), "--h", str(h), "--spp", "8", "--seed", "9"]
    T = ["--tex", st_, "--uv", su]
    for extra, want in ((T, tx), (T + ["--progressive", "3"], tx), (T + ["--mis"], tx_mis), (T + ["--spec", ss], tx_spec), (T + ["--aa"], tx_aa),
                        (T + ["--mode", "flat"], flat), ([], plain)):
        out = str(tmp_path / "o.rgba")
        subprocess.run(base + ["--out", out] + extra, check=True, capture_output=True, timeout=120)
        assert open(out, "rb").read() == want.tobytes(), extra
    scene.write_uv(str(tmp_path / "short.uv"), uv[:50])
    for bad in (["--tex", st_], ["--uv", su], ["--tex", st_, "--uv", str(tmp_path / "short.uv")], ["--tex", str(tmp_path / "none.tex"), "--uv", su],
                ["--tex", su, "--uv", su], T + ["--nee"]):
        r = subprocess.run(base + ["--out", str(tmp_path / "x.rgba")] + bad, capture_output=True, timeout=120)
        assert r.returncode != 0, bad
    from spath_amd import renderer
    r = renderer.HipRenderer(w, h, seed=9)                # both set: the flag is on, as in the adapter; the flat pass stays
    r.set_texture(TILE_ATLAS)
    out = renderer.Bitmap()
    r.render(renderer.Viewport(w, h, rays), t, m, t.shape[0], 8, out)
    assert np.asarray(out.values).tobytes() == plain.tobytes()          # an atlas alone turns nothing on
    r.set_uv(uv)
    r.render(renderer.Viewport(w, h, rays), t, m, t.shape[0], 8, out)
    assert np.asarray(out.values).tobytes() == tx.tobytes()
    r.render_flat(renderer.Viewport(w, h, rays), t, m, t.shape[0], 1, out)
    assert np.asarray(out.values).tobytes() == flat.tobytes()
    r.set_uv(None)
    r.render(renderer.Viewport(w, h, rays), t, m, t.shape[0], 8, out)
    assert np.asarray(out.values).tobytes() == plain.tobytes()
    r.close()
