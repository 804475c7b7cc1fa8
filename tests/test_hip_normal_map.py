"""Normal mapping (include/spath_hip.h: SPHIP_FLAG_NORMAL_MAP with sphip_set_normal_map and sphip_set_uv): one
map of signed tangent-space vectors on the context, addressed by the scene's UV table.  Each hit's shading normal becomes the map's
normal in the hit's tangent frame, and the hit is from there on a smooth one in every rule.

The arithmetic is stated operation by operation in the header and restated in numpy (tests/nmap_model.py: perturb, and path_model's
walker with the step in place).  STATED TOLERANCE: 0 -- the selftest, images, means, scan counts and G-buffer normals bit for bit.  The
statistical bar is the project's (hip_checks.z_grid).

CPU part: the flag and the symbols; the orientation of the frame against geometry in float64; every fall-back; the scene.py helpers;
what the model's cases cover.  GPU part: the selftest; the model for variants 1 and 16, both estimators; the G-buffer; flat map, zero
UVs and stand-in tables = no flag; the compositions; one expectation; the error contract; the front ends."""
import ctypes as C
import os

import numpy as np
import pytest

import env_model
import hip_checks as hc
import nmap_model as nm
import path_model
import texture_model as tm
from hip_checks import E_INVALID, E_STATE, ESTIMATORS, NEE_MIS, REPLAY_SEED, SPP, H, W, _torch_first, shape  # noqa: F401  (fixtures)
from path_model import F, _bits
from spath_amd import capi, scene, view

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NMAP, TEX = capi.FLAG_NORMAL_MAP, capi.FLAG_TEXTURE
SPEC, GLOSSY, SMOOTH, GLASS, ENV = capi.FLAG_SPECULAR, capi.FLAG_GLOSSY, capi.FLAG_SMOOTH, capi.FLAG_DIELECTRIC, capi.FLAG_ENVIRONMENT
_MODEL = {}

# six tangent-space vectors, one per 8 x 8 tile of the 24 x 16 map of the per-tile cases: two mild tilts, a steep one (grazing rays and
# smooth normals fall back), the unperturbed normal, one that points below the surface, and one whose length overflows
TILE_NORMALS = np.array([[0.3, 0.2, 0.9], [-0.4, 0.3, 0.8], [0.95, -0.1, 0.15], [0.0, 0.0, 1.0], [0.2, -0.3, -0.5], [1e25, 0.0, 1e25]], F)
TILE_MAP = tm.tile_atlas(TILE_NORMALS, 8, 3)
FLAT_MAP = np.zeros((4, 4, 3), F)
FLAT_MAP[..., 2] = 1
TILE_COLOURS = np.array([[0.9, 0.35, 0.2], [0.25, 0.8, 0.3], [0.3, 0.4, 0.95], [0.85, 0.8, 0.15], [0.6, 0.2, 0.7], [0.5, 0.55, 0.6]], F)
TILE_ATLAS = tm.tile_atlas(TILE_COLOURS, 8, 3)


# ---------------------------------------------------------------------------------------------------------------- scenes
def tile_uv(n, special=True):
    """triangle i sees tile i % 6 alone, as the texture tests map it: three distinct UVs in the tile's central 4 x 4 texels, moved by
    whole repeats.  Three rows in 18 are special: zeros (i % 18 == 9), one UV three times (det = 0, i % 18 == 10) and a t axis whose
    tangent overflows (lt = inf, i % 18 == 11); special=False leaves them out"""
    i = np.arange(n)
    k = i % 6
    c0, r0 = (k % 3) * 8.0, (k // 3) * 8.0
    uv = np.zeros((n, 6))
    for v, (a, b) in enumerate(((2.25, 2.5), (5.75, 2.25), (3.5, 5.75))):
        uv[:, 2 * v] = (c0 + a) / 24.0 + (i % 3 - 1)
        uv[:, 2 * v + 1] = (r0 + b) / 16.0 + (i % 2)
    uv = uv.astype(F)
    if not special:
        return uv
    uv[i % 18 == 9] = 0
    uv[i % 18 == 10] = (0.3, 0.4, 0.3, 0.4, 0.3, 0.4)
    uv[i % 18 == 11] = (0.0, 0.0, 1.0, 1e30, 0.0, 2e30)
    return uv


def _random_rough(n, seed):
    return np.array([0, 0.05, 0.3, 1], F)[np.random.default_rng(seed).integers(0, 4, n)]


def case(name):
    """the scenes the model is held to -> dict(t, m, s, vn, g, env, rough, uv, nmap): the plain room under the per-tile map and under a
    map that varies inside the triangles; the room with a mixed specular table and alpha in {0, 0.05, 0.3, 1}; the room with a smooth
    sphere, partly glass; the open clutter under the sky"""
    s = vn = g = env = rough = None
    nmap = TILE_MAP
    if name in ("room", "room_var"):
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
    uv = tile_uv(t.shape[0])
    if name == "room_var":                                    # three repeats of a bumpy 24 x 16 map over every triangle
        uv = scene.uv_table(t, (0, 0, 3, 0, 0, 3))
        nmap = scene.normal_map_from_height(np.random.default_rng(12).random((16, 24)), 3.0)
    return {"t": t, "m": m, "s": s, "vn": vn, "g": g, "env": env, "rough": rough, "uv": uv, "nmap": nmap}


CASES = ("room", "room_var", "spec+rough", "glass+vn", "env")


def _flags(k):
    return hc.table_flags(k["s"], k["vn"], k["g"], k["env"], k["rough"])


def _ctx(k, devs=None, nmap=True, uv=True):
    c = hc.ctx(k["t"], k["m"], k["s"], k["vn"], devs, k["g"], k["env"], k["rough"])
    if nmap:
        c.set_normal_map(k["nmap"])
    if uv:
        c.set_uv(k["uv"])
    return c


def _model(name, est):
    """the path model with the step in place -> (rgba, mean, scans, info, (pix, first ns), guard counts): computed once per case"""
    if (name, est) not in _MODEL:
        k = case(name)
        fn, counts = [], {}
        _MODEL[name, est] = nm.render(hc.rays(), k["t"], k["m"], SPP, REPLAY_SEED, est, k["nmap"], k["uv"], k["s"], k["vn"], k["g"], k["env"],
                                      k["rough"], first_ns=fn, counts=counts) + (fn[0], counts)
    return _MODEL[name, est]


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


def _flat_turned(tv, d):
    """the flat normal of the vertices turned against d, as selftests 7 and 13 take the stored normal"""
    t = np.zeros((tv.shape[0], 12), F)
    t[:, :9] = tv
    with np.errstate(all="ignore"):
        n = scene.flat_normals(t)[:, 9:12]
    n = n.copy()
    flip = path_model._dot(n, d) > F(0)
    n[flip] = n[flip] * F(-1)
    return n


# ---------------------------------------------------------------------------------------------------------------- CPU part
def test_flag_value_and_symbols():
    assert capi.FLAG_NORMAL_MAP == 0x8000000
    assert NMAP & (capi.FLAG_NEE | capi.FLAG_MIS | capi.FLAG_ACCEL | capi.FLAG_PRIMARY_REUSE | capi.FLAG_CAMERA_SAMPLES | SPEC | SMOOTH | GLASS |
                   ENV | GLOSSY | TEX | 0xFF | 0xFF0000) == 0
    names = {"sphip_set_normal_map", "sphip_set_normal_map_device"}
    assert names <= set(capi.SYMBOLS)
    hdr = open(os.path.join(ROOT, "include", "spath_hip.h")).read()
    assert "SPHIP_FLAG_NORMAL_MAP = 0x8000000" in hdr and "normal mapping" in hdr
    assert all(f"int {n}(" in hdr for n in names)
    lib = C.CDLL(capi.LIB_PATH)
    assert all(hasattr(lib, n) for n in names)
    assert capi.load().sphip_abi_version() == 3
    assert capi.Context.SELFTEST_OUT[13] == ("float32", 6)


def _floor(s_axis, t_axis):
    """one floor triangle in y = 0 with stored normal +y and its planar UV row"""
    t = np.zeros((1, 12), F)
    t[0, :9] = (-2, 0, -2, -2, 0, 3, 3, 0, -2)             # (v1 - v0) x (v2 - v0) = (0, 0, 5) x (5, 0, 0) = +y
    t = scene.flat_normals(t)
    assert t[0, 9:12].tolist() == [0, 1, 0]
    return t, scene.planar_uv(t, s_axis=s_axis, t_axis=t_axis)


def test_orientation_pin():
    """the model against geometry, not against its own frame code: on the floor y = 0 with s along +x and t along +z a 1 x 1 map
    (a, b, c) gives normalize(a, c, b); with s along -x normalize(-a, c, b); with s, t swapped normalize(b, c, a); from below
    normalize(a, -c, b).  BOUND 2^-20 per component against float64: about a dozen f32 roundings (2^-24 each) on unit vectors"""
    a, b, c = 0.3, 0.2, 0.9
    m = np.array([[[a, b, c]]], F)
    m64 = m[0, 0].astype(np.float64)
    above = (np.array([[0.5, 2.0, 0.25]], F), np.array([[-0.1, -0.9, 0.2]], F))
    below = (np.array([[0.5, -2.0, 0.25]], F), np.array([[-0.1, 0.9, 0.2]], F))
    for (o, d), s_axis, t_axis, pick in ((above, (1, 0, 0), (0, 0, 1), lambda a, b, c: (a, c, b)),
                                         (above, (-1, 0, 0), (0, 0, 1), lambda a, b, c: (-a, c, b)),
                                         (above, (0, 0, 1), (1, 0, 0), lambda a, b, c: (b, c, a)),
                                         (below, (1, 0, 0), (0, 0, 1), lambda a, b, c: (a, -c, b))):
        t, uv = _floor(s_axis, t_axis)
        nrm = path_model.turned_normal(t, np.array([0]), d)
        _, _, ns, sm, why = nm.perturb(m, o, d, t[:, :9], uv, nrm, nrm, np.array([False]))
        want = np.array(pick(*m64))
        want /= np.sqrt((want * want).sum())
        print(s_axis, t_axis, "np", ns[0], "want", want, "max err", np.abs(ns[0] - want).max())
        assert why[0] == nm.PERTURBED and sm[0]
        assert np.abs(ns[0].astype(np.float64) - want).max() <= 2.0 ** -20
    t, uv = _floor((1, 0, 0), (0, 0, 1))                   # the figures a prototype of the header's arithmetic printed
    ns = nm.perturb(m, *above, t[:, :9], uv, t[:, 9:12], t[:, 9:12], np.array([False]))[2]
    assert np.abs(ns[0].astype(np.float64) - (0.3094264, 0.9282791, 0.20628425)).max() < 5e-8


def test_fall_backs():
    """(0, 0, 1), m.z <= 0, degenerate UVs, a row of zeros, a non-finite s, a texel so steep that np leaves n's side and a grazing ray each
    leave ns and sm bitwise as given, whether the hit came in flat or smooth"""
    t, uv = _floor((1, 0, 0), (0, 0, 1))
    tv = t[:, :9]
    o, d = np.array([[0.5, 2.0, 0.25]], F), np.array([[-0.1, -0.9, 0.2]], F)
    n = t[:, 9:12]
    tilted = np.array([[0.6, 0.8, 0.0]], F)                # a smooth normal 37 degrees off the stored one
    one = lambda v: np.array([[v]], F)
    inf_uv = uv.copy()
    inf_uv[0, 2] = np.inf
    graze_d = np.array([[0.995, -0.1, 0.0]], F)
    cases = ((one((0, 0, 1)), o, d, uv, n, nm.FLAT_TEXEL), (one((0.3, 0.2, 0.0)), o, d, uv, n, nm.MZ), (one((0.3, 0.2, -0.7)), o, d, uv, n, nm.MZ),
             (one((0.3, 0.2, 0.9)), o, d, np.array([[0.3, 0.4] * 3], F), n, nm.DET), (one((0.3, 0.2, 0.9)), o, d, np.zeros((1, 6), F), n, nm.UNTEXTURED),
             (one((0.3, 0.2, 0.9)), o, d, inf_uv, n, nm.UNTEXTURED), (one((0.99, 0.0, 0.05)), o, d, uv, tilted, nm.BELOW),
             (one((0.95, 0.0, 0.2)), o, graze_d, uv, n, nm.GRAZING), (one((1e25, 0, 1e25)), o, d, uv, n, nm.LP),
             (one((0.3, 0.2, 0.9)), o, d, np.array([[0, 0, 1, 1e30, 0, 2e30]], F), n, nm.LT))
    for m, o_, d_, uvr, ns_in, code in cases:
        for sm_in in (False, True):
            _, _, ns, sm, why = nm.perturb(m, o_, d_, tv, uvr, n, ns_in, np.array([sm_in]))
            assert why[0] == code, (nm.GUARDS[why[0]], nm.GUARDS[code])
            assert np.array_equal(_bits(ns), _bits(ns_in)) and sm[0] == sm_in
    assert nm.perturb(one((0.3, 0.2, 0.9)), o, d, tv, uv, n, tilted, np.array([True]))[4][0] == nm.PERTURBED


def test_scene_helpers(tmp_path):
    flat = scene.normal_map_from_height(np.full((5, 7), 0.25), 4.0)
    assert flat.shape == (5, 7, 3) and flat.dtype == F and np.array_equal(flat, np.broadcast_to(np.array([0, 0, 1], F), flat.shape))
    # a ramp along i of slope 0.5 per texel, away from the wrap column: (-k 0.5, 0, 1) / |.|; along j likewise in y
    ramp = np.arange(8)[None, :] * 0.5 + np.zeros((6, 1))
    for k in (1.0, 2.0):
        want = np.array([-k * 0.5, 0.0, 1.0]) / np.sqrt(1 + (k * 0.5) ** 2)
        got = scene.normal_map_from_height(ramp, k)
        assert np.array_equal(got[:, 1:7], np.broadcast_to(want.astype(F), (6, 6, 3)))
        assert np.array_equal(scene.normal_map_from_height(ramp.T, k)[1:7, :], np.broadcast_to(want[[1, 0, 2]].astype(F), (6, 6, 3)))
        assert (got[..., 2] > 0).all() and np.abs(np.sqrt((got.astype(np.float64) ** 2).sum(2)) - 1).max() < 2.0 ** -22
        assert got[0, 0, 0] > 0                                # the wrap column sees the ramp fall back to 0
    with pytest.raises(ValueError):
        scene.normal_map_from_height(np.zeros(4))
    with pytest.raises(ValueError):
        scene.normal_map_from_height(np.full((2, 2), np.nan))
    dec = scene.decode_normal_map(np.array([[[0.5, 0.0, 1.0], [0.25, 0.75, 1.0]]]))
    assert dec.dtype == F and dec.tolist() == [[[0.0, -1.0, 1.0], [-0.5, 0.5, 1.0]]]
    with pytest.raises(ValueError):
        scene.decode_normal_map(np.zeros((4, 4)))
    scene.write_normal_map(str(tmp_path / "a.nmap"), TILE_MAP)
    raw = open(tmp_path / "a.nmap", "rb").read()
    assert raw[:4] == b"SPNM" and np.frombuffer(raw[4:12], np.uint32).tolist() == [24, 16] and raw[12:] == TILE_MAP.tobytes()
    assert np.array_equal(_bits(scene.read_normal_map(str(tmp_path / "a.nmap"))), _bits(TILE_MAP))
    scene.write_texture(str(tmp_path / "a.tex"), TILE_MAP)
    with pytest.raises(ValueError):
        scene.read_normal_map(str(tmp_path / "a.tex"))
    with pytest.raises(ValueError, match=r"\(nh, nw, 3\)"):
        scene.write_normal_map(str(tmp_path / "b.nmap"), np.zeros((4, 4), F))
    c = object.__new__(capi.Context)                     # the check that needs no device
    with pytest.raises(ValueError, match=r"\(nh, nw, 3\)"):
        capi.Context.set_normal_map(c, np.zeros((4, 4), F))


def test_model_coverage():
    """what the model's cases meet, from the model alone (the table of DESIGN.md section 5.16): every case has perturbed hits; across
    the cases every guard falls back at least once, and paths end by the diffuse rule, the mirror rule, a glossy rule and a glass rule"""
    tot = {}
    for name in CASES:
        for est in sorted(ESTIMATORS):
            info, counts = _model(name, est)[3], _model(name, est)[5]
            row = {g: counts.get(g, 0) for g in nm.GUARDS}
            row.update({k: info[k] for k in ("hits", "ended_diffuse", "ended_mirror", "ended", "ended_above", "ended_below", "ended_glass_c",
                                             "ended_glass_reflect", "ended_glass_transmit")})
            print(name, est, row)
            assert sum(counts.values()) == info["hits"] and row["perturbed"] > 0, (name, est)
            for k, v in row.items():
                tot[k] = tot.get(k, 0) + v
    assert all(tot[g] > 0 for g in nm.GUARDS), tot
    assert tot["ended_diffuse"] > 0 and tot["ended_mirror"] > 0 and tot["ended"] + tot["ended_above"] + tot["ended_below"] > 0
    assert tot["ended_glass_c"] + tot["ended_glass_reflect"] + tot["ended_glass_transmit"] > 0


# ---------------------------------------------------------------------------------------------------------------- GPU part
def _selftest_inputs(n):
    """4096 hits: flat and smooth (random vertex normals) rows, back faces among them, rows of zero UVs, degenerate UVs, UVs and rays
    that give non-finite coordinates, and a tangent that overflows"""
    rng = np.random.default_rng(31)
    o, d, tv = _random_hits(n, 32)
    uvr = rng.uniform(-3, 4, (n, 6)).astype(F)
    vn = rng.normal(size=(n, 9)).astype(F)
    vn[: n // 2] = 0                                    # flat rows
    uvr[0:128] = 0
    uvr[128:136, 1] = -0.0
    uvr[128:136, 0] = 0
    uvr[128:136, 2:] = 0
    uvr[256:320, 2:4] = uvr[256:320, 0:2]               # degenerate: v1's UV is v0's ...
    uvr[320:384] = np.tile(uvr[320:384, 0:2], 3)        # ... or all three are one
    uvr[512:576, 2] = np.inf
    uvr[576:640, 5] = np.nan
    d[640:704] = 0
    uvr[704:768, 3] = 1e30
    uvr[704:768, 5] = -2e30
    uvr[n // 2:n // 2 + 64] = 0                         # smooth rows that stay what shade_normal made them
    return o, d, tv, vn, uvr


def _selftest_want(nmap, o, d, tv, vn, uvr):
    nrm = _flat_turned(tv, d)
    _, _, ns, sm = path_model.shade_normal(o, d, tv, vn, nrm)
    s, t, ns2, sm2, why = nm.perturb(nmap, o, d, tv, uvr, nrm, ns, sm)
    return s, t, ns2, why, sm


SELFTEST_MAPS = {(1, 1): np.array([[[0.5, -0.3, 0.6]]], F)}


def _selftest_map(size):
    nw, nh = size
    if size not in SELFTEST_MAPS:
        rng = np.random.default_rng(40 + nw)
        m = rng.uniform(-1, 1, (nh, nw, 3)).astype(F)
        m[..., 2] = rng.uniform(-0.2, 1, (nh, nw)).astype(F)
        k = 3 if nw >= 24 else 1                          # blocks of equal texels: footprints inside them sample the texel itself
        m[0:k, 0:k] = (0, 0, 1)
        m[nh - k:, nw - k:] = (1e25, 0, 1e25)
        SELFTEST_MAPS[size] = m
    return SELFTEST_MAPS[size]


def test_selftest_inputs_cover_every_branch():
    """the model alone: at every map size at least a quarter of the selftest's rows are perturbed and the fall-backs that do not depend
    on the texel are taken (untextured, det, lt, below, grazing); a 1 x 1 map of one mild vector can reach none of the three that do
    ((0, 0, z), m.z <= 0, lp): the 24 x 16 map takes all three, the 5 x 3 map lp, and every fall-back is taken over the three sizes"""
    n = 4096
    seen = set()
    always = {nm.PERTURBED, nm.UNTEXTURED, nm.DET, nm.LT, nm.BELOW, nm.GRAZING}
    by_texel = {(1, 1): set(), (5, 3): {nm.LP}, (24, 16): {nm.FLAT_TEXEL, nm.MZ, nm.LP}}
    for size in ((1, 1), (5, 3), (24, 16)):
        s, t, ns, why, sm = _selftest_want(_selftest_map(size), *_selftest_inputs(n))
        print(size, {g: int((why == k).sum()) for k, g in enumerate(nm.GUARDS)}, "smooth", int(sm.sum()))
        assert (why == nm.PERTURBED).sum() >= n // 4
        assert set(np.unique(why).tolist()) >= always | by_texel[size], size
        seen |= set(np.unique(why).tolist())
        assert sm[why == nm.PERTURBED].any() and (~sm[why == nm.PERTURBED]).any() and sm[why != nm.PERTURBED].any()
    assert seen == set(range(len(nm.GUARDS))), seen


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(1, 1), (5, 3), (24, 16)])
def test_selftest_nmap(size):
    """what 13, the device function the kernels call after shade_normal, against the model bit for bit"""
    n = 4096
    nmap = _selftest_map(size)
    o, d, tv, vn, uvr = _selftest_inputs(n)
    s, t, ns, why, _ = _selftest_want(nmap, o, d, tv, vn, uvr)
    cx = capi.Context(0)
    with pytest.raises(RuntimeError, match=E_STATE):
        cx.selftest(13, np.zeros(30, F), 1)
    cx.set_normal_map(nmap)
    got = cx.selftest(13, np.concatenate([o, d, tv, vn, uvr], 1).astype(F), n).reshape(n, 6)
    cx.close()
    want = np.concatenate([s[:, None], t[:, None], ns, (why == nm.PERTURBED).astype(F)[:, None]], 1).astype(F)
    nan = np.isnan(want)
    assert not nan[why == nm.PERTURBED].any()
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(_bits(got)[~nan], _bits(want)[~nan])


@pytest.mark.gpu
@pytest.mark.parametrize("est", sorted(ESTIMATORS))
@pytest.mark.parametrize("variant", [1, 16])
@pytest.mark.parametrize("name", CASES)
def test_model_bit_exact(name, variant, est):
    """RGBA8, means and scans of the normal-mapped render are the model's, bit for bit; the map matters"""
    k = case(name)
    want_img, want_mean, want_scans = _model(name, est)[:3]
    c = _ctx(k)
    r = hc.rays()
    f = _flags(k) | ESTIMATORS[est] | variant
    img, mean = c.render(r, W, H, SPP, seed=REPLAY_SEED, flags=f | NMAP, want_accum=True)
    st = c.stats()
    plain = c.render(r, W, H, SPP, seed=REPLAY_SEED, flags=f, want_accum=True)
    c.close()
    assert st["kernel_variant"] == variant
    assert np.array_equal(_bits(mean), _bits(want_mean))
    assert np.array_equal(img, want_img)
    assert st["scans_executed"] == want_scans
    assert not hc.same(plain, (img, mean))


def _gbuffer_direct(c, d_rays, flags):
    import torch
    d_g = torch.zeros(W * H * 32, dtype=torch.uint8, device="cuda")
    c.gbuffer_device(d_rays.data_ptr(), W * H, d_g.data_ptr(), flags=flags, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return d_g.cpu().numpy().view(capi.gbuffer_dtype())


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["room_var", "glass+vn"])
def test_gbuffer(name):
    """the normals of sphip_accum_gbuffer and sphip_gbuffer_device are the model's ns of the primary ray, flat or smooth underneath;
    dist, albedo and mat are the unflagged G-buffer's; the flag without its tables is SPHIP_E_STATE"""
    import torch
    k = case(name)
    rays = hc.rays()
    pix, ns = _model(name, "plain")[4]
    first = np.unique(pix, return_index=True)[1]
    f = _flags(k)
    c = _ctx(k, nmap=False, uv=False)
    d_rays = torch.from_numpy(rays).to("cuda")
    g0 = _gbuffer_direct(c, d_rays, f)
    for setter, text in ((lambda: None, "sphip_set_uv"), (lambda: c.set_uv(k["uv"]), "sphip_set_normal_map")):
        setter()
        with pytest.raises(RuntimeError, match=E_STATE) as e:
            _gbuffer_direct(c, d_rays, f | NMAP)
        assert text in str(e.value)
    c.set_normal_map(k["nmap"])
    assert _gbuffer_direct(c, d_rays, f).tobytes() == g0.tobytes()
    g1 = _gbuffer_direct(c, d_rays, f | NMAP)
    assert np.array_equal(_bits(g1["n"][pix[first]]), _bits(ns[first]))
    for key in ("dist", "a", "mat"):
        assert g1[key].tobytes() == g0[key].tobytes(), key
    assert (_bits(g1["n"]) != _bits(g0["n"])).any(1).mean() > 0.2
    c.accum_begin(rays=rays, w=W, h=H, seed=REPLAY_SEED, flags=f | NMAP | 16)
    c.accum_step(2)
    assert c.accum_gbuffer().tobytes() == g1.tobytes()
    den0, den1 = c.accum_denoise(), c.accum_denoise()
    assert den0.shape == (W * H, 4) and np.array_equal(den0, den1)
    c.set_normal_map(FLAT_MAP)
    assert _gbuffer_direct(c, d_rays, f | NMAP).tobytes() == g0.tobytes()
    c.close()


def _zero_tables(t, m, tables):
    """(s, vn, g, env, rough) of the no-flag identities' table sets over the bad room"""
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
def test_flat_map_and_zero_uv_are_no_flag(variant, tables, est):
    """a map of (0, 0, 1) under real UVs, and any map under zero UVs: the flagged render is the unflagged one bit for bit, scans
    included, from rays and, with and without camera samples, from a camera.  With tables "none" the flag runs on stand-in tables
    only (zero vertex normals, the white texel, zero rows, the black map); and a real map under real UVs matters"""
    t, m = scene.closed_room(200)
    s, vn, g, env, rough = _zero_tables(t, m, tables)
    c = hc.ctx(t, m, s, vn, None, g, env, rough)
    f = hc.table_flags(s, vn, g, env, rough) | ESTIMATORS[est] | variant
    c.set_normal_map(FLAT_MAP)
    c.set_uv(tile_uv(t.shape[0]))
    hc.check_zero_table_is_no_flag(c, f, NMAP)
    c.set_normal_map(TILE_MAP)
    c.set_uv(np.zeros((t.shape[0], 6), F))
    hc.check_zero_table_is_no_flag(c, f, NMAP)
    c.set_uv(tile_uv(t.shape[0]))
    r = hc.rays()
    assert not hc.same(c.render(r, W, H, SPP, seed=6, flags=f | NMAP, want_accum=True), c.render(r, W, H, SPP, seed=6, flags=f, want_accum=True))
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("glossy", [False, True])
def test_zero_uv_is_no_flag_camera_samples_256(monkeypatch, glossy):
    """the instantiation whose glossy twin once came out wrong with an inlined helper: NEE|MIS, vertex normals
    and camera samples, variant 16 in its 256-thread shape, a table of zeros, over 8 seeds"""
    monkeypatch.setenv("SPATH_HIP_CYLM_SHAPE", "256")
    t, m, s, vn = hc.smooth_case("bad_room", True)
    c = hc.ctx(t, m, s, vn, rough=np.zeros(t.shape[0], F) if glossy else None)
    c.set_normal_map(TILE_MAP)
    c.set_uv(np.zeros((t.shape[0], 6), F))
    cam = view.Camera(40, 26)
    cam.set_delta_mov([0.1, 0.2, 0.3])
    f = NEE_MIS | SPEC | SMOOTH | (GLOSSY if glossy else 0) | capi.FLAG_CAMERA_SAMPLES | 16
    for seed in range(8):
        want = c.render_camera(cam, SPP, seed=seed, flags=f, want_accum=True)
        ws = c.stats()["scans_executed"]
        got = c.render_camera(cam, SPP, seed=seed, flags=f | NMAP, want_accum=True)
        assert hc.same(got, want) and c.stats()["scans_executed"] == ws, seed
    assert hc._tiles(c)[1] == 256
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("est", sorted(ESTIMATORS))
@pytest.mark.parametrize("name", ["spec+rough", "glass+vn"])
def test_both_block_shapes(shape, name, est):
    """variant 16 in its 256- and its 512-thread shape: the model, a progressive and an adaptive split, primary-hit reuse, camera
    samples, and zero UVs = no flag; the tile size of the stream says which shape ran"""
    k = case(name)
    c = _ctx(k)
    hc.check_both_block_shapes(c, shape, ESTIMATORS[est] | 16 | _flags(k), NMAP, _model(name, est)[:3], lambda c: c.set_uv(np.zeros_like(k["uv"])))
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("est", sorted(ESTIMATORS))
@pytest.mark.parametrize("variant", [16, capi.FLAG_ACCEL, 1])
def test_progressive_adaptive_denoise(variant, est):
    k = case("glass+vn")
    c = _ctx(k)
    hc.check_progressive_adaptive_denoise(c, _flags(k) | ESTIMATORS[est] | variant | NMAP)
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("est", sorted(ESTIMATORS))
def test_accel_parity(est):
    k = case("spec+rough")
    c = _ctx(k)
    hc.check_accel_parity(c, _flags(k) | ESTIMATORS[est] | NMAP)
    assert c.stats()["kernel_variant"] == 8
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("est", sorted(ESTIMATORS))
@pytest.mark.parametrize("variant", [1, capi.FLAG_ACCEL, 16])
def test_camera_samples_and_device_setters(variant, est):
    """camera samples with the flag are the chain of one-sample accumulations over sphip_camera_rays_device's rays; the map and the
    UVs come from device pointers here and give the host setters' render"""
    import torch
    k = case("spec+rough")
    f = _flags(k) | ESTIMATORS[est] | variant | NMAP
    c = _ctx(k)
    want = c.render(hc.rays(), W, H, SPP, seed=5, flags=f, want_accum=True)
    c.close()
    c = _ctx(k, nmap=False, uv=False)
    hc.set_device_table(c.set_uv_device, k["uv"])
    d = torch.from_numpy(k["nmap"]).to("cuda")
    c.set_normal_map_device(d.data_ptr(), k["nmap"].shape[1], k["nmap"].shape[0], torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    del d
    assert hc.same(c.render(hc.rays(), W, H, SPP, seed=5, flags=f, want_accum=True), want)
    hc.check_camera_samples(c, f)
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("est", sorted(ESTIMATORS))
@pytest.mark.parametrize("variant", [1, 16])
def test_with_texture(variant, est):
    """SPHIP_FLAG_TEXTURE beside the flag: every triangle sees one tile of the atlas and one of the map (no special UV rows here), so
    the render is the normal-mapped one of the materials times the tiles' colours (the texture tests' equivalence), which the model
    tests hold; without SPHIP_FLAG_TEXTURE the atlas is ignored"""
    k = case("spec+rough")
    k["uv"] = tile_uv(k["t"].shape[0], special=False)
    m2 = k["m"].copy()
    m2[:, :3] = (k["m"][:, :3] * TILE_COLOURS[np.arange(m2.shape[0]) % 6]).astype(F)
    r = hc.rays()
    f = _flags(k) | ESTIMATORS[est] | variant | NMAP
    c = _ctx(k)
    c.set_texture(TILE_ATLAS)
    got = c.render(r, W, H, SPP, seed=REPLAY_SEED, flags=f | TEX, want_accum=True)
    scans = c.stats()["scans_executed"]
    off = c.render(r, W, H, SPP, seed=REPLAY_SEED, flags=f, want_accum=True)
    c.close()
    c = _ctx(dict(k, m=m2))
    want = c.render(r, W, H, SPP, seed=REPLAY_SEED, flags=f, want_accum=True)
    assert hc.same(got, want) and c.stats()["scans_executed"] == scans
    c.close()
    c = _ctx(k)
    assert hc.same(off, c.render(r, W, H, SPP, seed=REPLAY_SEED, flags=f, want_accum=True)) and not hc.same(off, got)
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("est", sorted(ESTIMATORS))
@pytest.mark.parametrize("name", ["room", "env"])
def test_reuse_chunks_multi_device(name, est):
    """primary-hit reuse, sample chunks, variant 1 and multi-device contexts ({0,0} and {0,0,0}, one-shot and in two steps) give the
    single context's render; the setter ends a multi-device accumulation.  A COPY of hip_checks.check_reuse_chunks_multi_device's
    body, as in the texture tests: the helper builds its contexts itself and cannot give them a map or a UV table"""
    k = case(name)
    r = hc.rays()
    f = _flags(k) | ESTIMATORS[est] | NMAP
    c = _ctx(k)
    want = c.render(r, W, H, SPP, seed=4, flags=f, want_accum=True)
    assert not hc.same(want, c.render(r, W, H, SPP, seed=4, flags=f & ~NMAP, want_accum=True))
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
        assert mc.accum_gbuffer().shape[0] == W * H
        mc.set_normal_map(k["nmap"])                      # ends the accumulation
        with pytest.raises(RuntimeError, match=E_STATE):
            mc.accum_step(1)
        mc.accum_begin(rays=r, w=W, h=H, seed=4, flags=f)
        img, mean, _ = mc.accum_step(SPP, want_mean=True)
        assert hc.same((img, mean), want), devs
        mc.close()


@pytest.mark.gpu
def test_unbiased_plain_vs_mis():
    """plain and NEE|MIS estimate one image of the room whose every triangle carries three repeats of a bumpy map
    (hip_checks.z_grid: |z| < 4 for the image, < 5 per cell, 16 seeds x 256 spp at 32 x 32)"""
    k = case("room_var")
    w = h = 32
    rays = hc.rays(w, h)
    seeds = list(range(100, 116))
    c = _ctx(k)
    a = hc.seeds_means(c, rays, w, h, 256, NMAP | NEE_MIS, seeds)
    b = hc.seeds_means(c, rays, w, h, 256, NMAP, seeds)
    u = hc.seeds_means(c, rays, w, h, 256, 0, seeds[:1])
    c.close()
    assert not np.array_equal(u[0], b[0])
    hc.z_grid(a, b, h, w, "normal-mapped room: MIS vs plain, seeds 100..115")


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

    refused(E_STATE, lambda: c.render(rays, W, H, 2, seed=1, flags=NMAP), "sphip_set_uv")           # neither: the UV table is asked for first
    refused(E_STATE, lambda: c.accum_begin(rays=rays, w=W, h=H, seed=1, flags=NMAP), "sphip_set_uv")
    c.set_normal_map(TILE_MAP)
    refused(E_STATE, lambda: c.render(rays, W, H, 2, seed=1, flags=NMAP), "sphip_set_uv")           # the map alone
    c.set_normal_map(None)
    c.set_uv(uv)
    refused(E_STATE, lambda: c.render(rays, W, H, 2, seed=1, flags=NMAP), "sphip_set_normal_map")   # the UVs alone
    refused(E_STATE, lambda: c.accum_begin(rays=rays, w=W, h=H, seed=1, flags=NMAP), "sphip_set_normal_map")
    c.set_texture(TILE_ATLAS)                                                                     # an atlas is no normal map
    refused(E_STATE, lambda: c.render(rays, W, H, 2, seed=1, flags=NMAP), "sphip_set_normal_map")
    c.set_texture(None)
    c.set_normal_map(TILE_MAP)
    good = c.render(rays, W, H, 2, seed=1, flags=NMAP, want_accum=True)
    unflagged = c.render(rays, W, H, 2, seed=1, want_accum=True)                                  # without the flag both are ignored
    assert not hc.same(good, unflagged)
    refused(E_INVALID, lambda: c.render(rays, W, H, 1, seed=1, mode=capi.MODE_FLAT, flags=NMAP), "SPHIP_MODE_PT only")
    refused(E_INVALID, lambda: c.render(rays, W, H, 2, seed=1, flags=NMAP | capi.FLAG_NEE), "SPHIP_FLAG_NEE alone")
    refused(E_INVALID, lambda: c.accum_begin(rays=rays, w=W, h=H, seed=1, flags=NMAP | capi.FLAG_NEE))
    for v in (2, 15, 9):                                                                          # the A/B scans, a retired variant
        refused(E_INVALID, lambda: c.render(rays, W, H, 2, seed=1, flags=NMAP | v))
        refused(E_INVALID, lambda: c.accum_begin(rays=rays, w=W, h=H, seed=1, flags=NMAP | v))
    import torch                                                                                  # hit queries ignore the flag
    d_rays = torch.from_numpy(rays).to("cuda")
    hits = []
    for f in (0, NMAP, NMAP | capi.FLAG_NEE, NMAP | 2):
        d_idx = torch.full((W * H,), -7, dtype=torch.int32, device="cuda")
        d_dist = torch.zeros(W * H, dtype=torch.float32, device="cuda")
        c.closest_hit_device(d_rays.data_ptr(), W * H, d_idx.data_ptr(), d_dist.data_ptr(), flags=f, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        hits.append((d_idx.cpu().numpy(), d_dist.cpu().numpy()))
    assert all(np.array_equal(h[0], hits[0][0]) and np.array_equal(_bits(h[1]), _bits(hits[0][1])) for h in hits) and (hits[0][0] >= 0).any()
    # texels that are not finite, a bad size: the message names the first offender and what was set stays; negative values are legal
    for bad in (np.nan, np.inf, -np.inf):
        ab = TILE_MAP.copy()
        ab[3, 5, 1] = bad
        ab[9, 2, 0] = bad
        with pytest.raises(RuntimeError, match=E_INVALID) as e:
            c.set_normal_map(ab)
        assert "normal map: texel (5, 3) has component 1 " in str(e.value) and "every value finite)" in str(e.value), str(e.value)
        assert hc.same(c.render(rays, W, H, 2, seed=1, flags=NMAP, want_accum=True), good)
    for nw, nh in ((0, 4), (4, 0), (4097, 1), (1, 4097)):
        with pytest.raises(RuntimeError, match=E_INVALID):
            c._check(L.sphip_set_normal_map(c._h, TILE_MAP.ctypes.data, nw, nh), "sphip_set_normal_map")
        assert hc.same(c.render(rays, W, H, 2, seed=1, flags=NMAP, want_accum=True), good)        # the host form left the map in place
        with pytest.raises(RuntimeError, match=E_INVALID):                                         # the device form refuses the size too, and clears
            c.set_normal_map_device(d_rays.data_ptr(), nw, nh)
        refused(E_STATE, lambda: c.render(rays, W, H, 2, seed=1, flags=NMAP), "sphip_set_normal_map")
        c.set_normal_map(TILE_MAP)
    # set_scene clears the UVs and keeps the map
    c.set_scene(t, m)
    refused(E_STATE, lambda: c.render(rays, W, H, 2, seed=1, flags=NMAP), "sphip_set_uv")
    c.set_uv(uv)
    assert hc.same(c.render(rays, W, H, 2, seed=1, flags=NMAP, want_accum=True), good)
    c.set_normal_map(None)
    refused(E_STATE, lambda: c.render(rays, W, H, 2, seed=1, flags=NMAP), "sphip_set_normal_map")   # NULL cleared it
    assert hc.same(c.render(rays, W, H, 2, seed=1, want_accum=True), unflagged)
    c.set_normal_map(TILE_MAP)
    # the setter ends an accumulation, in the same way and with the same code as set_scene does
    c.accum_begin(rays=rays, w=W, h=H, seed=1, flags=NMAP)
    c.accum_step(2)
    c.set_scene(t, m)
    with pytest.raises(RuntimeError, match=E_STATE) as by_scene:
        c.accum_step(2)
    c.set_uv(uv)
    c.accum_begin(rays=rays, w=W, h=H, seed=1, flags=NMAP)
    c.accum_step(2)
    c.set_normal_map(TILE_MAP)
    with pytest.raises(RuntimeError, match=E_STATE) as by_setter:
        c.accum_step(2)
    assert str(by_setter.value) == str(by_scene.value)
    assert hc.same(c.render(rays, W, H, 2, seed=1, flags=NMAP, want_accum=True), good)
    c.close()
    # the map needs no scene
    c = capi.Context(0)
    c.set_normal_map(TILE_MAP)
    c.set_scene(t, m)
    c.set_uv(uv)
    assert hc.same(c.render(rays, W, H, 2, seed=1, flags=NMAP, want_accum=True), good)
    c.close()
    # the device-pointer form on a multi-device context
    mc = capi.Context.multi([0, 0])
    mc.set_scene(t, m)
    with pytest.raises(RuntimeError, match=E_STATE):
        mc.set_normal_map_device(0, 1, 1)
    assert L.sphip_last_error(mc._h)
    mc.set_uv(uv)
    with pytest.raises(RuntimeError, match=E_STATE):
        mc.render(rays, W, H, 2, seed=1, flags=NMAP)
    ab = TILE_MAP.copy()
    ab[0, 0, 2] = np.nan
    with pytest.raises(RuntimeError, match=E_INVALID):
        mc.set_normal_map(ab)
    mc.set_normal_map(TILE_MAP)
    assert hc.same(mc.render(rays, W, H, 2, seed=1, flags=NMAP, want_accum=True), good)
    mc.close()


@pytest.mark.gpu
def test_cli_and_adapter(tmp_path):
    """spath_cli --nmap FILE --uv FILE goes through hip_renderer::set_normal_map and set_uv and gives the capi image, one-shot,
    progressive, with --mis, with --spec or --tex beside it and on the camera path; the flat pass is unchanged; --nmap without --uv, a
    missing file, an atlas file for a map and --nee alone are refused; the Python renderer mirrors the adapter"""
    import subprocess
    cli = os.path.join(ROOT, "spath_amd", "host", "build", "spath_cli")
    k = case("spec+rough")
    t, m, s, uv = k["t"], k["m"], k["s"], k["uv"]
    sp, ss, st_, su, sn = (str(tmp_path / x) for x in ("s.bin", "s.spec", "s.tex", "s.uv", "s.nmap"))
    scene.write_scene(sp, t, m)
    scene.write_specular(ss, s)
    scene.write_texture(st_, TILE_ATLAS)
    scene.write_uv(su, uv)
    scene.write_normal_map(sn, TILE_MAP)
    w, h = 40, 24
    cam = view.Camera(w, h)
    rays = np.ascontiguousarray(cam.get_viewport(), dtype=F)
    c = hc.ctx(t, m, s)
    c.set_normal_map(TILE_MAP)
    c.set_texture(TILE_ATLAS)
    c.set_uv(uv)
    nx = c.render(rays, w, h, 8, seed=9, flags=NMAP)
    nx_mis = c.render(rays, w, h, 8, seed=9, flags=NMAP | NEE_MIS)
    nx_spec = c.render(rays, w, h, 8, seed=9, flags=NMAP | SPEC)
    nx_tex = c.render(rays, w, h, 8, seed=9, flags=NMAP | TEX)
    nx_aa = c.render_camera(cam, 8, seed=9, flags=NMAP | capi.FLAG_CAMERA_SAMPLES)
    plain = c.render(rays, w, h, 8, seed=9)
    flat = c.render(rays, w, h, 1, mode=capi.MODE_FLAT)
    c.close()
    assert len({nx.tobytes(), nx_mis.tobytes(), nx_spec.tobytes(), nx_tex.tobytes(), nx_aa.tobytes(), plain.tobytes()}) == 6
    base = [cli, "--scene", sp, "--w", str(w), "--h", str(h), "--spp", "8", "--seed", "9"]
    N = ["--nmap", sn, "--uv", su]
    for extra, want in ((N, nx), (N + ["--progressive", "3"], nx), (N + ["--mis"], nx_mis), (N + ["--spec", ss], nx_spec), (N + ["--tex", st_], nx_tex),
                        (N + ["--aa"], nx_aa), (N + ["--mode", "flat"], flat), ([], plain)):
        out = str(tmp_path / "o.rgba")
        subprocess.run(base + ["--out", out] + extra, check=True, capture_output=True, timeout=120)
        assert open(out, "rb").read() == want.tobytes(), extra
    for bad in (["--nmap", sn], ["--nmap", str(tmp_path / "none.nmap"), "--uv", su], ["--nmap", st_, "--uv", su], N + ["--nee"]):
        r = subprocess.run(base + ["--out", str(tmp_path / "x.rgba")] + bad, capture_output=True, timeout=120)
        assert r.returncode != 0, bad
    from spath_amd import renderer
    r = renderer.HipRenderer(w, h, seed=9)                # both set: the flag is on, as in the adapter; the flat pass stays
    r.set_normal_map(TILE_MAP)
    out = renderer.Bitmap()
    r.render(renderer.Viewport(w, h, rays), t, m, t.shape[0], 8, out)
    assert np.asarray(out.values).tobytes() == plain.tobytes()          # a map alone turns nothing on
    r.set_uv(uv)
    r.render(renderer.Viewport(w, h, rays), t, m, t.shape[0], 8, out)
    assert np.asarray(out.values).tobytes() == nx.tobytes()             # and the UV table beside it turns on this flag alone
    r.set_texture(TILE_ATLAS)
    r.render(renderer.Viewport(w, h, rays), t, m, t.shape[0], 8, out)
    assert np.asarray(out.values).tobytes() == nx_tex.tobytes()
    r.set_texture(None)
    r.render_flat(renderer.Viewport(w, h, rays), t, m, t.shape[0], 1, out)
    assert np.asarray(out.values).tobytes() == flat.tobytes()
    r.set_normal_map(None)
    r.render(renderer.Viewport(w, h, rays), t, m, t.shape[0], 8, out)
    assert np.asarray(out.values).tobytes() == plain.tobytes()
    r.close()
