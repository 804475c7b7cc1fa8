"""Glossy reflection (include/spath_hip.h: SPHIP_FLAG_GLOSSY with sphip_set_roughness): a per-triangle GGX
alpha that roughens the mirror lobe of SPHIP_FLAG_SPECULAR.  A hit that took the lobe of a triangle with alpha > 0 reflects about a
microfacet normal drawn from the distribution of visible normals and is weighted by the Smith term G1 of the outgoing direction.

The arithmetic is stated operation by operation in the header, so it is replayed in numpy (tests/glossy_model.py's draw in
tests/path_model.py's loop, its `rough` table).  STATED TOLERANCE: 0 -- images, means and scan counts bit for bit.  The statistical bars
are the project's: hip_checks.z_grid over 16 seeds x 256 spp at 32 x 32 for plain against NEE|MIS, and 5 standard errors of the mean
for the statement against the float64 quadrature of what it must mean.  The f32 statement is held to a float64 restatement of the same
formulas at 2^-6 where cl >= 1/16 (test_f32_statement_against_float64 says where the figure comes from).

CPU part: the flag and the symbols; the model with a table of zeros and on rows of zeros against the model without a table; a plane by
hand; the statement against the quadrature; the f32 statement against float64; scene.roughness_table; the coverage of the replay cases.
GPU part: the selftest; the replay for variants 1, 8 and 16, both estimators; zero table = no flag; both workgroup shapes; the
compositions; one expectation and the sample bound; the error contract; the front ends."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

import env_model
import glossy_model as gm
import hip_checks as hc
import path_model
from hip_checks import E_INVALID, E_STATE, ESTIMATORS, NEE_MIS, REPLAY_SEED, SPP, H, W, _torch_first, shape  # noqa: F401  (fixtures)
from path_model import F, _bits
from spath_amd import capi, scene, view

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GLOSSY = capi.FLAG_GLOSSY
SPEC = capi.FLAG_SPECULAR
SMOOTH = capi.FLAG_SMOOTH
GLASS = capi.FLAG_DIELECTRIC
ENV = capi.FLAG_ENVIRONMENT
BAR = 2.0 ** -6                                       # test_f32_statement_against_float64
_MODEL = {}


# ---------------------------------------------------------------------------------------------------------------- scenes
def _random_rough(n, seed):
    """alpha in {0, 0.05, 0.3, 1} per triangle"""
    return np.array([0, 0.05, 0.3, 1], F)[np.random.default_rng(seed).integers(0, 4, n)]


def case(name):
    """the replay's scenes -> dict(t, m, s, vn, g, env, rough): the mirror floor made glossy; the mixed room with alpha in {0, 0.05,
    0.3, 1} per triangle; the mirror sphere, smooth and glossy; the glass sphere over a glossy floor; the open clutter under the sky"""
    vn = g = env = None
    if name == "floor":
        t, m, s = hc.mirror_floor()
        rough = scene.roughness_table(t, 0.3, which=[1, 2])
    elif name == "mixed":
        t, m, s = hc.mixed_room()
        rough = _random_rough(t.shape[0], 5)
    elif name == "sphere":
        t, m, s, vn = hc.sphere_scene(True)
        rough = scene.roughness_table(t, 0.4, which=np.arange(7, t.shape[0]))
    elif name == "glass":
        t, m, s, _ = hc.sphere_scene(False)
        g = scene.dielectric_table(t, 1.5, (0.9, 0.95, 1.0), which=np.arange(7, t.shape[0]))
        s[1:3] = (0.9, 0.8, 0.7, 1.0)
        rough = scene.roughness_table(t, 0.3)                 # ignored on the sphere's interfaces, idle on the diffuse walls
    elif name == "sky":
        t, m = scene.open_clutter(100)
        s = hc.mixed_table(t, m)
        rough = _random_rough(t.shape[0], 6)
        env = env_model.replay_maps()["sky64"]
    else:
        raise KeyError(name)
    return {"t": t, "m": m, "s": s, "vn": vn, "g": g, "env": env, "rough": rough}


CASES = ("floor", "mixed", "sphere", "glass", "sky")


def _flags(k):
    return hc.table_flags(k["s"], k["vn"], k["g"], k["env"], k["rough"])


def _ctx(k, devs=None, rough=True):
    return hc.ctx(k["t"], k["m"], k["s"], k["vn"], devs, k["g"], k["env"], k["rough"] if rough else None)


def _model(name, est):
    """the replay's reference, computed once per case"""
    if (name, est) not in _MODEL:
        k = case(name)
        _MODEL[name, est] = path_model.render(hc.rays(), k["t"], k["m"], SPP, REPLAY_SEED, est, k["s"], k["vn"], k["g"], k["env"], k["rough"])
    return _MODEL[name, est]


def _covered(info, name):
    gm.covered(info, smooth=name == "sphere")
    if name in ("mixed", "sky"):
        assert info["alpha0"] > 0, info
    if name == "glass":
        assert info["glass"] > 0, info
    if name == "sky":
        assert info["miss_after_glossy"] > 0, info
    if name in ("floor", "mixed"):
        assert info["emit_after_glossy"] > 0, info


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1)[:, None]).astype(F)


def _random_inputs(n, seed):
    """unit rays, unit normals turned against them, alpha in (0, 1], uniforms in [0, 1)"""
    rng = np.random.default_rng(seed)
    d, ns = _unit(rng, n), _unit(rng, n)
    ns[gm._dot(d, ns) > 0] *= F(-1)
    al = (1.0 - rng.random(n)).astype(F)
    return d, ns, al, rng.random(n), rng.random(n)


# ---------------------------------------------------------------------------------------------------------------- CPU part
def test_flag_value_and_symbols():
    assert capi.FLAG_GLOSSY == 0x2000000
    assert capi.FLAG_GLOSSY & (capi.FLAG_NEE | capi.FLAG_MIS | capi.FLAG_ACCEL | capi.FLAG_PRIMARY_REUSE | capi.FLAG_CAMERA_SAMPLES |
                               capi.FLAG_SPECULAR | capi.FLAG_SMOOTH | capi.FLAG_DIELECTRIC | capi.FLAG_ENVIRONMENT | 0xFF | 0xFF0000) == 0
    assert {"sphip_set_roughness", "sphip_set_roughness_device"} <= set(capi.SYMBOLS)
    lib = C.CDLL(capi.LIB_PATH)
    assert hasattr(lib, "sphip_set_roughness") and hasattr(lib, "sphip_set_roughness_device")
    assert capi.load().sphip_abi_version() == 3
    hdr = open(os.path.join(ROOT, "include", "spath_hip.h")).read()
    assert "SPHIP_FLAG_GLOSSY = 0x2000000" in hdr
    L = capi.load()
    assert L.sphip_set_roughness(None, None) == -1 and L.sphip_set_roughness_device(None, None, None) == -1


@pytest.mark.parametrize("est", sorted(ESTIMATORS))
@pytest.mark.parametrize("tables", ["spec", "spec+glass+vn", "spec+env"])
def test_zero_table_is_no_table(tables, est):
    """a roughness table of zeros executes the step and changes nothing: the bits and the scans of the call without the table, plain
    and mis, bare and with glass, vertex normals and a map; and rows of zeros among non-zero rows are the mirror: a table that is
    non-zero only on triangles whose lobe is never specular changes nothing"""
    k = case("glass" if "glass" in tables else "sky" if "env" in tables else "mixed")
    t, m, s = k["t"], k["m"], k["s"]
    vn = scene.vertex_normals(t, which=np.arange(7, t.shape[0])) if "vn" in tables else None
    r = hc.rays(24, 16)
    want = path_model.samples(r, t, m, REPLAY_SEED, 0, 2, est, s, vn, k["g"], k["env"])
    for rough in (np.zeros(t.shape[0], F), np.where(s[:, 3] > 0, F(0), F(0.5)).astype(F)):
        got = path_model.samples(r, t, m, REPLAY_SEED, 0, 2, est, s, vn, k["g"], k["env"], rough)
        assert np.array_equal(_bits(got[0]), _bits(want[0])) and got[1] == want[1]
        assert got[2]["glossy"] == 0 and got[2]["alpha0"] > 0


def test_plane_by_hand():
    """one ray straight down on a glossy plane: ns = (0, 0, 1), dir = (0, 0, -1).  The frame is the identity, v = vh = (0, 0, 1) whatever
    alpha, l2 = 0 so T1 = (1, 0, 0), and u1 = 0 (the disk's centre) gives m = ns, nd = -dir, g = 1 exactly"""
    d, ns = np.array([[0, 0, -1]], F), np.array([[0, 0, 1]], F)
    for al in (2.0 ** -10, 0.2, 1.0):
        parts = {}
        m, nd, g, ok = gm.gloss_bounce(d, ns, np.array([al], F), np.array([0.0]), np.array([0.37]), parts)
        assert np.array_equal(parts["t"], [[1, 0, 0]]) and np.array_equal(parts["bt"], [[0, 1, 0]])
        assert np.array_equal(parts["vh"], [[0, 0, 1]]) and np.array_equal(parts["T1"], [[1, 0, 0]]) and np.array_equal(parts["T2"], [[0, 1, 0]])
        assert np.array_equal(m, ns) and np.array_equal(nd, -d) and g[0] == 1 and ok[0]
    # the other sign of the frame, and ns.z = -0
    for nz in (-1.0, -0.0):
        n2 = np.array([[0, 1 if nz == 0 else 0, nz]], F)
        d2 = -n2
        m, nd, g, ok = gm.gloss_bounce(d2, n2, np.array([0.5], F), np.array([0.0]), np.array([0.1]))
        assert np.array_equal(m, n2 + F(0)) and np.array_equal(nd, n2 + F(0)) and g[0] == 1 and ok[0]


def _quadrature(al, cv, nw=3000, nphi=1500):
    """float64 midpoint quadrature of int D(m) G1(v) G1(l) / (4 cos_v) dl over the upper hemisphere of l, taken over the microfacet normal
    m (dl = 4 (v . m) dm) in the coordinates that flatten D: D(m) cos_m dm = dxi dphi / (2 pi) with tan^2 theta_m = al^2 xi / (1 - xi),
    and xi = sin^2(pi w / 2) so that the 1 / cos_m of grazing normals meets a vanishing Jacobian.  v = (sqrt(1 - cv^2), 0, cv): the
    integrand is even in phi, so half the circle is taken twice"""
    w = (np.arange(nw) + 0.5) / nw
    ph = (np.arange(nphi) + 0.5) / nphi * np.pi
    sw, cw = np.sin(0.5 * np.pi * w), np.cos(0.5 * np.pi * w)
    jac = np.pi * sw * cw                                  # dxi / dw
    tan_m = al * sw / cw                                  # sqrt(xi / (1 - xi)) = tan(pi w / 2)
    cos_m = 1.0 / np.sqrt(1.0 + tan_m * tan_m)
    sin_m = tan_m * cos_m
    vx, vz = np.sqrt(1.0 - cv * cv), cv
    mx, my, mz = sin_m[:, None] * np.cos(ph)[None, :], sin_m[:, None] * np.sin(ph)[None, :], cos_m[:, None] * np.ones(nphi)[None, :]
    vm = vx * mx + vz * mz
    lz = 2.0 * vm * mz - vz

    def G1(c):
        return 2.0 * c / (c + np.sqrt(al * al + (1.0 - al * al) * c * c))
    f = np.where((vm > 0) & (lz > 0), G1(vz) * vm / (vz * mz) * G1(np.maximum(lz, 1e-300)), 0.0)
    return float((f * jac[:, None]).sum() / nw * 2.0 / (2.0 * nphi))


@pytest.mark.parametrize("cv", [0.95, 0.5, 0.15])
@pytest.mark.parametrize("al", [0.05, 0.2, 0.5, 1.0])
def test_statement_against_quadrature(al, cv):
    """the statement against what it must mean: the draws' pdf is D G1(v) / (4 cos_v) per solid angle of l and the reflectance of the
    lobe D G1(v) G1(l) / (4 cos_v), so the mean of the weight g (0 where !ok) over the draws is the float64 quadrature of that integral.
    4 x 10^5 draws around a random normal; the bar is 5 standard errors of the mean, from the draws.  Besides: g <= 1 everywhere, and no
    microfacet normal faces away from the view (dot3(dir, m) <= 0)"""
    n = 400000
    rng = np.random.default_rng(int(al * 1000) * 7 + int(cv * 100))
    ns = _unit(rng, 1).astype(np.float64)[0]
    tx = np.cross(ns, [0.3, -0.5, 0.8])
    tx /= np.linalg.norm(tx)
    v = np.sqrt(1.0 - cv * cv) * tx + cv * ns
    d = np.broadcast_to((-v).astype(F), (n, 3))
    nsf = np.broadcast_to(ns.astype(F), (n, 3))
    assert (gm._dot(d, nsf) < 0).all()
    m, nd, g, ok = gm.gloss_bounce(d, nsf, np.full(n, al, F), rng.random(n), rng.random(n))
    assert (g[ok] <= 1).all() and (g[ok] > 0).all()
    assert (gm._dot(d, m) <= 0).all()
    assert np.abs(np.sqrt(gm._dot(m, m).astype(np.float64)) - 1).max() < 1e-6
    wgt = np.where(ok, g, 0).astype(np.float64)
    want = _quadrature(al, float(gm._dot(d[:1], nsf[:1])[0]) * -1.0)
    se = wgt.std(ddof=1) / np.sqrt(n)
    z = (wgt.mean() - want) / se
    print(f"alpha {al} cos_v {cv}: mean g {wgt.mean():.6f}, quadrature {want:.6f}, se {se:.2e}, z {z:+.2f}, !ok {1 - ok.mean():.4f}")
    assert abs(z) <= 5, z


def test_f32_statement_against_float64():
    """the f32 statement against a float64 restatement of the same formulas (glossy_model.gloss_bounce64) on 2 x 10^6 random
    (dir, ns, alpha, u1, u2), compared where the float64 cl >= 1/16.  Measured with the model: max |m - m64| 9.8e-4, max |nd - nd64|
    1.7e-3, max |g - g64| 3.9e-5; the bar is 8 x the largest rounded up to a power of two (the project's rule, DESIGN.md sections 5.10
    and 5.11): 2^-6.  The largest differences sit at the disk's rim under a small alpha (u1 > 0.999, alpha < 0.02): z = sqrtf(z2) takes
    the root of a rounding error there (about 3e-4) and the unstretch divides it by alpha.  For u1 < 0.99 the three maxima are 1.1e-5,
    1.8e-5 and 2.7e-5"""
    n = 2000000
    d, ns, al, u1, u2 = _random_inputs(n, 41)
    m, nd, g, ok = gm.gloss_bounce(d, ns, al, u1, u2)
    m64, nd64, g64, cl64 = gm.gloss_bounce64(d, ns, al, u1, u2)
    k = cl64 >= 1.0 / 16
    assert k.mean() > 0.5 and ok[k].all()
    em, en, eg = np.abs(m[k] - m64[k]).max(), np.abs(nd[k] - nd64[k]).max(), np.abs(g[k] - g64[k]).max()
    print(f"max |m - m64| {em:.3e}, max |nd - nd64| {en:.3e}, max |g - g64| {eg:.3e} over {int(k.sum())} draws; bar {BAR:.3e}")
    assert max(em, en, eg) < BAR


def test_roughness_table_rule(tmp_path):
    t, m = scene.default_scene()
    n = t.shape[0]
    a = scene.roughness_table(t)
    assert a.dtype == F and a.shape == (n,) and (a == F(0.2)).all()
    a = scene.roughness_table(t, 0.5, which=[1, 2])
    assert (a[1:3] == F(0.5)).all() and a.sum() == 1 and (scene.roughness_table(t, 0.0) == 0).all()
    mask = np.zeros(n, bool)
    mask[3] = True
    per = np.linspace(0, 1, n).astype(F)
    a = scene.roughness_table(t, per, which=mask)
    assert a[3] == per[3] and np.count_nonzero(a) == 1
    for bad in (-0.1, 1.5, np.nan, np.inf):
        with pytest.raises(ValueError):
            scene.roughness_table(t, bad)
    p = str(tmp_path / "r.bin")
    scene.write_roughness(p, per)
    raw = open(p, "rb").read()
    assert raw[:4] == b"SPRG" and struct.unpack("<I", raw[4:8])[0] == n and raw[8:] == per.tobytes()


@pytest.mark.parametrize("est", sorted(ESTIMATORS))
@pytest.mark.parametrize("name", CASES)
def test_replay_cases_are_covered(name, est):
    _covered(_model(name, est)[3], name)


# ---------------------------------------------------------------------------------------------------------------- GPU part
@pytest.mark.gpu
def test_selftest_gloss():
    """what 11, the device function the kernels call, against the model bit for bit: random inputs and the blocks ns = +z and -z (both
    signs of the frame) and ns.z = -0, normal incidence (l2 = 0), grazing incidence (c about 0), alpha = 2^-10 and alpha = 1, u1 = 0"""
    n = 8192
    d, ns, al, u1, u2 = _random_inputs(n, 29)
    rng = np.random.default_rng(30)
    ns[0:256] = (0, 0, 1)
    ns[256:512] = (0, 0, -1)
    ns[512:768, 2] = -0.0
    ns[512:768] /= np.sqrt(gm._dot(ns[512:768], ns[512:768]))[:, None]
    d[0:768] = _unit(rng, 768)
    flip = gm._dot(d[0:768], ns[0:768]) > 0
    d[0:768][flip] *= F(-1)
    d[768:1024] = -ns[768:1024]                                     # normal incidence
    d[128:192] = -ns[128:192]                                       # ... along +z: l2 = 0 exactly
    graz = np.cross(ns[1024:1280].astype(np.float64), _unit(rng, 256).astype(np.float64))
    graz = graz / np.linalg.norm(graz, axis=1)[:, None] - 1e-4 * ns[1024:1280]
    d[1024:1280] = graz.astype(F)
    al[1280:1536] = 2.0 ** -10
    al[1536:1792] = 1.0
    al[0:64] = 1.0
    u1[1792:2048] = 0.0
    m, nd, g, ok = gm.gloss_bounce(d, ns, al, u1, u2)
    assert np.signbit(ns[512:768, 2]).all() and (np.abs(gm._dot(d[1024:1280], ns[1024:1280])) < 1e-3).all() and (~ok).sum() > 16
    q = np.concatenate([d.astype(np.float64), ns.astype(np.float64), al.astype(np.float64)[:, None], u1[:, None], u2[:, None]], 1)
    cx = capi.Context(0)
    got = cx.selftest(11, q, n).reshape(n, 8)
    cx.close()
    want = np.concatenate([m, nd, g[:, None], ok.astype(F)[:, None]], 1).astype(F)
    nan = np.isnan(want)
    assert not nan[ok].any() and nan.mean() < 0.01
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(_bits(got)[~nan], _bits(want)[~nan])


@pytest.mark.gpu
@pytest.mark.parametrize("est", sorted(ESTIMATORS))
@pytest.mark.parametrize("variant", [1, 16])
@pytest.mark.parametrize("name", CASES)
def test_model_bit_exact(name, variant, est):
    k = case(name)
    want_img, want_mean, want_scans, info = _model(name, est)
    _covered(info, name)
    c = _ctx(k)
    img, mean = c.render(hc.rays(), W, H, SPP, seed=REPLAY_SEED, flags=_flags(k) | ESTIMATORS[est] | variant, want_accum=True)
    st = c.stats()
    c.close()
    assert st["kernel_variant"] == variant
    assert np.array_equal(_bits(mean), _bits(want_mean))
    assert np.array_equal(img, want_img)
    assert st["scans_executed"] == want_scans


@pytest.mark.gpu
@pytest.mark.parametrize("est", sorted(ESTIMATORS))
@pytest.mark.parametrize("name", CASES)
def test_accel_parity(name, est):
    """variant 8: the BVH gives variant 16's image up to its rare rounding-noise accepts (at least 99 % of the pixels), and the flag
    matters there too"""
    k = case(name)
    c = _ctx(k)
    f = _flags(k) | ESTIMATORS[est]
    b = hc.check_accel_parity(c, f)
    assert c.stats()["kernel_variant"] == 8
    unflagged = c.render(hc.rays(), W, H, SPP, seed=3, flags=(f & ~GLOSSY) | capi.FLAG_ACCEL, want_accum=True)[1]
    c.close()
    assert not np.array_equal(_bits(b), _bits(unflagged))


@pytest.mark.gpu
@pytest.mark.parametrize("est", sorted(ESTIMATORS))
@pytest.mark.parametrize("tables", ["spec", "spec+glass", "spec+vn", "spec+glass+vn+env"])
@pytest.mark.parametrize("variant", [1, capi.FLAG_ACCEL, 16])
def test_zero_table_is_no_flag(variant, tables, est):
    """a table of zeros: the flagged render is the unflagged one bit for bit, scans included, from rays and, with and without camera
    samples, from a camera; with and without glass, normals and a map; and a real table matters"""
    t, m, s, vn = hc.smooth_case("bad_room", True)
    vn = vn if "vn" in tables else None
    f = ESTIMATORS[est] | variant | SPEC | (SMOOTH if vn is not None else 0)
    c = hc.ctx(t, m, s, vn)
    if "glass" in tables:
        c.set_dielectric(scene.dielectric_table(t, which=np.arange(14, 40)))
        f |= GLASS
    if "env" in tables:
        c.set_environment(env_model.replay_maps()["n3"])
        f |= ENV
    c.set_roughness(np.zeros(t.shape[0], F))
    hc.check_zero_table_is_no_flag(c, f, GLOSSY)
    c.set_roughness(scene.roughness_table(t, 0.3))
    rays = hc.rays()
    assert not hc.same(c.render(rays, W, H, SPP, seed=6, flags=f | GLOSSY, want_accum=True), c.render(rays, W, H, SPP, seed=6, flags=f, want_accum=True))
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("est", sorted(ESTIMATORS))
@pytest.mark.parametrize("name", ["mixed", "sphere"])
def test_both_block_shapes(shape, name, est):
    """variant 16 in its 256- and its 512-thread shape: the replay, a progressive and an adaptive split, primary-hit reuse, camera
    samples, and zero table = no flag; the tile size of the stream says which shape ran"""
    k = case(name)
    c = _ctx(k)
    hc.check_both_block_shapes(c, shape, ESTIMATORS[est] | 16 | (_flags(k) & ~GLOSSY), GLOSSY, _model(name, est)[:3],
                               lambda c: c.set_roughness(np.zeros_like(k["rough"])))
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("est", sorted(ESTIMATORS))
@pytest.mark.parametrize("variant", [16, capi.FLAG_ACCEL, 1])
def test_progressive_adaptive_denoise(variant, est):
    k = case("sphere")
    f = _flags(k) | ESTIMATORS[est] | variant
    c = _ctx(k)
    hc.check_progressive_adaptive_denoise(c, f)
    g1 = c.accum_gbuffer()
    c.accum_begin(rays=hc.rays(), w=W, h=H, seed=9, flags=f & ~GLOSSY, adaptive=(0.3, 0.05, 4))
    c.accum_step(4)
    assert c.accum_gbuffer().tobytes() == g1.tobytes()      # the G-buffer is unchanged
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("est", sorted(ESTIMATORS))
@pytest.mark.parametrize("variant", [1, capi.FLAG_ACCEL, 16])
def test_camera_samples_and_device_table(variant, est):
    """camera samples with the flag are the chain of one-sample accumulations over sphip_camera_rays_device's rays; the table comes
    from a device pointer here"""
    k = case("sphere")
    c = _ctx(k, rough=False)
    hc.set_device_table(c.set_roughness_device, k["rough"])
    hc.check_camera_samples(c, _flags(k) | ESTIMATORS[est] | variant)
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("est", sorted(ESTIMATORS))
@pytest.mark.parametrize("name", ["floor", "glass"])
def test_reuse_chunks_multi_device(name, est):
    """primary-hit reuse, sample chunks, variant 1 and multi-device contexts ({0,0} and {0,0,0}, one-shot and in two steps) give the
    single context's render; sphip_set_roughness ends a multi-device accumulation"""
    k = case(name)
    r = hc.rays()
    f = _flags(k) | ESTIMATORS[est]
    c = _ctx(k)
    want = c.render(r, W, H, SPP, seed=4, flags=f, want_accum=True)
    assert not hc.same(want, c.render(r, W, H, SPP, seed=4, flags=f & ~GLOSSY, want_accum=True))      # a real table changes the image
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
        mc.set_roughness(k["rough"])                  # ends the accumulation
        with pytest.raises(RuntimeError, match=E_STATE):
            mc.accum_step(1)
        mc.accum_begin(rays=r, w=W, h=H, seed=4, flags=f)
        img, mean, _ = mc.accum_step(SPP, want_mean=True)
        assert hc.same((img, mean), want), devs
        mc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("seed0", [100, 300])
@pytest.mark.parametrize("name", ["floor", "sphere"])
def test_unbiased_plain_vs_mis(name, seed0):
    """plain and NEE|MIS estimate one image of the glossy floor and of the glossy smooth sphere (hip_checks.z_grid: |z| < 4 for the
    image, < 5 per cell, 16 seeds x 256 spp at 32 x 32), for two disjoint sets of seeds"""
    k = case(name)
    w = h = 32
    rays = hc.rays(w, h)
    seeds = list(range(seed0, seed0 + 16))
    f = _flags(k)
    c = _ctx(k)
    a = hc.seeds_means(c, rays, w, h, 256, f | NEE_MIS, seeds)
    b = hc.seeds_means(c, rays, w, h, 256, f, seeds)
    c.close()
    hc.z_grid(a, b, h, w, f"glossy {name}: MIS vs plain, seeds {seed0}..{seed0 + 15}", alike_is_zero=True)


@pytest.mark.gpu
@pytest.mark.parametrize("est", sorted(ESTIMATORS))
def test_bounded_samples(est):
    """the glossy floor (p in {0, 1}, so wD = wS = 1): a diffuse bounce multiplies by 2 rho cos <= 2 rho and a glossy one by ks g <= ks,
    so with rho_max the larger of the reflectances and ks / 2 per channel no one-sample pixel exceeds
    sum_{d=0..4} (2 rho_max)^d (Le_max + 2 rho_max Le_max) (tests/test_hip_mis.py's bound; relative slack 1e-5 for f32 rounding),
    over 16 one-sample renders"""
    k = case("floor")
    mt = np.asarray(k["m"], np.float64)
    rho = np.maximum(mt[:, 0:3].max(0), 0.5 * np.asarray(k["s"], np.float64)[:, 0:3].max(0))
    le = mt[:, 3:6].max(0)
    bound = sum((2 * rho) ** d for d in range(5)) * (le + 2 * rho * le)
    c = _ctx(k)
    r = hc.rays()
    top = np.zeros(3)
    for seed in range(16):
        mean = c.render(r, W, H, 1, seed=seed, flags=_flags(k) | ESTIMATORS[est], want_accum=True)[1]
        top = np.maximum(top, mean.max(0))
    c.close()
    print("largest one-sample pixel", top, "bound", bound)
    assert (top <= bound * (1 + 1e-5)).all() and (top > 0).all()


@pytest.mark.gpu
def test_error_contract():
    k = case("floor")
    t, m, s, a = k["t"], k["m"], k["s"], k["rough"]
    rays = hc.rays()
    c = hc.ctx(t, m, s)
    L = capi.load()
    GS = GLOSSY | SPEC

    def refused(code, fn, text=None):
        with pytest.raises(RuntimeError, match=code) as e:
            fn()
        assert L.sphip_last_error(c._h), "sphip_last_error is set"
        assert text is None or text in str(e.value), str(e.value)
        c.render(rays, W, H, 1, seed=1)                    # the context stays usable

    refused(E_STATE, lambda: c.render(rays, W, H, 2, seed=1, flags=GS))                          # flag without table
    refused(E_STATE, lambda: c.accum_begin(rays=rays, w=W, h=H, seed=1, flags=GS))
    c.set_roughness(a)
    good = c.render(rays, W, H, 2, seed=1, flags=GS, want_accum=True)
    refused(E_INVALID, lambda: c.render(rays, W, H, 2, seed=1, flags=GLOSSY), "SPHIP_FLAG_SPECULAR")   # flag without _SPECULAR
    refused(E_INVALID, lambda: c.accum_begin(rays=rays, w=W, h=H, seed=1, flags=GLOSSY), "SPHIP_FLAG_SPECULAR")
    refused(E_INVALID, lambda: c.render(rays, W, H, 1, seed=1, mode=capi.MODE_FLAT, flags=GS))   # flag with FLAT
    refused(E_INVALID, lambda: c.render(rays, W, H, 2, seed=1, flags=GS | capi.FLAG_NEE))        # flag with NEE alone
    refused(E_INVALID, lambda: c.accum_begin(rays=rays, w=W, h=H, seed=1, flags=GS | capi.FLAG_NEE))
    for v in (2, 15, 9):                                                                         # the A/B scans, a retired variant
        refused(E_INVALID, lambda: c.render(rays, W, H, 2, seed=1, flags=GS | v))
        refused(E_INVALID, lambda: c.accum_begin(rays=rays, w=W, h=H, seed=1, flags=GS | v))
    # a call that breaks several rules hears of them in the established order: the environment's rule before this one's
    refused(E_STATE, lambda: c.render(rays, W, H, 2, seed=1, flags=GLOSSY | ENV), "SPHIP_FLAG_ENVIRONMENT")
    import torch                                                                                 # hit queries ignore the flag
    d_rays = torch.from_numpy(rays).to("cuda")
    hits = []
    for f in (0, GS, GLOSSY, GS | capi.FLAG_NEE, GS | 2):
        d_idx = torch.full((W * H,), -7, dtype=torch.int32, device="cuda")
        d_dist = torch.zeros(W * H, dtype=torch.float32, device="cuda")
        c.closest_hit_device(d_rays.data_ptr(), W * H, d_idx.data_ptr(), d_dist.data_ptr(), flags=f, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        hits.append((d_idx.cpu().numpy(), d_dist.cpu().numpy()))
    assert all(np.array_equal(h[0], hits[0][0]) and np.array_equal(_bits(h[1]), _bits(hits[0][1])) for h in hits) and (hits[0][0] >= 0).any()
    t2, m2, s2 = hc.mixed_room()                                                                 # bad rows, in a scene with a triangle 60
    c.set_scene(t2, m2)
    c.set_specular(s2)
    a2 = scene.roughness_table(t2, 0.3)
    c.set_roughness(a2)
    good2 = c.render(rays, W, H, 2, seed=1, flags=GS, want_accum=True)
    for bad in (-0.5, 1.5, np.nan, np.inf, -np.inf):
        ab = a2.copy()
        ab[40] = bad
        ab[60] = bad
        with pytest.raises(RuntimeError, match=E_INVALID) as e:
            c.set_roughness(ab)
        assert "triangle 40 " in str(e.value), str(e.value)
        assert hc.same(c.render(rays, W, H, 2, seed=1, flags=GS, want_accum=True), good2)            # the table stays as it was
    c.set_scene(t, m)
    c.set_specular(s)
    refused(E_STATE, lambda: c.render(rays, W, H, 2, seed=1, flags=GS))                          # set_scene cleared it
    c.set_roughness(a)
    # without the flag the table is ignored
    unflagged = c.render(rays, W, H, 2, seed=1, flags=SPEC, want_accum=True)
    c.set_roughness(None)
    refused(E_STATE, lambda: c.render(rays, W, H, 2, seed=1, flags=GS))                          # NULL cleared it
    assert hc.same(c.render(rays, W, H, 2, seed=1, flags=SPEC, want_accum=True), unflagged)
    assert not hc.same(unflagged, good)
    # set_roughness ends an accumulation, in the same way and with the same code as set_scene does
    c.set_roughness(a)
    c.accum_begin(rays=rays, w=W, h=H, seed=1, flags=GS)
    c.accum_step(2)
    c.set_scene(t, m)
    with pytest.raises(RuntimeError, match=E_STATE) as by_scene:
        c.accum_step(2)
    c.set_specular(s)
    c.set_roughness(a)
    c.accum_begin(rays=rays, w=W, h=H, seed=1, flags=GS)
    c.accum_step(2)
    c.set_roughness(a)
    with pytest.raises(RuntimeError, match=E_STATE) as by_table:
        c.accum_step(2)
    assert str(by_table.value) == str(by_scene.value)
    assert hc.same(c.render(rays, W, H, 2, seed=1, flags=GS, want_accum=True), good)
    c.close()
    # table before scene
    c = capi.Context(0)
    with pytest.raises(RuntimeError, match=E_STATE):
        c.set_roughness(a)
    with pytest.raises(RuntimeError, match=E_STATE):
        c.set_roughness_device(0)
    assert L.sphip_last_error(c._h)
    c.set_scene(t, m)
    c.set_specular(s)
    c.set_roughness(a)
    assert hc.same(c.render(rays, W, H, 2, seed=1, flags=GS, want_accum=True), good)
    with pytest.raises(ValueError):
        c.set_roughness(a[:3])
    c.close()
    # the device-pointer form on a multi-device context
    mc = capi.Context.multi([0, 0])
    mc.set_scene(t, m)
    mc.set_specular(s)
    with pytest.raises(RuntimeError, match=E_STATE):
        mc.set_roughness_device(0)
    assert L.sphip_last_error(mc._h)
    with pytest.raises(RuntimeError, match=E_STATE):
        mc.render(rays, W, H, 2, seed=1, flags=GS)
    ab = a.copy()
    ab[2] = 1.5
    with pytest.raises(RuntimeError, match=E_INVALID):
        mc.set_roughness(ab)
    mc.set_roughness(a)
    assert hc.same(mc.render(rays, W, H, 2, seed=1, flags=GS, want_accum=True), good)
    mc.close()


@pytest.mark.gpu
def test_cli_and_adapter(tmp_path):
    """spath_cli --rough FILE goes through hip_renderer::set_roughness and gives the capi image, one-shot, progressive, with --mis, with
    --glass and --normals beside it and on the camera path; the flat pass is unchanged; --rough without --spec, a table of the wrong
    size, a missing file and --nee alone are refused; the Python renderer mirrors the adapter"""
    import subprocess
    cli = os.path.join(ROOT, "spath_amd", "host", "build", "spath_cli")
    k = case("glass")
    t, m, s, g, a = k["t"], k["m"], k["s"], k["g"], k["rough"]
    vn = scene.vertex_normals(t, which=np.arange(7, t.shape[0]))
    sp, sg, ss, sn, sr = (str(tmp_path / x) for x in ("s.bin", "s.glass", "s.spec", "s.vn", "s.rough"))
    scene.write_scene(sp, t, m)
    scene.write_dielectric(sg, g)
    scene.write_specular(ss, s)
    scene.write_vertex_normals(sn, vn)
    scene.write_roughness(sr, a)
    w, h = 40, 24
    cam = view.Camera(w, h)
    rays = np.ascontiguousarray(cam.get_viewport(), dtype=F)
    c = hc.ctx(t, m, s, vn)
    c.set_dielectric(g)
    c.set_roughness(a)
    GS = GLOSSY | SPEC
    gl = c.render(rays, w, h, 8, seed=9, flags=GS)
    gl_mis = c.render(rays, w, h, 8, seed=9, flags=GS | NEE_MIS)
    gl_all = c.render(rays, w, h, 8, seed=9, flags=GS | GLASS | SMOOTH)
    gl_aa = c.render_camera(cam, 8, seed=9, flags=GS | capi.FLAG_CAMERA_SAMPLES)
    mirror = c.render(rays, w, h, 8, seed=9, flags=SPEC)
    flat = c.render(rays, w, h, 1, mode=capi.MODE_FLAT)
    c.close()
    assert len({gl.tobytes(), gl_mis.tobytes(), gl_all.tobytes(), gl_aa.tobytes(), mirror.tobytes()}) == 5
    base = [cli, "--scene", sp, "--w", str(w), "--h", str(h), "--spp", "8", "--seed", "9", "--spec", ss]
    for extra, want in ((["--rough", sr], gl), (["--rough", sr, "--progressive", "3"], gl), (["--rough", sr, "--mis"], gl_mis),
                        (["--rough", sr, "--glass", sg, "--normals", sn], gl_all), (["--rough", sr, "--aa"], gl_aa),
                        (["--rough", sr, "--mode", "flat"], flat), ([], mirror)):
        out = str(tmp_path / "o.rgba")
        subprocess.run(base + ["--out", out] + extra, check=True, capture_output=True, timeout=120)
        assert open(out, "rb").read() == want.tobytes(), extra
    scene.write_roughness(str(tmp_path / "short.rough"), a[:50])
    for bad in (["--rough", str(tmp_path / "short.rough")], ["--rough", str(tmp_path / "none.rough")], ["--rough", ss], ["--rough", sr, "--nee"]):
        r = subprocess.run(base + ["--out", str(tmp_path / "x.rgba")] + bad, capture_output=True, timeout=120)
        assert r.returncode != 0, bad
    r = subprocess.run(base[:-2] + ["--out", str(tmp_path / "x.rgba"), "--rough", sr], capture_output=True, timeout=120)   # without --spec
    assert r.returncode != 0 and b"--spec" in r.stderr + r.stdout
    from spath_amd import renderer
    r = renderer.HipRenderer(w, h, seed=9)                # the table turns the flag on, as in the adapter; the flat pass stays
    r.set_specular(s)
    r.set_roughness(a)
    out = renderer.Bitmap()
    r.render(renderer.Viewport(w, h, rays), t, m, t.shape[0], 8, out)
    assert np.asarray(out.values).tobytes() == gl.tobytes()
    r.render_flat(renderer.Viewport(w, h, rays), t, m, t.shape[0], 1, out)
    assert np.asarray(out.values).tobytes() == flat.tobytes()
    r.set_roughness(None)
    r.render(renderer.Viewport(w, h, rays), t, m, t.shape[0], 8, out)
    assert np.asarray(out.values).tobytes() == mirror.tobytes()
    r.close()
