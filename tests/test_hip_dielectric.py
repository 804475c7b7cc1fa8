"""Transparency (include/spath_hip.h: SPHIP_FLAG_DIELECTRIC with sphip_set_dielectric): a per-triangle table
kt.r kt.g kt.b ior; a triangle with ior >= 1 is a smooth interface between vacuum and a dielectric that reflects with the Fresnel
probability and transmits by Snell's law otherwise.

The arithmetic is stated operation by operation in the header, so it is replayed in numpy (tests/dielectric_model.py's interface in
tests/path_model.py's loop, its `glass` table).  STATED TOLERANCE: 0 -- images, means and scan counts bit for bit.  The statistical bar
(plain against NEE|MIS) is the project's: hip_checks.z_grid over 16 seeds x 256 spp at 32 x 32.  The f32 statement is held to float64
Snell/Fresnel at 2^-16 (test_f32_statement_against_float64 says where the figure comes from).

CPU part: the flag and the symbols; the model with a table of zeros against the model without a table; a slab by hand; the f32
statement against float64; scene.dielectric_table; the coverage of the replay cases; the BVH case's noise accepts.
GPU part: the selftest; the replay for variants 1 and 16, both estimators; zero table = no flag; both workgroup shapes; the
compositions; the BVH's parity; one expectation; the error contract; the front ends."""
import ctypes as C
import os

import numpy as np
import pytest

import dielectric_model as dm
import hip_checks as hc
import path_model
from hip_checks import E_INVALID, E_STATE, ESTIMATORS, NEE_MIS, REPLAY_SEED, SPP, H, W, _torch_first, shape  # noqa: F401  (fixtures)
from path_model import F, _bits
from spath_amd import capi, scene, view

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GLASS = capi.FLAG_DIELECTRIC
SPEC = capi.FLAG_SPECULAR
SMOOTH = capi.FLAG_SMOOTH
KT = (0.5, 0.25, 1.0)
BAR = 2.0 ** -16                                      # test_f32_statement_against_float64
_MODEL = {}


# ---------------------------------------------------------------------------------------------------------------- scenes
def slab_scene():
    """a glass slab between z = 1 (triangle 0, normal -z) and z = 2 (triangle 1, normal +z), kt = (0.5, 0.25, 1), ior = 1.5, an emitter
    E = (2, 3, 0.75) in z = 4, and one ray from the origin along +z"""
    def tri(z, nz):
        v = np.array([[-10, -10, z], [10, -10, z], [0, 20, z]], np.float64)
        if np.cross(v[1] - v[0], v[2] - v[0])[2] * nz < 0:
            v = v[[0, 2, 1]]
        return v.ravel()
    t = np.zeros((3, 12), F)
    t[0, :9], t[1, :9], t[2, :9] = tri(1, -1), tri(2, 1), tri(4, -1)
    t = scene.flat_normals(t)
    assert t[0, 11] == -1 and t[1, 11] == 1
    m = np.zeros((3, 6), F)
    m[0:2, 0:3] = 0.5                                 # ignored on an interface
    m[2, 3:6] = (2.0, 3.0, 0.75)
    g = np.zeros((3, 4), F)
    g[0:2] = KT + (1.5,)
    return t, m, g, np.array([[0, 0, 0, 0, 0, 1]], F)


def sphere_scene(smooth, mixed):
    """default_scene plus icosphere(1) of glass (kt tinted, ior 1.5) at hip_checks.SPHERE_C / SPHERE_R, flat or with vertex normals on
    the sphere, with nothing or hip_checks.mixed_table elsewhere -> (tris, mats, spec or None, vn or None, glass)"""
    t, m, s, vn = hc.sphere_scene(False)
    g = scene.dielectric_table(t, 1.5, (0.9, 0.95, 1.0), which=np.arange(7, t.shape[0]))
    if mixed:
        s[7:, 3] = 1                                  # mixed_table leaves the sphere's rows alone; they are ignored on an interface
        s = hc.mixed_table(t, m, s)
    return t, m, (s if mixed else None), (vn if smooth else None), g


def _model(smooth, mixed, est):
    """the replay's reference, computed once per case"""
    key = (smooth, mixed, est)
    if key not in _MODEL:
        t, m, s, vn, g = sphere_scene(smooth, mixed)
        _MODEL[key] = path_model.render(hc.rays(), t, m, SPP, REPLAY_SEED, est, s, vn, g, collect=("accepts",))
    return _MODEL[key]


def _covered(info, smooth):
    """a replay case proves something only where its rules fire: interfaces hit, transmissions, total internal reflections, an emitter
    reached straight after glass, samples that cross two interfaces or more; under smooth shading each of the three ending rules"""
    for k in ("glass", "transmit", "tir", "emitter_after_glass", "two_transmissions"):
        assert info[k] > 0, (k, info)
    assert info["transmit"] < info["glass"]
    if smooth:
        for k in ("sm", "ended_glass_c", "ended_glass_reflect", "ended_glass_transmit"):
            assert info[k] > 0, (k, info)


# ---------------------------------------------------------------------------------------------------------------- CPU part
def test_flag_value_and_symbols():
    assert capi.FLAG_DIELECTRIC == 0x8000
    assert capi.FLAG_DIELECTRIC & (capi.FLAG_NEE | capi.FLAG_MIS | capi.FLAG_ACCEL | capi.FLAG_PRIMARY_REUSE | capi.FLAG_CAMERA_SAMPLES |
                                   capi.FLAG_SPECULAR | capi.FLAG_SMOOTH | 0xFF | 0xFF0000) == 0
    assert {"sphip_set_dielectric", "sphip_set_dielectric_device"} <= set(capi.SYMBOLS)
    lib = C.CDLL(capi.LIB_PATH)
    assert hasattr(lib, "sphip_set_dielectric") and hasattr(lib, "sphip_set_dielectric_device")
    assert capi.load().sphip_abi_version() == 3
    hdr = open(os.path.join(ROOT, "include", "spath_hip.h")).read()
    assert "SPHIP_FLAG_DIELECTRIC = 0x8000" in hdr


def test_null_context_and_triangle_limit():
    """what sphip_set_dielectric checks without a device: a null context is SPHIP_E_INVALID for both forms.  The limit of 2^29
    triangles is a host check in front of everything else; a scene of that size (24 GiB of triangles) is out of a test's reach, so
    the bit it protects and the refusal's text are read from the sources and the library"""
    L = capi.load()
    g = np.zeros(4, F)
    assert L.sphip_set_dielectric(None, None) == -1
    assert L.sphip_set_dielectric(None, g.ctypes.data) == -1
    assert L.sphip_set_dielectric_device(None, None, None) == -1
    src = open(os.path.join(ROOT, "spath_amd", "csrc", "sp_integrator.h")).read()
    assert "constexpr int kTransBit = 0x20000000;" in src and "constexpr int kSpecBit = 0x40000000;" in src
    assert b"a dielectric table needs a scene of fewer than 2^29 triangles" in open(capi.LIB_PATH, "rb").read()
    # the limit is the dielectric row's max_tris (sp_host_tables.h), held to the bit when the library is compiled, and both forms of
    # the one setter check it
    rows = open(os.path.join(ROOT, "spath_amd", "csrc", "sp_host_tables.h")).read()
    assert '(size_t)1 << 29, "a dielectric table needs a scene of fewer than 2^29 triangles (this one has %zu)"' in rows
    host = open(os.path.join(ROOT, "spath_amd", "csrc", "spath_hip.hip")).read()
    import re
    assert re.search(r"static_assert\([^;]*kTriTables\[kTabDielectric\]\.max_tris == \(size_t\)sp::kTransBit", host)
    assert host.count("c->n_tris >= t.max_tris") == 2                     # set_table and set_table_device


@pytest.mark.parametrize("tables", ["none", "spec", "vn", "spec+vn"])
def test_zero_table_is_no_table(tables):
    """a dielectric table of zeros (whatever kt) executes the step and changes nothing: the bits, the scans and every counter of the
    call without the table, for every estimator that takes one, with and without a specular table and vertex normals"""
    t, m, s, vn = hc.smooth_case("diffuse_sphere", True)
    s, vn = (s if "spec" in tables else None), (vn if "vn" in tables else None)
    rays = hc.rays(16, 12)
    z = np.zeros((t.shape[0], 4), F)
    z[:, 0:3] = 0.6                                   # kt alone changes nothing
    for est in sorted(ESTIMATORS):
        want, want_scans, wi = path_model.samples(rays, t, m, 5, 1, 3, est, s, vn)
        rec, scans, info = path_model.samples(rays, t, m, 5, 1, 3, est, s, vn, z)
        assert np.array_equal(_bits(rec), _bits(want)) and scans == want_scans, est
        assert info["glass"] == 0 and info == wi, est
    # zero dielectric table = zero specular table = no table
    if tables == "none":
        for est in sorted(ESTIMATORS):
            a = path_model.samples(rays, t, m, 5, 1, 3, est, None, None, z)
            b = path_model.samples(rays, t, m, 5, 1, 3, est, np.zeros_like(z))
            assert np.array_equal(_bits(a[0]), _bits(b[0])) and a[1] == b[1], est


@pytest.mark.parametrize("est", sorted(ESTIMATORS))
def test_slab_by_hand(est):
    """one ray through a glass slab onto an emitter: every sample is exactly kt * kt * E = (0.5, 0.1875, 0.75) or 0 under both
    estimators, and the non-zero share lies within 5 binomial standard deviations of T^2 (1 + R^2), R = 0.04, T = 0.96 (straight
    through, or once back and forth inside): 0.92307 +- 0.021 at 4096 samples"""
    t, m, g, ray = slab_scene()
    n = 4096
    rec, scans, info = path_model.samples(ray, t, m, 5, 0, n, est, glass=g)
    want = np.asarray(KT, F) * (np.asarray(KT, F) * m[2, 3:6])
    assert list(want) == [F(0.5), F(0.1875), F(0.75)]
    lit = rec[0].any(1)
    assert np.array_equal(_bits(rec[0][lit]), np.broadcast_to(_bits(want), (int(lit.sum()), 3)))
    R, T = 0.04, 0.96
    p = T * T * (1 + R * R)
    share = lit.mean()
    print(f"slab, {est}: non-zero share {share:.5f} of {n} (expected {p:.5f}), {scans} scans, {info['glass']} interface hits")
    assert abs(share - p) < 5 * np.sqrt(p * (1 - p) / n), share
    assert info["tir"] == 0 and info["emitter_after_glass"] >= int(lit.sum()) and info["lights"] == 0
    assert (int(lit.sum()), scans) == (3786, 18639)           # seed 5: pinned, the same under both estimators (no shadow ray is ever traced)


def _random_interfaces(n, seed):
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d = (d / np.sqrt((d * d).sum(1))[:, None]).astype(F)
    ns = rng.normal(size=(n, 3))
    ns = (ns / np.sqrt((ns * ns).sum(1))[:, None]).astype(F)
    flip = path_model._dot(ns, d) > F(0)
    ns[flip] = ns[flip] * F(-1)
    ior = np.asarray([1.1, 1.33, 1.5, 2.4], F)[rng.integers(0, 4, n)]
    return d, ns, ior, rng.integers(0, 2, n).astype(bool)


def test_f32_statement_against_float64():
    """the header's f32 statement against float64 Snell/Fresnel on the same f32 inputs: 2 * 10^6 random unit dir / ns, ior in {1.1,
    1.33, 1.5, 2.4}, both sides.  The TIR decision agrees on every input; where k >= 1/16 and ci >= 1/16 (near the critical angle and
    at grazing incidence the error is unbounded) |Fr - Fr64| and |nt - nt64| stay below the bar.
    MEASURED with this model and seed: max |Fr - Fr64| = 1.779e-6, max |nt - nt64| = 1.586e-6 over the 1 228 141 inputs inside the
    restriction.  The bar is 8 x the larger (1.42e-5) rounded up to a power of two: 2^-16 = 1.53e-5; the margin covers other random draws.  Normal incidence at ior = 1.5 gives Fr within it of 0.04"""
    d, ns, ior, ent = _random_interfaces(2_000_000, 17)
    Fr, tir, nt, c = dm.dielectric(d, ns, ior, ent)
    Fr64, tir64, nt64 = dm.dielectric64(d, ns, ior, ent)
    assert np.array_equal(tir, tir64), int((tir != tir64).sum())
    eta = np.where(ent, F(1) / ior, ior).astype(F)
    ci = -c
    k = F(1) - (eta * eta) * (F(1) - ci * ci)
    ok = (k >= F(1 / 16)) & (ci >= F(1 / 16))
    assert 0.5 * ok.size < ok.sum() < ok.size and tir.sum() > 0.05 * ok.size
    eF = np.abs(Fr[ok].astype(np.float64) - Fr64[ok]).max()
    eN = np.abs(nt[ok].astype(np.float64) - nt64[ok]).max()
    print(f"max |Fr - Fr64| = {eF:.3e}, max |nt - nt64| = {eN:.3e} over {int(ok.sum())} inputs; bar {BAR:.3e}")
    assert eF < BAR and eN < BAR
    z = np.array([[0, 0, 1]], F)
    for e in (True, False):
        Fr0, tir0, nt0, _ = dm.dielectric(z, -z, np.array([1.5], F), np.array([e]))
        assert not tir0[0] and abs(float(Fr0[0]) - 0.04) < BAR and np.abs(nt0[0] / np.sqrt((nt0[0] ** 2).sum()) - z[0]).max() < BAR


def test_dielectric_table_rule(tmp_path):
    t, m = scene.closed_room(50)
    g = scene.dielectric_table(t)
    assert g.dtype == F and g.shape == (50, 4) and (g == np.asarray([1, 1, 1, 1.5], F)).all()
    g = scene.dielectric_table(t, 1.33, (0.5, 0.25, 1.0), which=[3, 7])
    assert np.flatnonzero(g.any(1)).tolist() == [3, 7] and list(g[7]) == [F(0.5), F(0.25), F(1.0), F(1.33)]
    mask = np.zeros(50, bool)
    mask[10:20] = True
    assert np.flatnonzero(scene.dielectric_table(t, np.full(50, 2.4, F), 0.0, which=mask)[:, 3]).tolist() == list(range(10, 20))
    assert list(scene.dielectric_table(t, 1.0)[0]) == [1, 1, 1, 1]
    for bad in (dict(ior=0.9), dict(ior=0.0), dict(ior=np.nan), dict(ior=np.inf), dict(kt=-0.1), dict(kt=np.nan), dict(kt=(1, np.inf, 1))):
        with pytest.raises(ValueError):
            scene.dielectric_table(t, **bad)
    p = str(tmp_path / "g.bin")
    scene.write_dielectric(p, g)
    raw = open(p, "rb").read()
    assert raw[:4] == b"SPDI" and int.from_bytes(raw[4:8], "little") == 50 and raw[8:] == g.tobytes()


@pytest.mark.parametrize("est", sorted(ESTIMATORS))
@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("smooth", [False, True])
def test_replay_cases_are_covered(smooth, mixed, est):
    info = _model(smooth, mixed, est)[3]
    print(smooth, mixed, est, {k: v for k, v in info.items() if k != "accepts"})
    _covered(info, smooth)


@pytest.mark.parametrize("est", sorted(ESTIMATORS))
def test_accel_parity_scene_keeps_noise_accepts_rare(est):
    """the BVH against variant 16 is asked for 99 % of the pixels (DESIGN.md section 5.8's preparation): on the CPU model of the very
    render test_accel_geometric_parity compares, u and v recomputed in double at every hit the float test accepts, path and shadow
    rays alike; the hits whose exact point lies outside their triangle stay far below 1 % of the pixels"""
    from test_hip_smooth import noise_accept_share
    t = sphere_scene(True, True)[0]
    info = _model(True, True, est)[3]
    share, n = noise_accept_share(info["accepts"], t)
    print(f"glass sphere, smooth, mixed, {est}: noise accepts {share:.5f} of {n} accepted hits ({share * n:.0f} hits, {W * H} pixels)")
    assert n >= info["hits"] and share * n < 0.001 * W * H, (share, n)


# ---------------------------------------------------------------------------------------------------------------- GPU part
@pytest.mark.gpu
def test_selftest_dielectric():
    """what 8, the device function the kernels call, against the model bit for bit: random interfaces, total internal reflection,
    grazing incidence (ci = 0) and ior = 1.  Under tir Fr and nt mean nothing (a NaN's payload is not the statement's): NaN there
    must meet NaN, everything else its bits"""
    n = 8192
    d, ns, ior, ent = _random_interfaces(n, 23)
    d[0:64] = (1, 0, 0)
    ns[0:64] = (0, 1, 0)                              # grazing: ci = 0
    ior[64:128] = 1.0                                 # no interface at all: Fr = 0 and nt = dir up to rounding
    ent[128:192] = False
    ior[128:192] = 2.4                                # from inside diamond: mostly tir
    Fr, tir, nt, c = dm.dielectric(d, ns, ior, ent)
    assert tir[128:192].sum() > 32 and 0.1 * n < tir.sum() < 0.5 * n and (c[0:64] == 0).all()
    assert not tir[64:128].any() and np.abs(nt[64:128] - d[64:128]).max() < 1e-5 and Fr[64:128].max() < 1e-9   # up to rounding
    q = np.concatenate([d, ns, ior[:, None], ent.astype(F)[:, None]], 1).astype(F)
    cx = capi.Context(0)
    got = cx.selftest(8, q, n).reshape(n, 6)
    cx.close()
    want = np.concatenate([Fr[:, None], tir.astype(F)[:, None], nt, c[:, None]], 1).astype(F)
    nan = np.isnan(want)
    assert not nan[~tir].any()
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(_bits(got)[~nan], _bits(want)[~nan])


@pytest.mark.gpu
@pytest.mark.parametrize("est", sorted(ESTIMATORS))
@pytest.mark.parametrize("variant", [1, 16])
def test_slab_bit_exact(variant, est):
    """the hand scene: W x H copies of the one ray (the pixel keys the draws), image, mean and scans"""
    t, m, g, ray = slab_scene()
    rays = np.ascontiguousarray(np.broadcast_to(ray, (W * H, 6)))
    want_img, want_mean, want_scans, info = path_model.render(rays, t, m, SPP, REPLAY_SEED, est, glass=g)
    assert info["transmit"] > 0 and info["emitter_after_glass"] > 0 and info["glass"] > info["transmit"]
    c = hc.ctx(t, m, glass=g)
    img, mean = c.render(rays, W, H, SPP, seed=REPLAY_SEED, flags=GLASS | ESTIMATORS[est] | variant, want_accum=True)
    st = c.stats()
    c.close()
    assert st["kernel_variant"] == variant
    assert np.array_equal(_bits(mean), _bits(want_mean))
    assert np.array_equal(img, want_img)
    assert st["scans_executed"] == want_scans


@pytest.mark.gpu
@pytest.mark.parametrize("est", sorted(ESTIMATORS))
@pytest.mark.parametrize("variant", [1, 16])
@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("smooth", [False, True])
def test_model_bit_exact(smooth, mixed, variant, est):
    t, m, s, vn, g = sphere_scene(smooth, mixed)
    want_img, want_mean, want_scans, info = _model(smooth, mixed, est)
    _covered(info, smooth)
    c = hc.ctx(t, m, s, vn, glass=g)
    img, mean = c.render(hc.rays(), W, H, SPP, seed=REPLAY_SEED, flags=hc.table_flags(s, vn, g) | ESTIMATORS[est] | variant, want_accum=True)
    st = c.stats()
    c.close()
    assert st["kernel_variant"] == variant
    assert np.array_equal(_bits(mean), _bits(want_mean))
    assert np.array_equal(img, want_img)
    assert st["scans_executed"] == want_scans


@pytest.mark.gpu
@pytest.mark.parametrize("est", sorted(ESTIMATORS))
@pytest.mark.parametrize("tables", ["none", "spec", "vn", "spec+vn"])
@pytest.mark.parametrize("variant", [1, capi.FLAG_ACCEL, 16])
def test_zero_table_is_no_flag(variant, tables, est):
    """a table of zeros (whatever kt): the flagged render is the unflagged one bit for bit, scans included, from rays and, with and
    without camera samples, from a camera; with and without the other two tables; and a real table matters"""
    t, m, s, vn = hc.smooth_case("bad_room", True)
    s, vn = (s if "spec" in tables else None), (vn if "vn" in tables else None)
    f = ESTIMATORS[est] | variant | (SPEC if s is not None else 0) | (SMOOTH if vn is not None else 0)
    z = np.zeros((t.shape[0], 4), F)
    z[:, 0:3] = 0.7
    c = hc.ctx(t, m, s, vn, glass=z)
    hc.check_zero_table_is_no_flag(c, f, GLASS)
    c.set_dielectric(scene.dielectric_table(t, which=np.arange(14, t.shape[0])))
    rays = hc.rays()
    assert not hc.same(c.render(rays, W, H, SPP, seed=6, flags=f | GLASS, want_accum=True), c.render(rays, W, H, SPP, seed=6, flags=f, want_accum=True))
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("est", sorted(ESTIMATORS))
@pytest.mark.parametrize("smooth", [False, True])
def test_both_block_shapes(shape, smooth, est):
    """variant 16 in its 256- and its 512-thread shape: the replay, a progressive and an adaptive split, primary-hit reuse, camera
    samples, and zero table = no flag; the tile size of the stream says which shape ran"""
    t, m, s, vn, g = sphere_scene(smooth, True)
    c = hc.ctx(t, m, s, vn, glass=g)
    hc.check_both_block_shapes(c, shape, ESTIMATORS[est] | 16 | (hc.table_flags(s, vn, g) & ~GLASS), GLASS, _model(smooth, True, est)[:3],
                               lambda c: c.set_dielectric(np.zeros_like(g)))
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("est", sorted(ESTIMATORS))
@pytest.mark.parametrize("variant", [16, capi.FLAG_ACCEL, 1])
def test_progressive_adaptive_denoise(variant, est):
    t, m, s, vn, g = sphere_scene(True, True)
    f = hc.table_flags(s, vn, g) | ESTIMATORS[est] | variant
    c = hc.ctx(t, m, s, vn, glass=g)
    hc.check_progressive_adaptive_denoise(c, f)
    g1 = c.accum_gbuffer()
    c.accum_begin(rays=hc.rays(), w=W, h=H, seed=9, flags=f & ~GLASS, adaptive=(0.3, 0.05, 4))
    c.accum_step(4)
    assert c.accum_gbuffer().tobytes() == g1.tobytes()      # the G-buffer is unchanged
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("est", sorted(ESTIMATORS))
@pytest.mark.parametrize("variant", [1, capi.FLAG_ACCEL, 16])
def test_camera_samples_and_device_table(variant, est):
    """camera samples with the flag are the chain of one-sample accumulations over sphip_camera_rays_device's rays; the table comes
    from a device pointer here"""
    t, m, s, vn, g = sphere_scene(True, True)
    c = hc.ctx(t, m, s, vn)
    hc.set_device_table(c.set_dielectric_device, g)
    hc.check_camera_samples(c, hc.table_flags(s, vn, g) | ESTIMATORS[est] | variant)
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("est", sorted(ESTIMATORS))
@pytest.mark.parametrize("smooth", [False, True])
def test_reuse_chunks_multi_device(smooth, est):
    """primary-hit reuse, sample chunks, variant 1 and multi-device contexts ({0,0} and {0,0,0}, one-shot and in two steps) give the
    single context's render; sphip_set_dielectric ends a multi-device accumulation"""
    t, m, s, vn, g = sphere_scene(smooth, False)
    r = hc.rays()
    f = hc.table_flags(s, vn, g) | ESTIMATORS[est]
    c = hc.ctx(t, m, s, vn, glass=g)
    want = c.render(r, W, H, SPP, seed=4, flags=f, want_accum=True)
    assert not hc.same(want, c.render(r, W, H, SPP, seed=4, flags=f & ~GLASS, want_accum=True))
    for extra in (capi.FLAG_PRIMARY_REUSE, capi.flag_chunks(1), capi.flag_chunks(4), capi.flag_chunks(3) | capi.FLAG_PRIMARY_REUSE, 1, 1 | capi.FLAG_PRIMARY_REUSE):
        assert hc.same(c.render(r, W, H, SPP, seed=4, flags=f | extra, want_accum=True), want), extra
    c.close()
    for devs in ([0, 0], [0, 0, 0]):
        mc = hc.ctx(t, m, s, vn, devs, glass=g)
        got = mc.render(r, W, H, SPP, seed=4, flags=f, want_accum=True)
        mc.accum_begin(rays=r, w=W, h=H, seed=4, flags=f)
        mc.accum_step(1)
        img, mean, _ = mc.accum_step(SPP - 1, want_mean=True)
        assert hc.same(got, want), devs
        assert hc.same((img, mean), want), devs
        mc.set_dielectric(g)                          # ends the accumulation
        with pytest.raises(RuntimeError, match=E_STATE):
            mc.accum_step(1)
        mc.accum_begin(rays=r, w=W, h=H, seed=4, flags=f)
        img, mean, _ = mc.accum_step(SPP, want_mean=True)
        assert hc.same((img, mean), want), devs
        mc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("est", sorted(ESTIMATORS))
def test_accel_geometric_parity(est):
    """the BVH gives variant 16's image up to its rare rounding-noise accepts: at least 99 % of the pixels"""
    t, m, s, vn, g = sphere_scene(True, True)
    c = hc.ctx(t, m, s, vn, glass=g)
    f = hc.table_flags(s, vn, g) | ESTIMATORS[est]
    b = hc.check_accel_parity(c, f)
    assert c.stats()["kernel_variant"] == 8
    unflagged = c.render(hc.rays(), W, H, SPP, seed=3, flags=(f & ~GLASS) | capi.FLAG_ACCEL, want_accum=True)[1]
    c.close()
    assert not np.array_equal(_bits(b), _bits(unflagged))


@pytest.mark.gpu
@pytest.mark.parametrize("seed0", [100, 300])
@pytest.mark.parametrize("smooth", [False, True])
def test_unbiased_plain_vs_mis(smooth, seed0):
    """plain and NEE|MIS estimate one image of the glass sphere (hip_checks.z_grid: |z| < 4 for the image, < 5 per cell, 16 seeds x
    256 spp at 32 x 32), flat and smooth, for two disjoint sets of seeds"""
    t, m, s, vn, g = sphere_scene(smooth, False)
    w = h = 32
    rays = hc.rays(w, h)
    seeds = list(range(seed0, seed0 + 16))
    f = hc.table_flags(s, vn, g)
    c = hc.ctx(t, m, s, vn, glass=g)
    a = hc.seeds_means(c, rays, w, h, 256, f | NEE_MIS, seeds)
    b = hc.seeds_means(c, rays, w, h, 256, f, seeds)
    c.close()
    hc.z_grid(a, b, h, w, f"glass sphere {'smooth' if smooth else 'flat'}: MIS vs plain, seeds {seed0}..{seed0 + 15}", alike_is_zero=True)


@pytest.mark.gpu
def test_error_contract():
    t, m, s, vn, g = sphere_scene(False, False)
    rays = hc.rays()
    c = hc.ctx(t, m)
    L = capi.load()

    def refused(code, fn):
        with pytest.raises(RuntimeError, match=code):
            fn()
        assert L.sphip_last_error(c._h), "sphip_last_error is set"
        c.render(rays, W, H, 1, seed=1)                    # the context stays usable

    refused(E_STATE, lambda: c.render(rays, W, H, 2, seed=1, flags=GLASS))                      # flag without table
    refused(E_STATE, lambda: c.accum_begin(rays=rays, w=W, h=H, seed=1, flags=GLASS))
    c.set_dielectric(g)
    good = c.render(rays, W, H, 2, seed=1, flags=GLASS, want_accum=True)
    refused(E_INVALID, lambda: c.render(rays, W, H, 1, seed=1, mode=capi.MODE_FLAT, flags=GLASS))   # flag with FLAT
    refused(E_INVALID, lambda: c.render(rays, W, H, 2, seed=1, flags=GLASS | capi.FLAG_NEE))        # flag with NEE alone
    refused(E_INVALID, lambda: c.accum_begin(rays=rays, w=W, h=H, seed=1, flags=GLASS | capi.FLAG_NEE))
    for v in (2, 15, 9):                                                                         # the A/B scans, an unshipped variant
        refused(E_INVALID, lambda: c.render(rays, W, H, 2, seed=1, flags=GLASS | v))
        refused(E_INVALID, lambda: c.accum_begin(rays=rays, w=W, h=H, seed=1, flags=GLASS | v))
    import torch                                                                                 # hit queries ignore the flag
    d_rays = torch.from_numpy(rays).to("cuda")
    hits = []
    for f in (0, GLASS, GLASS | capi.FLAG_NEE, GLASS | 2):
        d_idx = torch.full((W * H,), -7, dtype=torch.int32, device="cuda")
        d_dist = torch.zeros(W * H, dtype=torch.float32, device="cuda")
        c.closest_hit_device(d_rays.data_ptr(), W * H, d_idx.data_ptr(), d_dist.data_ptr(), flags=f, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        hits.append((d_idx.cpu().numpy(), d_dist.cpu().numpy()))
    assert all(np.array_equal(h[0], hits[0][0]) and np.array_equal(_bits(h[1]), _bits(hits[0][1])) for h in hits) and (hits[0][0] >= 7).any()
    for col, bad in ((0, -0.5), (1, np.nan), (2, np.inf), (3, 0.5), (3, -1.5), (3, np.nan), (3, np.inf)):   # bad rows
        gb = g.copy()
        gb[40, col] = bad
        gb[60, col] = bad
        with pytest.raises(RuntimeError, match=E_INVALID) as e:
            c.set_dielectric(gb)
        assert "triangle 40 " in str(e.value), str(e.value)
        assert hc.same(c.render(rays, W, H, 2, seed=1, flags=GLASS, want_accum=True), good)          # the table stays as it was
    # without the flag the table is ignored
    c.set_dielectric(None)
    refused(E_STATE, lambda: c.render(rays, W, H, 2, seed=1, flags=GLASS))                      # NULL cleared it
    unflagged = c.render(rays, W, H, 2, seed=1, want_accum=True)
    c.set_dielectric(g)
    assert hc.same(c.render(rays, W, H, 2, seed=1, want_accum=True), unflagged)
    # set_scene clears the table
    c.set_scene(t, m)
    refused(E_STATE, lambda: c.render(rays, W, H, 2, seed=1, flags=GLASS))
    # set_dielectric ends an accumulation, in the same way and with the same code as set_scene does
    c.set_dielectric(g)
    c.accum_begin(rays=rays, w=W, h=H, seed=1, flags=GLASS)
    c.accum_step(2)
    c.set_scene(t, m)
    with pytest.raises(RuntimeError, match=E_STATE) as by_scene:
        c.accum_step(2)
    c.set_dielectric(g)
    c.accum_begin(rays=rays, w=W, h=H, seed=1, flags=GLASS)
    c.accum_step(2)
    c.set_dielectric(g)
    with pytest.raises(RuntimeError, match=E_STATE) as by_table:
        c.accum_step(2)
    assert str(by_table.value) == str(by_scene.value)
    assert hc.same(c.render(rays, W, H, 2, seed=1, flags=GLASS, want_accum=True), good)
    c.close()
    # table before scene
    c = capi.Context(0)
    with pytest.raises(RuntimeError, match=E_STATE):
        c.set_dielectric(g)
    with pytest.raises(RuntimeError, match=E_STATE):
        c.set_dielectric_device(0)
    assert L.sphip_last_error(c._h)
    c.set_scene(t, m)
    c.set_dielectric(g)
    assert hc.same(c.render(rays, W, H, 2, seed=1, flags=GLASS, want_accum=True), good)
    with pytest.raises(ValueError):
        c.set_dielectric(g[:50])
    c.close()
    # the device-pointer form on a multi-device context
    mc = capi.Context.multi([0, 0])
    mc.set_scene(t, m)
    with pytest.raises(RuntimeError, match=E_STATE):
        mc.set_dielectric_device(0)
    assert L.sphip_last_error(mc._h)
    with pytest.raises(RuntimeError, match=E_STATE):
        mc.render(rays, W, H, 2, seed=1, flags=GLASS)
    gb = g.copy()
    gb[40, 3] = 0.5
    with pytest.raises(RuntimeError, match=E_INVALID):
        mc.set_dielectric(gb)
    mc.set_dielectric(g)
    assert hc.same(mc.render(rays, W, H, 2, seed=1, flags=GLASS, want_accum=True), good)
    mc.close()


@pytest.mark.gpu
def test_cli_and_adapter(tmp_path):
    """spath_cli --glass FILE goes through hip_renderer::set_dielectric and gives the capi image, one-shot, progressive, with --mis,
    with --spec and --normals beside it and on the camera path; the flat pass is unchanged; a table of the wrong size, a missing file
    and --nee alone are refused; the Python renderer mirrors the adapter"""
    import subprocess
    cli = os.path.join(ROOT, "spath_amd", "host", "build", "spath_cli")
    t, m, s, vn, g = sphere_scene(True, True)
    sp, sg, ss, sn = str(tmp_path / "s.bin"), str(tmp_path / "s.glass"), str(tmp_path / "s.spec"), str(tmp_path / "s.vn")
    scene.write_scene(sp, t, m)
    scene.write_dielectric(sg, g)
    scene.write_specular(ss, s)
    scene.write_vertex_normals(sn, vn)
    w, h = 40, 24
    cam = view.Camera(w, h)
    rays = np.ascontiguousarray(cam.get_viewport(), dtype=F)
    c = hc.ctx(t, m, s, vn, glass=g)
    glass = c.render(rays, w, h, 8, seed=9, flags=GLASS)
    glass_mis = c.render(rays, w, h, 8, seed=9, flags=GLASS | NEE_MIS)
    glass_all = c.render(rays, w, h, 8, seed=9, flags=GLASS | SPEC | SMOOTH)
    glass_aa = c.render_camera(cam, 8, seed=9, flags=GLASS | capi.FLAG_CAMERA_SAMPLES)
    plain = c.render(rays, w, h, 8, seed=9)
    flat = c.render(rays, w, h, 1, mode=capi.MODE_FLAT)
    c.close()
    assert len({glass.tobytes(), glass_mis.tobytes(), glass_all.tobytes(), glass_aa.tobytes(), plain.tobytes()}) == 5
    base = [cli, "--scene", sp, "--w", str(w), "--h", str(h), "--spp", "8", "--seed", "9"]
    for extra, want in ((["--glass", sg], glass), (["--glass", sg, "--progressive", "3"], glass), (["--glass", sg, "--mis"], glass_mis),
                        (["--glass", sg, "--spec", ss, "--normals", sn], glass_all), (["--glass", sg, "--aa"], glass_aa),
                        (["--glass", sg, "--mode", "flat"], flat), ([], plain)):
        out = str(tmp_path / "o.rgba")
        subprocess.run(base + ["--out", out] + extra, check=True, capture_output=True, timeout=120)
        assert open(out, "rb").read() == want.tobytes(), extra
    scene.write_dielectric(str(tmp_path / "short.glass"), g[:50])
    for bad in (["--glass", str(tmp_path / "short.glass")], ["--glass", str(tmp_path / "none.glass")], ["--glass", ss], ["--glass", sg, "--nee"]):
        r = subprocess.run(base + ["--out", str(tmp_path / "x.rgba")] + bad, capture_output=True, timeout=120)
        assert r.returncode != 0, bad
    from spath_amd import renderer
    r = renderer.HipRenderer(w, h, seed=9)                # the table turns the flag on, as in the adapter; the flat pass stays
    r.set_dielectric(g)
    out = renderer.Bitmap()
    r.render(renderer.Viewport(w, h, rays), t, m, t.shape[0], 8, out)
    assert np.asarray(out.values).tobytes() == glass.tobytes()
    r.render_flat(renderer.Viewport(w, h, rays), t, m, t.shape[0], 1, out)
    assert np.asarray(out.values).tobytes() == flat.tobytes()
    r.set_dielectric(None)
    r.render(renderer.Viewport(w, h, rays), t, m, t.shape[0], 8, out)
    assert np.asarray(out.values).tobytes() == plain.tobytes()
    r.close()
