"""Environment lighting on the device (include/spath_hip.h "environment lighting"): sphip_set_environment and its
device-pointer form, the importance tables the library builds behind both, the two device functions of the octahedral mapping
(sphip_selftest_device what 9 and 10), and SPHIP_FLAG_ENVIRONMENT in the path kernels.

The arithmetic is stated operation by operation in the header, so it is replayed in numpy (tests/env_model.py's steps in
tests/path_model.py's loop, its `env` map).  STATED TOLERANCE: 0 -- texel indices, r3, directions, wt, rc, marg, tpdf, T, w_env and W,
and the images, means and scans_executed of flagged renders, bit for bit.  Without the flag renders with a map set are held to the renders without one, bit for bit."""
import ctypes as C
import os

import numpy as np
import pytest

import env_model as em
import hip_checks as hc
import path_model
from oracle import oracle as O
from hip_checks import E_INVALID, E_STATE, ESTIMATORS, H, REPLAY_SEED, SPP, W, _torch_first, shape  # noqa: F401  (fixtures)
from path_model import F, _bits
from spath_amd import capi, scene, view

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = capi.FLAG_ENVIRONMENT

pytestmark = pytest.mark.gpu
SIZES = (1, 2, 3, 5, 64, 257)         # the non-powers of two and one size beyond a workgroup: where a row kernel's indexing can go wrong
_SCENE = {}


def _scene():
    if not _SCENE:
        _SCENE["open"] = scene.open_clutter(100)
    return _SCENE["open"]


def _random_map(n, seed=9):
    """random radiances with a few black texels and one black row (n >= 3), so that equal neighbours occur in rc and marg"""
    rng = np.random.default_rng(seed + n)
    tx = (rng.random((n, n, 3)) * 4).astype(F)
    tx[rng.random((n, n)) < 0.1] = 0
    if n >= 3:
        tx[n // 2] = 0
    return tx


def _edge_directions():
    """axis directions and the diagonal folds, a or b exactly 0 and +-1, d.y = +-0, unnormalised directions scaled by 2^-20 and 2^20, a zero
    and a NaN direction"""
    base = [[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]]
    base += [[sx, sy, sz] for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)]
    base += [[0, 1, 1], [0, -1, 1], [1, 1, 0], [1, -1, 0], [0, 1, -1], [-1, -1, 0], [0, 0.5, 0.5], [0.5, -0.5, 0]]     # a or b exactly 0
    base += [[1, 0.0, 1], [1, -0.0, 1], [-1, 0.0, 0.25], [-1, -0.0, 0.25], [0.3, -0.0, -0.7], [1, -1e-30, 1]]           # d.y = +-0: b or a +-1 on the rim
    base += [[3, 4, -5], [-0.3, -0.2, 0.7], [7, -1, 2]]
    d = np.array(base, F)
    d = np.concatenate([d, d * F(2.0 ** -20), d * F(2.0 ** 20), np.array([[0, 0, 0], [-0.0, 0, -0.0], [np.nan, 1, 0], [1, np.nan, np.nan], [np.inf, 1, 0]], F)])
    return d


def _same_dump(got, want_tab, want_sp):
    n = got["n"]
    assert n == want_tab["n"]
    for k in ("wt", "rc", "marg"):
        assert np.array_equal(got[k].view(np.uint64), want_tab[k].view(np.uint64)), (n, k)
    assert np.array_equal(_bits(got["tpdf"]), _bits(want_sp["tpdf"])), (n, "tpdf")
    assert (got["T"], got["w_env"], got["W"]) == (want_tab["T"], want_sp["w_env"], want_sp["W"]), n


@pytest.mark.parametrize("n", [3, 64, 2048])
def test_env_lookup_selftest(n):
    """what 9 against the model, 10^5 random directions of every scale and sign and the edge cases; only n enters the lookup"""
    rng = np.random.default_rng(n)
    d = (rng.standard_normal((100_000, 3)) * np.exp2(rng.integers(-8, 9, (100_000, 1)))).astype(F)
    d[rng.random(100_000) < 0.05, 1] = 0                      # the rim
    d = np.concatenate([_edge_directions(), d])
    c = capi.Context(0)
    c.set_environment(np.zeros((n, n, 3), F))
    got = c.selftest(9, d, d.shape[0]).reshape(-1, 4)
    c.close()
    i, j, r3, ok = em.lookup(d, n)
    assert np.array_equal(got[:, 3] != 0, ok) and ok.sum() == d.shape[0] - 5
    assert np.array_equal(got[:, 0], i.astype(F)) and np.array_equal(got[:, 1], j.astype(F))
    assert np.array_equal(_bits(got[:, 2]), _bits(r3))


@pytest.mark.parametrize("n", [3, 64])
def test_env_sample_selftest(n):
    """what 10 against the model on 10^5 uniform draws, with the ends of the interval; the sky map at n = 64, a random map at n = 3"""
    tx = scene.sky_environment(64) if n == 64 else _random_map(3)
    rng = np.random.default_rng(n)
    u = rng.random((100_000, 4))
    u[0], u[1], u[2] = 0.0, np.nextafter(1.0, 0.0), (0.0, np.nextafter(1.0, 0.0), 0.5, 0.0)
    c = capi.Context(0)
    c.set_environment(tx)
    got = c.selftest(10, u, u.shape[0]).reshape(-1, 6)
    c.close()
    tab = em.tables(tx)
    i, j, wd, r3 = em.sample(tab, *u.T)
    assert np.array_equal(got[:, 0], i.astype(F)) and np.array_equal(got[:, 1], j.astype(F))
    assert np.array_equal(_bits(got[:, 2:5]), _bits(wd)) and np.array_equal(_bits(got[:, 5]), _bits(r3))
    assert len(np.unique(j * n + i)) > (n * n) // 2            # the draws reach most of the map


@pytest.mark.parametrize("n", SIZES)
def test_tables_equal_the_model(n):
    t, m = _scene()
    tx = _random_map(n)
    c = hc.ctx(t, m)
    c.set_environment(tx)
    got = c.selftest_env_dump()
    c.close()
    tab = em.tables(tx)
    _same_dump(got, tab, em.scene_part(tab, t, m))
    assert got["T"] > 0 and 0 < got["w_env"] < got["W"]


def test_one_lit_texel_takes_every_sample():
    """a map black but for texel (3, 2) of 5 x 5: every one of 10^4 samples lands on it, r8 = r9 = 0 included; black rows and leading
    black texels are never chosen"""
    tx = np.zeros((5, 5, 3), F)
    tx[2, 3] = (1, 2, 3)
    u = np.random.default_rng(11).random((10_000, 4))
    u[0] = 0.0
    u[1, 0:2] = np.nextafter(1.0, 0.0)
    c = capi.Context(0)
    c.set_environment(tx)
    got = c.selftest(10, u, u.shape[0]).reshape(-1, 6)
    look = c.selftest(9, np.ascontiguousarray(got[:, 2:5]), u.shape[0]).reshape(-1, 4)
    c.close()
    assert (got[:, 0] == 3).all() and (got[:, 1] == 2).all()
    assert (look[:, 0] == 3).all() and (look[:, 1] == 2).all() and (look[:, 3] == 1).all()


def test_black_map_adds_no_entry():
    """an all-zero map: T = 0, no entry in the light table (w_env = 0, W the triangles' own), tpdf zeros"""
    t, m = _scene()
    c = hc.ctx(t, m)
    c.set_environment(np.zeros((3, 3, 3), F))
    got = c.selftest_env_dump()
    c.close()
    assert got["T"] == 0 and got["w_env"] == 0 and got["W"] == scene.light_table(t, m)[3]
    assert not got["tpdf"].any() and not got["marg"].any()


def test_set_scene_keeps_the_map_and_the_scene_part_follows():
    t, m = _scene()
    t2, m2 = scene.closed_room(200)
    tx = scene.sky_environment(64)
    tab = em.tables(tx)
    c = hc.ctx(t, m)
    c.set_environment(tx)
    a = c.selftest_env_dump()
    c.set_scene(t2, m2)
    b = c.selftest_env_dump()
    c.close()
    _same_dump(a, tab, em.scene_part(tab, t, m))
    _same_dump(b, tab, em.scene_part(tab, t2, m2))
    assert a["w_env"] != b["w_env"] and a["W"] != b["W"]


def test_host_and_device_setter_agree():
    import torch
    t, m = _scene()
    tx = _random_map(64)
    c = hc.ctx(t, m)
    c.set_environment(tx)
    a = c.selftest_env_dump()
    c.set_environment(None)
    d = torch.from_numpy(tx).to("cuda")
    c.set_environment_device(d.data_ptr(), 64, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    del d                                                      # the texels were copied
    b = c.selftest_env_dump()
    c.close()
    for k in ("wt", "rc", "marg", "tpdf", "T", "w_env", "W"):
        assert np.array_equal(a[k], b[k]), k


def test_multi_device_context_takes_the_map():
    t, m = _scene()
    tx = _random_map(5)
    mc = hc.ctx(t, m, devs=[0, 0])
    mc.set_environment(tx)
    got = mc.selftest_env_dump()
    look = mc.selftest(9, np.array([[0, 1, 0]], F), 1)
    with pytest.raises(capi.SpathHipError, match=E_STATE):
        mc.set_environment_device(1, 5)
    mc.close()
    tab = em.tables(tx)
    _same_dump(got, tab, em.scene_part(tab, t, m))
    assert look.tolist() == [2, 2, 1, 1]


def test_error_contract():
    t, m = _scene()
    tx = _random_map(5)
    tab = em.tables(tx)
    c = capi.Context(0)
    L, h = c._L, c._h
    buf = np.zeros(3, F)
    with pytest.raises(capi.SpathHipError, match=E_STATE):     # no map yet
        c.selftest(9, np.zeros((1, 3), F), 1)
    with pytest.raises(capi.SpathHipError, match=E_STATE):
        c.selftest(10, np.zeros((1, 4)), 1)
    c.set_environment(tx)
    with pytest.raises(capi.SpathHipError, match=E_STATE):     # a map, no scene
        c.selftest_env_dump()
    c.set_scene(t, m)
    assert L.sphip_set_environment(h, buf.ctypes.data, 0) == -1                 # n == 0
    assert L.sphip_set_environment(h, buf.ctypes.data, 2049) == -1 and b"2049" in L.sphip_last_error(h)     # n > 2048: refused before a texel is read
    for bad in (-1.0, np.nan, np.inf):
        x = tx.copy()
        x[3, 1, 2] = bad                                       # texel (1, 3), component 2; a later bad texel is not the one named
        x[4, 4, 0] = -2
        with pytest.raises(capi.SpathHipError, match=r"\[-1\].*texel \(1, 3\) has component 2"):
            c.set_environment(x)
    _same_dump(c.selftest_env_dump(), tab, em.scene_part(tab, t, m))           # the map stayed as it was
    import torch
    st = torch.cuda.current_stream().cuda_stream
    d = torch.from_numpy(tx).to("cuda")
    for n in (0, 2049):                                        # the device form checks n too, and leaves no map behind
        c.set_environment(tx)
        with pytest.raises(capi.SpathHipError, match=E_INVALID):
            c.set_environment_device(d.data_ptr(), n, st)
        with pytest.raises(capi.SpathHipError, match=E_STATE):
            c.selftest_env_dump()
    c.set_environment(tx)
    c.set_environment(None)                                    # NULL clears the map
    with pytest.raises(capi.SpathHipError, match=E_STATE):
        c.selftest_env_dump()
    with pytest.raises(ValueError):
        c.set_environment(np.zeros((4, 5, 3), F))
    c.close()


def test_unflagged_renders_do_not_read_the_map_and_an_accumulation_ends():
    """without the flag image, mean and scans_executed with a map are those without, for the plain estimator and NEE|MIS;
    set during an accumulation it ends the accumulation, as sphip_set_specular does"""
    t, m = _scene()
    r = hc.rays()
    c = hc.ctx(t, m)
    want = {}
    for f in (0, hc.NEE_MIS):
        want[f] = (c.render(r, W, H, SPP, seed=hc.REPLAY_SEED, flags=f, want_accum=True), c.stats()["scans_executed"])
    c.set_environment(scene.sky_environment(64))
    for f in (0, hc.NEE_MIS):
        got = c.render(r, W, H, SPP, seed=hc.REPLAY_SEED, flags=f, want_accum=True)
        assert hc.same(got, want[f][0]) and c.stats()["scans_executed"] == want[f][1]
    c.accum_begin(rays=r, w=W, h=H, seed=4)
    c.accum_step(1)
    c.set_environment(None)
    with pytest.raises(capi.SpathHipError, match=E_STATE):
        c.accum_step(1)
    c.close()


# ---------------------------------------------------------------------------------------------------------------- the flag in the kernels
_MODEL = {}
MAPS = em.replay_maps()


def _replay_scene(name, tables):
    return em.replay_scene(name, tables, hc.mixed_table)


def _model(name, tables, mp, est):
    key = (name, tables, mp, est)
    if key not in _MODEL:
        t, m, s, vn, g = _replay_scene(name, tables)
        _MODEL[key] = path_model.render(hc.rays(), t, m, SPP, REPLAY_SEED, est, s, vn, g, MAPS[mp])
    return _MODEL[key]


def test_flag_value():
    assert ENV == 0x1000000 and not ENV & (0xFFFF | capi.flag_chunks(255))


def test_orientation_by_hand():
    """one triangle behind the camera, a 4 x 4 map of 16 distinct colours, plain estimator, 1 spp: every pixel is the RGBA8 of the texel
    its primary ray's env_lookup names; a camera turned to +y sees the centre texels, one turned to -y the corners"""
    t = np.zeros((1, 12), F)
    t[0, :9] = [-1, -1, -50, 1, -1, -50, 0, 1, -50]
    t = scene.flat_normals(t)
    m = np.full((1, 6), 0.5, F)
    env = (np.arange(48, dtype=F).reshape(4, 4, 3) + 1) / F(64)
    c = hc.ctx(t, m, env=env)
    seen = {}
    for tag, rot in (("ahead", (0.0, 0.0, 0.0)), ("up", (-np.pi / 2, 0.0, 0.0)), ("down", (np.pi / 2, 0.0, 0.0))):
        cam = view.Camera(24, 16)
        cam.set_delta_rot(rot)
        r = np.ascontiguousarray(cam.get_viewport(), dtype=F)
        assert (O.closest_hits(r, t, np.full(r.shape[0], -1, np.int32))[0] < 0).all(), tag
        img = c.render(r, 24, 16, 1, seed=1, flags=ENV | 1)
        i, j, _, ok = em.lookup(r[:, 3:6], 4)
        assert ok.all()
        want = (np.clip(env[j, i], 0, 1) * F(255) + F(0.5)).astype(np.uint32).astype(np.uint8)
        assert np.array_equal(img[:, :3], want), tag
        seen[tag] = (float(r[:, 4].mean()), set(zip(i.tolist(), j.tolist())))
    c.close()
    centre, corners = {(1, 1), (1, 2), (2, 1), (2, 2)}, {(0, 0), (0, 3), (3, 0), (3, 3)}
    assert abs(seen["ahead"][0]) < 0.1
    assert seen["up"][0] > 0.9 and seen["up"][1] == centre, seen["up"]
    assert seen["down"][0] < -0.9 and seen["down"][1] == corners, seen["down"]


def _replay(name, mp, tables, variant, est, shape=None):
    t, m, s, vn, g = _replay_scene(name, tables)
    want_img, want_mean, want_scans, info = _model(name, tables, mp, est)
    em.covered(info, name, tables, est)
    c = hc.ctx(t, m, s, vn, glass=g, env=MAPS[mp])
    img, mean = c.render(hc.rays(), W, H, SPP, seed=REPLAY_SEED, flags=hc.table_flags(s, vn, g) | ENV | ESTIMATORS[est] | variant, want_accum=True)
    st = c.stats()
    if shape is not None:
        assert hc._tiles(c)[1] == shape
    c.close()
    assert st["kernel_variant"] == (8 if variant == capi.FLAG_ACCEL else variant)
    print("pixels that differ from the model:", (_bits(mean) != _bits(want_mean)).any(1).sum(), "scans", st["scans_executed"], want_scans)
    assert np.array_equal(_bits(mean), _bits(want_mean))
    assert np.array_equal(img, want_img)
    assert st["scans_executed"] == want_scans


@pytest.mark.parametrize("est", sorted(ESTIMATORS))
@pytest.mark.parametrize("variant", [1, capi.FLAG_ACCEL])
@pytest.mark.parametrize("tables", [False, True])
@pytest.mark.parametrize("mp", sorted(MAPS))
@pytest.mark.parametrize("name", ["open", "glass"])
def test_replay(name, mp, tables, variant, est):
    """48 x 32 x 4 spp, seed 3: image, mean and scans_executed are the model's (variants 1 and 8)"""
    _replay(name, mp, tables, variant, est)


@pytest.mark.parametrize("est", sorted(ESTIMATORS))
@pytest.mark.parametrize("tables", [False, True])
@pytest.mark.parametrize("mp", sorted(MAPS))
@pytest.mark.parametrize("name", ["open", "glass"])
def test_replay_default_scan(shape, name, mp, tables, est):
    """the same for variant 16, under both forced shapes of the default scan"""
    _replay(name, mp, tables, 16, est, shape)


@pytest.mark.parametrize("est", sorted(ESTIMATORS))
@pytest.mark.parametrize("variant", [1, capi.FLAG_ACCEL, 16])
def test_zero_map_is_no_flag(variant, est):
    """an all-zero map: the flagged render is the unflagged one bit for bit, scans included, from rays and from a camera with and without
    camera samples; and a real map matters"""
    t, m = _scene()
    c = hc.ctx(t, m, env=np.zeros((5, 5, 3), F))
    f = ESTIMATORS[est] | variant
    hc.check_zero_table_is_no_flag(c, f, ENV)
    c.set_environment(scene.sky_environment(64))
    r = hc.rays()
    assert not hc.same(c.render(r, W, H, SPP, seed=6, flags=f | ENV, want_accum=True), c.render(r, W, H, SPP, seed=6, flags=f, want_accum=True))
    c.close()


@pytest.mark.parametrize("est", sorted(ESTIMATORS))
def test_both_block_shapes(shape, est):
    t, m, s, vn, g = _replay_scene("glass", True)
    env = MAPS["sky64"]
    c = hc.ctx(t, m, s, vn, glass=g, env=env)
    hc.check_both_block_shapes(c, shape, ESTIMATORS[est] | 16 | hc.table_flags(s, vn, g), ENV, _model("glass", True, "sky64", est)[:3],
                               lambda c: c.set_environment(np.zeros_like(env)))
    c.close()


@pytest.mark.parametrize("est", sorted(ESTIMATORS))
@pytest.mark.parametrize("variant", [16, capi.FLAG_ACCEL, 1])
def test_progressive_adaptive_denoise(variant, est):
    t, m, s, vn, g = _replay_scene("glass", True)
    f = hc.table_flags(s, vn, g) | ENV | ESTIMATORS[est] | variant
    c = hc.ctx(t, m, s, vn, glass=g, env=MAPS["sky64"])
    hc.check_progressive_adaptive_denoise(c, f)
    g1 = c.accum_gbuffer()
    c.accum_begin(rays=hc.rays(), w=W, h=H, seed=9, flags=f & ~ENV, adaptive=(0.3, 0.05, 4))
    c.accum_step(4)
    assert c.accum_gbuffer().tobytes() == g1.tobytes()      # the G-buffer is unchanged
    c.close()


@pytest.mark.parametrize("est", sorted(ESTIMATORS))
@pytest.mark.parametrize("variant", [1, capi.FLAG_ACCEL, 16])
def test_camera_samples_and_device_setter(variant, est):
    """camera samples with the flag are the chain of one-sample accumulations over sphip_camera_rays_device's rays; the map comes from a
    device pointer here, and gives the image the host setter gives"""
    import torch
    t, m, s, vn, g = _replay_scene("open", True)
    env = MAPS["sky64"]
    f = hc.table_flags(s, vn, g) | ENV | ESTIMATORS[est] | variant
    c = hc.ctx(t, m, s, vn, glass=g, env=env)
    want = c.render(hc.rays(), W, H, SPP, seed=5, flags=f, want_accum=True)
    c.set_environment(None)
    d = torch.from_numpy(env).to("cuda")
    c.set_environment_device(d.data_ptr(), 64, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    del d
    assert hc.same(c.render(hc.rays(), W, H, SPP, seed=5, flags=f, want_accum=True), want)
    hc.check_camera_samples(c, f)
    c.close()


@pytest.mark.parametrize("est", sorted(ESTIMATORS))
def test_reuse_chunks_multi_device(est):
    """primary-hit reuse, sample chunks, variant 1 and multi-device contexts give the single context's render; sphip_set_environment ends
    a multi-device accumulation.  The clauses are hip_checks.check_reuse_chunks_multi_device's, written out because it builds its own
    contexts, without a dielectric table or a map"""
    t, m, s, vn, g = _replay_scene("glass", False)
    env = MAPS["sky64"]
    r = hc.rays()
    f = hc.table_flags(s, vn, g) | ENV | ESTIMATORS[est]
    c = hc.ctx(t, m, s, vn, glass=g, env=env)
    want = c.render(r, W, H, SPP, seed=4, flags=f, want_accum=True)
    assert not hc.same(want, c.render(r, W, H, SPP, seed=4, flags=f & ~ENV, want_accum=True))
    for extra in (capi.FLAG_PRIMARY_REUSE, capi.flag_chunks(1), capi.flag_chunks(4), capi.flag_chunks(3) | capi.FLAG_PRIMARY_REUSE, 1, 1 | capi.FLAG_PRIMARY_REUSE):
        assert hc.same(c.render(r, W, H, SPP, seed=4, flags=f | extra, want_accum=True), want), extra
    c.close()
    for devs in ([0, 0], [0, 0, 0]):
        mc = hc.ctx(t, m, s, vn, devs, g, env)
        got = mc.render(r, W, H, SPP, seed=4, flags=f, want_accum=True)
        mc.accum_begin(rays=r, w=W, h=H, seed=4, flags=f)
        mc.accum_step(1)
        img, mean, _ = mc.accum_step(SPP - 1, want_mean=True)
        assert hc.same(got, want), devs
        assert hc.same((img, mean), want), devs
        mc.set_environment(env)                         # ends the accumulation
        with pytest.raises(RuntimeError, match=E_STATE):
            mc.accum_step(1)
        mc.close()


@pytest.mark.parametrize("est", sorted(ESTIMATORS))
def test_accel_parity(est):
    t, m, s, vn, g = _replay_scene("glass", True)
    c = hc.ctx(t, m, s, vn, glass=g, env=MAPS["sky64"])
    hc.check_accel_parity(c, hc.table_flags(s, vn, g) | ENV | ESTIMATORS[est])
    assert c.stats()["kernel_variant"] == 8
    c.close()


def test_set_scene_keeps_the_map_and_the_flagged_table_follows():
    """after a set_scene the flagged render is the model's for the new scene under the old map"""
    t, m = scene.closed_room(200)
    c = hc.ctx(t, m, env=MAPS["sky64"])
    c.render(hc.rays(), W, H, 1, seed=1, flags=ENV | hc.NEE_MIS)
    t2, m2, s, vn, g = _replay_scene("open", False)
    c.set_scene(t2, m2)
    got = c.render(hc.rays(), W, H, SPP, seed=REPLAY_SEED, flags=ENV | hc.NEE_MIS, want_accum=True)
    scans = c.stats()["scans_executed"]
    c.close()
    want = _model("open", False, "sky64", "mis")
    assert hc.same(got, want[:2]) and scans == want[2]


def test_flag_error_contract():
    """one assertion per clause: E_INVALID with the flat mode, with NEE without MIS and with any other variant; E_STATE for the flag
    without a map; hit queries ignore the flag"""
    t, m = _scene()
    r = hc.rays()
    c = hc.ctx(t, m)
    with pytest.raises(capi.SpathHipError, match=E_STATE):
        c.render(r, W, H, 1, flags=ENV)
    with pytest.raises(capi.SpathHipError, match=E_STATE):
        c.accum_begin(rays=r, w=W, h=H, seed=1, flags=ENV)
    c.set_environment(MAPS["n3"])
    with pytest.raises(capi.SpathHipError, match=E_INVALID):
        c.render(r, W, H, 1, mode=capi.MODE_FLAT, flags=ENV)
    with pytest.raises(capi.SpathHipError, match=E_INVALID):
        c.render(r, W, H, 1, flags=ENV | capi.FLAG_NEE)
    for variant in (2, 15):
        with pytest.raises(capi.SpathHipError, match=E_INVALID):
            c.render(r, W, H, 1, flags=ENV | variant)
    c.render(r, W, H, 1, flags=ENV)
    import torch
    d_r = torch.from_numpy(r).to("cuda")
    hits = []
    for f in (0, ENV, ENV | capi.FLAG_NEE):                    # hit queries ignore the flag
        d_i, d_d = torch.zeros(W * H, dtype=torch.int32, device="cuda"), torch.zeros(W * H, dtype=torch.float32, device="cuda")
        c.closest_hit_device(d_r.data_ptr(), W * H, d_i.data_ptr(), d_d.data_ptr(), flags=f, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        hits.append((d_i.cpu().numpy().tobytes(), d_d.cpu().numpy().tobytes()))
    assert hits[0] == hits[1] == hits[2]
    c.set_environment(None)
    with pytest.raises(capi.SpathHipError, match=E_STATE):
        c.render(r, W, H, 1, flags=ENV)
    c.close()


def _seed_means(c, r, f, seeds, spp=256):
    return hc.seeds_means(c, r, 32, 32, spp, f, seeds)


@pytest.mark.parametrize("case", ["open_clutter_sky", "window_room"])
def test_one_expectation(case):
    """NEE|MIS minus plain, 16 seeds x 256 spp at 32 x 32, the project's bars (4 for the image, 5 per cell).  Measured on an MI355X
    (DESIGN.md section 5.11 records the z values)"""
    t, m = scene.open_clutter(100) if case == "open_clutter_sky" else em.window_room()
    seeds = range(500, 516) if case == "open_clutter_sky" else range(700, 716)
    r = hc.rays(32, 32)
    c = hc.ctx(t, m, env=MAPS["sky64"])
    a = _seed_means(c, r, ENV | hc.NEE_MIS, seeds)
    b = _seed_means(c, r, ENV, seeds)
    c.close()
    hc.z_grid(a, b, 32, 32, case, alike_is_zero=case == "window_room")     # cells that see only sky through the window: Le itself under both


def test_sun_scene_bound_and_variance():
    """every 1-spp NEE|MIS render over 16 seeds stays within sum_{d=0..4} (2 rho)^d 2 rho Le per channel on every pixel whose primary ray
    hits geometry; and at 64 spp the per-pixel sample variance (from the adaptive statistics' luminance proxy) summed over those pixels is
    lower under NEE|MIS than under the plain estimator"""
    t, m, env = em.sun_scene()
    r = hc.rays(32, 32)
    c = hc.ctx(t, m, env=env)
    on = O.closest_hits(r, t, np.full(r.shape[0], -1, np.int32))[0] >= 0
    assert on.sum() > 300
    rho = float(m[:, 0:3].max())
    bound = sum((2 * rho) ** d for d in range(5)) * 2 * rho * float(env.max())
    worst = 0.0
    for seed in range(16):
        mean = c.render(r, 32, 32, 1, seed=seed, flags=ENV | hc.NEE_MIS, want_accum=True)[1]
        worst = max(worst, float(mean[on].max()))
    print("largest 1-spp NEE|MIS value", worst, "bound", bound)
    assert worst <= bound
    var = {}
    for tag, f in (("mis", ENV | hc.NEE_MIS), ("plain", ENV)):
        smp = np.stack([c.render(r, 32, 32, 1, seed=100 + k, flags=f, want_accum=True)[1].astype(np.float64).sum(1) for k in range(64)])
        var[tag] = float(smp[:, on].var(0, ddof=1).sum())
    c.close()
    print("summed per-pixel sample variance: plain", var["plain"], "NEE|MIS", var["mis"], "ratio", var["plain"] / var["mis"])
    assert var["mis"] < var["plain"]


def test_cli_and_python_renderer(tmp_path):
    """spath_cli --env FILE goes through hip_renderer::set_environment and gives the C-ABI image, with and without --mis; it is refused with
    --mode flat and with --nee alone; the Python renderer mirrors the adapter"""
    import subprocess
    cli = os.path.join(ROOT, "spath_amd", "host", "build", "spath_cli")
    t, m = _scene()
    env = MAPS["sky64"]
    sp, se = str(tmp_path / "s.bin"), str(tmp_path / "s.env")
    scene.write_scene(sp, t, m)
    scene.write_environment(se, env)
    w, h = 40, 24
    rays = np.ascontiguousarray(view.Camera(w, h).get_viewport(), dtype=F)
    c = hc.ctx(t, m, env=env)
    lit = c.render(rays, w, h, 8, seed=9, flags=ENV)
    lit_mis = c.render(rays, w, h, 8, seed=9, flags=ENV | hc.NEE_MIS)
    plain = c.render(rays, w, h, 8, seed=9)
    flat = c.render(rays, w, h, 1, mode=capi.MODE_FLAT)
    c.close()
    assert len({lit.tobytes(), lit_mis.tobytes(), plain.tobytes()}) == 3
    base = [cli, "--scene", sp, "--w", str(w), "--h", str(h), "--spp", "8", "--seed", "9"]
    for extra, want in ((["--env", se], lit), (["--env", se, "--progressive", "3"], lit), (["--env", se, "--mis"], lit_mis), ([], plain)):
        out = str(tmp_path / "o.rgba")
        subprocess.run(base + ["--out", out] + extra, check=True, capture_output=True, timeout=120)
        assert open(out, "rb").read() == want.tobytes(), extra
    for bad in (["--env", se, "--mode", "flat"], ["--env", se, "--nee"], ["--env", sp], ["--env", str(tmp_path / "none.env")]):
        q = subprocess.run(base + ["--out", str(tmp_path / "x.rgba")] + bad, capture_output=True, timeout=120)
        assert q.returncode != 0, bad
    from spath_amd import renderer
    r = renderer.HipRenderer(w, h, seed=9)
    r.set_environment(env)
    out = renderer.Bitmap()
    r.render(renderer.Viewport(w, h, rays), t, m, t.shape[0], 8, out)
    assert np.asarray(out.values).tobytes() == lit.tobytes()
    r.render_flat(renderer.Viewport(w, h, rays), t, m, t.shape[0], 1, out)
    assert np.asarray(out.values).tobytes() == flat.tobytes()
    r.set_environment(None)
    r.render(renderer.Viewport(w, h, rays), t, m, t.shape[0], 8, out)
    assert np.asarray(out.values).tobytes() == plain.tobytes()
    r.close()
