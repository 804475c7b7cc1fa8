"""Specular reflection (include/spath_hip.h: SPHIP_FLAG_SPECULAR with sphip_set_specular): a per-triangle table
ks.r ks.g ks.b p; a hit takes the mirror lobe with probability p and the unchanged diffuse lobe otherwise.

The estimator is stated operation by operation in the header, so it is replayed here in numpy on top of the NEE and MIS replays'
pieces (tests/test_hip_nee.py, tests/test_hip_mis.py): closest hits of path and shadow rays through the oracle's strict scan, draws
and diffuse directions through the oracle's device math, every other step in f32 in the stated order.  STATED TOLERANCE: 0 --
images, means and scan counts bit for bit.  The one statistical bar (unbiasedness in p, and plain against NEE|MIS on a mirror
scene) is the project's: |z| < 5 in every cell of a 4 x 4 grid over 16 seeds x 256 spp, as tests/test_hip_mis.py::test_unbiased.

CPU part: the flag and the symbols; the model by hand on a three-triangle scene and against the plain and MIS models with a table of
zeros; the coverage the replay cases need; scene.specular_table; what sphip_set_specular checks without a device.
GPU part: the replay for variants 1, 2, 15, 16, both estimators and three scenes; zero table = no flag for every shipped variant;
variant 16 in both workgroup shapes (forced as tests/test_hip_shapes.py does);
the BVH's geometric parity; composition with progressive and adaptive accumulation, denoising, chunks, primary-hit reuse,
multi-device contexts and camera samples; unbiasedness; the error contract; the front ends."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import oracle as O
from spath_amd import capi, scene, view
from test_hip_nee import E_INVALID, INV_P, INV_PI, MARGIN, SPP, H, W, _bits, _dot, _philox, _rays, _unit_vec
from test_hip_mis import TWO_PI, NEE_MIS, _u
from test_hip_mis import model_samples as mis_model_samples

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_STATE = r"\[-3\]"
SPEC = capi.FLAG_SPECULAR
ESTIMATORS = {"plain": 0, "mis": NEE_MIS}


def model_samples(rays, tris, mats, spec, seed, s0, n, mis):
    """radiance [npix, n, 3] of global samples s0 .. s0 + n - 1 with the specular table `spec` under the plain estimator or NEE|MIS,
    the scans (path + shadow) they take, and what the samples met: {"spec_then_hit": samples with a specular bounce whose ray hit
    something, "emitter_after_spec": samples that reached an emitter directly after a specular bounce, "samples": all}"""
    tris = np.ascontiguousarray(tris, F).reshape(-1, 12)
    mats = np.ascontiguousarray(mats, F).reshape(-1, 6)
    spec = np.ascontiguousarray(spec, F).reshape(-1, 4)
    rays = np.ascontiguousarray(rays, F).reshape(-1, 6)
    npix = rays.shape[0]
    lt, cdf, ipdf, Wt, tip = scene.light_table(tris, mats)
    P = npix * n
    pix = np.repeat(np.arange(npix, dtype=np.uint32), n)
    smp = np.tile(np.arange(s0, s0 + n, dtype=np.uint32), npix)
    o, d = rays[pix, :3].copy(), rays[pix, 3:].copy()
    src = np.full(P, -1, np.int32)
    alive = np.ones(P, bool)
    hidx = np.full((5, P), -1, np.int64)
    hct = np.zeros((5, P), F)
    hspec = np.zeros((5, P), bool)
    E = np.zeros((5, P, 3), F)
    prev_spec = np.zeros(P, bool)
    spec_then_hit = np.zeros(P, bool)
    emit_after_spec = np.zeros(P, bool)
    scans = 0
    for depth in range(5):
        a = np.flatnonzero(alive)
        if a.size == 0:
            break
        scans += a.size
        idx, dist = O.closest_hits(np.concatenate([o[a], d[a]], 1), tris, src[a])
        hit = idx >= 0
        alive[a[~hit]] = False
        a, idx, dist = a[hit], idx[hit].astype(np.int64), dist[hit]
        ps = prev_spec[a]
        spec_then_hit[a[ps]] = True
        emit_after_spec[a[ps & (mats[idx, 3:6].astype(np.float64).sum(1) > 0)]] = True
        nrm = tris[idx, 9:12].copy()
        flip = _dot(nrm, d[a]) > F(0)
        nrm[flip] = nrm[flip] * F(-1)
        x = o[a] + d[a] * dist[:, None]
        # the lobe: specular iff r7 < (double)p
        p = spec[idx, 3]
        r7, _ = _philox(seed, pix[a], smp[a], 32 + depth)
        sl = r7 < p.astype(np.float64)
        with np.errstate(divide="ignore"):
            wD = F(1) / (F(1) - p)
        De = mats[idx, 3:6].copy()
        if mis:
            # Ew_d: in full at the camera's hit and after a mirror bounce, else weighted where the triangle is in the light table
            ip = tip[idx]
            w = np.flatnonzero((ip > F(0)) & ~ps) if depth > 0 else np.zeros(0, np.int64)
            if w.size:
                db = d[a[w]]
                cyb = np.abs(_dot(db, tris[idx[w], 9:12]))
                sxzb = np.sqrt(db[:, 0] * db[:, 0] + db[:, 2] * db[:, 2])
                opu = F(1) + _u(sxzb, dist[w] * dist[w], cyb, ip[w])
                De[w] = De[w] / opu[:, None]
            L = np.zeros((a.size, 3), F)
            if depth < 4 and lt.size:
                r3, r4 = _philox(seed, pix[a], smp[a], 8 + depth)
                r5, _ = _philox(seed, pix[a], smp[a], 16 + depth)
                e = np.minimum(np.searchsorted(cdf, r5 * Wt, side="right"), lt.size - 1)
                li = lt[e]
                v0 = tris[li, 0:3]
                e1, e2 = tris[li, 3:6] - v0, tris[li, 6:9] - v0
                ua, ub = np.sqrt(r3).astype(F), r4.astype(F)
                y = (v0 + e1 * (ua * (F(1) - ub))[:, None]) + e2 * (ua * ub)[:, None]
                wv = y - x
                dist2 = _dot(wv, wv)
                ok = (li != idx) & (dist2 > F(0)) & ~sl              # a specular hit draws no light sample
                with np.errstate(divide="ignore", invalid="ignore"):
                    dd = np.sqrt(dist2)
                    wd = wv / dd[:, None]
                    cx = _dot(wd, nrm)
                    cy = np.abs(_dot(wd, tris[li, 9:12]))
                    sxz = np.sqrt(wd[:, 0] * wd[:, 0] + wd[:, 2] * wd[:, 2])
                    ok &= (cx > F(0)) & (cy > F(0))
                    tmax = dd * MARGIN
                    g = (TWO_PI * cx) / (F(1) + _u(sxz, dist2, cy, ipdf[e]))
                    Lc = (mats[idx, 0:3] * INV_PI) * (mats[li, 3:6] * g[:, None])
                k = np.flatnonzero(ok)
                scans += k.size
                if k.size:
                    sidx, sd = O.closest_hits(np.concatenate([x[k], wd[k]], 1), tris, idx[k].astype(np.int32))
                    vis = ~((sidx >= 0) & (sd < tmax[k]))
                    kv = k[vis]
                    L[kv] = Lc[kv] * wD[kv][:, None]                 # L_d wD
            E[depth, a] = De + L if depth < 4 else De
        else:
            E[depth, a] = De
        # the bounce: the mirror direction dir - n * (c + c), or the diffuse direction as always
        c = _dot(d[a], nrm)
        t = c + c
        nd = (d[a] - nrm * t[:, None]).astype(F)
        ct = np.zeros(a.size, F)
        df = np.flatnonzero(~sl)
        if df.size:
            r1, r2 = _philox(seed, pix[a[df]], smp[a[df]], depth)
            ndd = _unit_vec(nrm[df], r1, r2)
            nd[df] = ndd
            ct[df] = _dot(ndd, nrm[df])
        hct[depth, a] = ct
        hidx[depth, a] = idx
        hspec[depth, a] = sl
        prev_spec[a] = sl
        o[a], d[a], src[a] = x, nd, idx.astype(np.int32)
    rec = np.zeros((P, 3), F)
    for depth in range(4, -1, -1):
        h = np.flatnonzero(hidx[depth] >= 0)
        i = hidx[depth, h]
        p = spec[i, 3]
        brdf = mats[i, 0:3] * INV_PI
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            wS = (F(1) / p)[:, None]
            wD = (F(1) / (F(1) - p))[:, None]
            dif = E[depth, h] + (((brdf * rec[h]) * hct[depth, h][:, None]) * INV_P) * wD
            spe = E[depth, h] + (spec[i, 0:3] * rec[h]) * wS
        rec[h] = np.where(hspec[depth, h][:, None], spe, dif).astype(F)
    info = {"spec_then_hit": int(spec_then_hit.sum()), "emitter_after_spec": int(emit_after_spec.sum()), "samples": P}
    return rec.reshape(npix, n, 3), scans, info


def model_render(rays, tris, mats, spec, n, seed, mis):
    """-> (rgba [npix, 4] u8, mean [npix, 3] f32, scans, info) of a one-shot flagged render of n samples"""
    rec, scans, info = model_samples(rays, tris, mats, spec, seed, 0, n, mis)
    acc = np.zeros((rec.shape[0], 3), F)
    for s in range(n):
        acc = acc + rec[:, s]
    mean = acc * F(1.0 / n)
    c = np.clip(mean, F(0), F(1)) * F(255) + F(0.5)
    q = np.where(c < 0, 0, np.where(c > 255, 255, c.astype(np.uint32) & 0xFF)).astype(np.uint8)
    rgba = np.zeros((rec.shape[0], 4), np.uint8)
    rgba[:, :3] = q
    return rgba, mean, scans, info


# ---------------------------------------------------------------------------------------------------------------- scenes
def mirror_floor():
    """the default scene with its two floor triangles pure mirrors"""
    t, m = scene.default_scene()
    s = np.zeros((t.shape[0], 4), F)
    s[1:3] = (0.9, 0.8, 0.7, 1.0)
    return t, m, s


def mixed_room():
    """closed_room(200) with every triangle mixed: p in (0.2, 0.8) and ks by a fixed pattern over the index"""
    t, m = scene.closed_room(200)
    j = np.arange(t.shape[0], dtype=F)
    s = np.zeros((t.shape[0], 4), F)
    s[:, 0] = F(0.3) + F(0.1) * (j % 5)
    s[:, 1] = F(0.2) + F(0.15) * (j % 4)
    s[:, 2] = F(0.5) + F(0.05) * (j % 7)
    s[:, 3] = F(0.2) + F(0.1) * (j % 7)
    return t, m, s


def facing_mirrors():
    """two pure mirrors facing each other across the camera (z = 2 and z = -4), a diffuse floor and an emitting ceiling panel"""
    def quad(a, b, c, d):
        return [list(a) + list(b) + list(c), list(a) + list(c) + list(d)]
    v = (quad((-3, -1, 2), (3, -1, 2), (3, 2, 2), (-3, 2, 2)) + quad((-3, -1, -4), (3, -1, -4), (3, 2, -4), (-3, 2, -4)) +
         quad((-3, -1, -4), (3, -1, -4), (3, -1, 2), (-3, -1, 2)) + quad((-1.5, 1.9, -3), (1.5, 1.9, -3), (1.5, 1.9, 1), (-1.5, 1.9, 1)))
    t = np.zeros((8, 12), F)
    t[:, :9] = np.asarray(v, F)
    t = scene.flat_normals(t)
    m = np.zeros((8, 6), F)
    m[0:4, 0:3] = 0.1
    m[4:6, 0:3] = (0.7, 0.6, 0.5)
    m[6:8] = (0.2, 0.2, 0.2, 1.0, 0.9, 0.8)
    s = np.zeros((8, 4), F)
    s[0:4] = (0.9, 0.9, 0.95, 1.0)
    return t, m, s


SCENES = {"mirror_floor": mirror_floor, "mixed_room": mixed_room, "facing_mirrors": facing_mirrors}
REPLAY_SEED = 3


def _covered(info, mis):
    """a replay case proves something only if at least 10 % of its samples take a specular bounce and then hit something and, under
    MIS, at least one reaches an emitter directly after a specular bounce"""
    assert info["spec_then_hit"] >= 0.1 * info["samples"], info
    if mis:
        assert info["emitter_after_spec"] >= 1, info


# ---------------------------------------------------------------------------------------------------------------- CPU part
def test_flag_value_and_symbols():
    assert capi.FLAG_SPECULAR == 0x2000
    assert capi.FLAG_SPECULAR & (capi.FLAG_NEE | capi.FLAG_MIS | capi.FLAG_ACCEL | capi.FLAG_PRIMARY_REUSE | capi.FLAG_CAMERA_SAMPLES |
                                 0xFF | 0xFF0000) == 0
    assert {"sphip_set_specular", "sphip_set_specular_device"} <= set(capi.SYMBOLS)
    lib = C.CDLL(capi.LIB_PATH)
    assert hasattr(lib, "sphip_set_specular") and hasattr(lib, "sphip_set_specular_device")
    assert capi.load().sphip_abi_version() == 3
    hdr = open(os.path.join(ROOT, "include", "spath_hip.h")).read()
    assert "SPHIP_FLAG_SPECULAR = 0x2000" in hdr


def test_null_context_is_refused():
    """what sphip_set_specular checks without a device: a null context is SPHIP_E_INVALID for both forms"""
    L = capi.load()
    spec = np.zeros(4, F)
    assert L.sphip_set_specular(None, None) == -1
    assert L.sphip_set_specular(None, spec.ctypes.data) == -1
    assert L.sphip_set_specular_device(None, None, None) == -1


def _hand_scene():
    """a pure mirror in the plane y = 0, an emitter E in the plane x = 2 above it, and a black triangle in the plane x = -2.  The
    emitter and the black triangle reflect nothing (ks = 0) and are specular too (p = 1), so that every path is fixed by hand: what
    leaves them goes up and out, above the triangle opposite"""
    t = np.zeros((3, 12), F)
    t[0, :9] = [-10, 0, -10, 10, 0, -10, 0, 0, 20]
    t[1, :9] = [2, 0.5, -3, 2, 0.5, 3, 2, 5, 0]
    t[2, :9] = [-2, 0.5, -3, -2, 0.5, 3, -2, 4, 0]
    t = scene.flat_normals(t)
    m = np.zeros((3, 6), F)
    m[0, 0:3] = 0.5
    m[1, 3:6] = (2.0, 3.0, 0.75)
    s = np.zeros((3, 4), F)
    s[0] = (0.5, 0.25, 1.0, 1.0)
    s[1:3, 3] = 1.0
    a = F(np.sqrt(0.5))
    rays = np.array([[-1, 1, 0, a, -a, 0],        # reflects at the origin into (a, a, 0): reaches the emitter at (2, 2, 0)
                     [1, 1, 0, -a, -a, 0],        # reflects into (-a, a, 0): the black triangle at (-2, 2, 0), then out
                     [0, 1, 0, 0, -1, 0]], F)     # reflects straight up: nothing there
    return t, m, s, rays


@pytest.mark.parametrize("est", sorted(ESTIMATORS))
def test_model_by_hand(est):
    """a pure mirror ks = (0.5, 0.25, 1), p = 1 in front of one emitter E: exactly ks * E for the ray that reflects into it, 0 for the
    rays that reflect past it, under both estimators (no hit is diffuse, so no shadow ray is drawn), with the scans and the coverage
    counts that follow: per sample ray 0 scans mirror, emitter, miss; ray 1 mirror, black triangle, miss; ray 2 mirror, miss"""
    t, m, s, rays = _hand_scene()
    rec, scans, info = model_samples(rays, t, m, s, 7, 0, 3, bool(ESTIMATORS[est]))
    want = s[0, 0:3] * m[1, 3:6]
    assert list(want) == [F(1.0), F(0.75), F(0.75)]
    for k in range(3):
        assert np.array_equal(_bits(rec[0, k]), _bits(want)), rec[0, k]
    assert not rec[1:].any()
    # rays 0 and 1 hit something after the mirror, ray 2 does not; ray 0 alone reaches the emitter, straight from the mirror
    assert info == {"spec_then_hit": 6, "emitter_after_spec": 3, "samples": 9}
    assert scans == 3 * (3 + 3 + 2)


@pytest.mark.parametrize("name", ["closed_room_200", "open_clutter_100"])
def test_zero_table_is_the_old_models(name):
    """with a table of zeros the model is the plain estimator (the oracle's counter-RNG render) and the MIS replay
    (tests/test_hip_mis.py), bit for bit, scans included"""
    t, m = {"closed_room_200": lambda: scene.closed_room(200), "open_clutter_100": lambda: scene.open_clutter(100)}[name]()
    rays = _rays(16, 12)
    z = np.zeros((t.shape[0], 4), F)
    z[:, 0:3] = 0.4                                       # ks alone changes nothing
    img, mean, scans, info = model_render(rays, t, m, z, 3, 5, False)
    want_img, want_mean, want_scans = O.render_counter(rays, t, m, 3, 5)
    assert np.array_equal(_bits(mean), _bits(want_mean)) and np.array_equal(img, want_img) and scans == want_scans
    assert info["spec_then_hit"] == 0
    rec, scans, _ = model_samples(rays, t, m, z, 5, 1, 3, True)
    want, want_scans = mis_model_samples(rays, t, m, 5, 1, 3)
    assert np.array_equal(_bits(rec), _bits(want)) and scans == want_scans


@pytest.mark.parametrize("est", sorted(ESTIMATORS))
@pytest.mark.parametrize("name", sorted(SCENES))
def test_replay_cases_are_covered(name, est):
    t, m, s = SCENES[name]()
    *_, info = model_render(_rays(), t, m, s, SPP, REPLAY_SEED, bool(ESTIMATORS[est]))
    print(name, est, info)
    _covered(info, bool(ESTIMATORS[est]))


def test_specular_table_rule():
    t, m = scene.closed_room(50)
    ks = (0.6, 0.3, 0.1)
    s = scene.specular_table(t, m, ks)
    assert s.dtype == F and s.shape == (50, 4)
    k64 = np.asarray(ks, F).astype(np.float64)
    sk = (k64[0] + k64[1]) + k64[2]
    r64 = m[:, 0:3].astype(np.float64)
    r = (r64[:, 0] + r64[:, 1]) + r64[:, 2]
    assert np.array_equal(s[:, 0:3], np.broadcast_to(np.asarray(ks, F), (50, 3)))
    assert np.array_equal(_bits(s[:, 3]), _bits((sk / (sk + r)).astype(F)))
    assert ((s[:, 3] > 0) & (s[:, 3] <= 1)).all()
    # a subset, a given p, ks = 0, no diffuse reflectance
    s = scene.specular_table(t, m, 0.5, which=[3, 7], p=0.25)
    assert np.flatnonzero(s.any(1)).tolist() == [3, 7] and list(s[3]) == [F(0.5), F(0.5), F(0.5), F(0.25)]
    assert not scene.specular_table(t, m, 0.0).any()
    m0 = m.copy()
    m0[:, 0:3] = 0
    assert (scene.specular_table(t, m0, 0.5)[:, 3] == 1).all()
    for bad in (dict(ks=-0.1), dict(ks=np.nan), dict(ks=0.5, p=1.5), dict(ks=0.5, p=-0.1)):
        with pytest.raises(ValueError):
            scene.specular_table(t, m, **bad)


# ---------------------------------------------------------------------------------------------------------------- GPU part
@pytest.fixture(autouse=True, scope="module")
def _torch_first():
    """torch's device runtime is brought up before the library's first context, as conftest.py's hip fixture does"""
    import torch
    torch.cuda.is_available()


def _ctx(t, m, s=None):
    c = capi.Context(0)
    c.set_scene(t, m)
    if s is not None:
        c.set_specular(s)
    return c


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(_bits(a[1]), _bits(b[1]))


@pytest.mark.gpu
@pytest.mark.parametrize("est", sorted(ESTIMATORS))
@pytest.mark.parametrize("variant", [1, 2, 15, 16])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_model_bit_exact(name, variant, est):
    t, m, s = SCENES[name]()
    rays = _rays()
    mis = bool(ESTIMATORS[est])
    want_img, want_mean, want_scans, info = model_render(rays, t, m, s, SPP, REPLAY_SEED, mis)
    _covered(info, mis)
    c = _ctx(t, m, s)
    img, mean = c.render(rays, W, H, SPP, seed=REPLAY_SEED, flags=SPEC | ESTIMATORS[est] | variant, want_accum=True)
    st = c.stats()
    c.close()
    assert st["kernel_variant"] == variant
    assert np.array_equal(_bits(mean), _bits(want_mean))
    assert np.array_equal(img, want_img)
    assert st["scans_executed"] == want_scans


@pytest.fixture(params=[256, 512])
def shape(request):
    """both workgroup shapes of the default scan forced in turn (tests/test_hip_shapes.py): the library reads the override when it
    builds the scan's stream, on the first render after a set_scene"""
    old = os.environ.get("SPATH_HIP_CYLM_SHAPE")
    os.environ["SPATH_HIP_CYLM_SHAPE"] = str(request.param)
    yield request.param
    if old is None:
        del os.environ["SPATH_HIP_CYLM_SHAPE"]
    else:
        os.environ["SPATH_HIP_CYLM_SHAPE"] = old


@pytest.mark.gpu
@pytest.mark.parametrize("est", sorted(ESTIMATORS))
@pytest.mark.parametrize("name", ["mixed_room", "facing_mirrors"])
def test_both_block_shapes(shape, name, est):
    """variant 16 in its 256- and its 512-thread shape: the replay with a non-zero table, zero table = no flag, a progressive split,
    primary-hit reuse and camera samples against the other paths; the tile size of the stream says which shape ran"""
    from test_hip_shapes import _tiles
    t, m, s = SCENES[name]()
    rays = _rays()
    mis = bool(ESTIMATORS[est])
    f = ESTIMATORS[est] | 16
    want_img, want_mean, want_scans, info = model_render(rays, t, m, s, SPP, REPLAY_SEED, mis)
    _covered(info, mis)
    c = _ctx(t, m, s)
    got = c.render(rays, W, H, SPP, seed=REPLAY_SEED, flags=f | SPEC, want_accum=True)
    st = c.stats()
    assert _tiles(c, rays)[1] == shape and st["kernel_variant"] == 16
    assert np.array_equal(_bits(got[1]), _bits(want_mean)) and np.array_equal(got[0], want_img)
    assert st["scans_executed"] == want_scans
    assert _same(c.render(rays, W, H, SPP, seed=REPLAY_SEED, flags=f | SPEC | capi.FLAG_PRIMARY_REUSE, want_accum=True), got)
    c.accum_begin(rays=rays, w=W, h=H, seed=REPLAY_SEED, flags=f | SPEC)
    c.accum_step(1)
    img, mean, _ = c.accum_step(SPP - 1, want_mean=True)
    assert _same((img, mean), got)
    c.accum_begin(rays=rays, w=W, h=H, seed=REPLAY_SEED, flags=f | SPEC, adaptive=(0.0, 0.0, 0xFFFFFFFF))   # never stops a pixel
    c.accum_step(1)
    img, mean, _ = c.accum_step(SPP - 1, want_mean=True)
    assert _same((img, mean), got)
    cam = view.Camera(40, 26)
    cam.set_delta_mov([0.1, 0.2, 0.3])
    ca = c.render_camera(cam, SPP, seed=6, flags=f | SPEC | capi.FLAG_CAMERA_SAMPLES, want_accum=True)
    c.accum_begin(cam=cam, seed=6, flags=f | SPEC | capi.FLAG_CAMERA_SAMPLES)
    c.accum_step(2)
    img, mean, _ = c.accum_step(SPP - 2, want_mean=True)
    assert _same((img, mean), ca)
    z = s.copy()
    z[:, 3] = 0
    c.set_specular(z)
    for extra in (0, capi.FLAG_CAMERA_SAMPLES):
        want = c.render_camera(cam, SPP, seed=6, flags=f | extra, want_accum=True)
        ws = c.stats()["scans_executed"]
        flagged = c.render_camera(cam, SPP, seed=6, flags=f | extra | SPEC, want_accum=True)
        assert _same(flagged, want) and c.stats()["scans_executed"] == ws, extra
    assert _tiles(c, rays)[1] == shape
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("est", sorted(ESTIMATORS))
@pytest.mark.parametrize("variant", [1, 2, capi.FLAG_ACCEL, 15, 16])
def test_zero_table_is_no_flag(variant, est):
    """p = 0 everywhere (whatever ks): the flagged render is the unflagged one bit for bit, scans included, from rays and, with and
    without camera samples, from a camera"""
    t, m = scene.closed_room(200)
    rays = _rays()
    z = np.zeros((t.shape[0], 4), F)
    z[:, 0:3] = 0.7
    f = ESTIMATORS[est] | variant
    cam = view.Camera(40, 26)
    cam.set_delta_mov([0.1, 0.2, 0.3])
    c = _ctx(t, m, z)
    c.set_lens(0.05, 2.5)
    want = c.render(rays, W, H, SPP, seed=6, flags=f, want_accum=True)
    ws = c.stats()["scans_executed"]
    got = c.render(rays, W, H, SPP, seed=6, flags=f | SPEC, want_accum=True)
    gs = c.stats()["scans_executed"]
    assert _same(got, want) and gs == ws
    for extra in (0, capi.FLAG_CAMERA_SAMPLES):
        want = c.render_camera(cam, SPP, seed=6, flags=f | extra, want_accum=True)
        ws = c.stats()["scans_executed"]
        got = c.render_camera(cam, SPP, seed=6, flags=f | extra | SPEC, want_accum=True)
        assert _same(got, want) and c.stats()["scans_executed"] == ws, extra
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("est", sorted(ESTIMATORS))
def test_accel_geometric_parity(est):
    """the BVH gives the same image up to its rare rounding-noise accepts (tests/test_hip_mis.py::test_accel_geometric_parity's rule)"""
    t, m, s = mixed_room()
    rays = _rays()
    c = _ctx(t, m, s)
    a = c.render(rays, W, H, SPP, seed=3, flags=SPEC | ESTIMATORS[est] | 16, want_accum=True)[1]
    b = c.render(rays, W, H, SPP, seed=3, flags=SPEC | ESTIMATORS[est] | capi.FLAG_ACCEL, want_accum=True)[1]
    assert c.stats()["kernel_variant"] == 8
    plain = c.render(rays, W, H, SPP, seed=3, flags=ESTIMATORS[est] | capi.FLAG_ACCEL, want_accum=True)[1]
    c.close()
    same = np.all(_bits(a) == _bits(b), axis=1)
    assert same.mean() >= 0.99, same.mean()
    assert not np.array_equal(_bits(b), _bits(plain))


@pytest.mark.gpu
@pytest.mark.parametrize("est", sorted(ESTIMATORS))
@pytest.mark.parametrize("variant", [16, 15, 2])
def test_progressive_adaptive_denoise(variant, est):
    t, m, s = mixed_room()
    rays = _rays()
    f = SPEC | ESTIMATORS[est] | variant
    c = _ctx(t, m, s)
    one = {n: c.render(rays, W, H, n, seed=9, flags=f, want_accum=True) for n in (3, 8, 16)}
    c.accum_begin(rays=rays, w=W, h=H, seed=9, flags=f)
    tot = 0
    for n in (3, 5, 8):
        img, mean, tot = c.accum_step(n, want_mean=True)
        assert np.array_equal(img, one[tot][0]) and np.array_equal(_bits(mean), _bits(one[tot][1])), tot
    c.accum_begin(rays=rays, w=W, h=H, seed=9, flags=f, adaptive=(0.3, 0.05, 4))
    for n in (4, 4, 8):
        img, mean, _ = c.accum_step(n, want_mean=True)
    counts, _ = c.accum_counts()
    cnt = counts.ravel()
    for n in np.unique(cnt):
        want = one.get(int(n)) or c.render(rays, W, H, int(n), seed=9, flags=f, want_accum=True)
        sel = cnt == n
        assert np.array_equal(img[sel], want[0][sel]) and np.array_equal(_bits(mean[sel]), _bits(want[1][sel])), n
    den0 = c.accum_denoise()
    den1 = c.accum_denoise()
    assert den0.shape == (W * H, 4) and np.array_equal(den0, den1)
    g1 = c.accum_gbuffer()
    c.accum_begin(rays=rays, w=W, h=H, seed=9, flags=f & ~SPEC, adaptive=(0.3, 0.05, 4))
    c.accum_step(4)
    assert c.accum_gbuffer().tobytes() == g1.tobytes()      # the G-buffer is unchanged
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("est", sorted(ESTIMATORS))
def test_reuse_chunks_multi_device(est):
    t, m, s = mixed_room()
    rays = _rays()
    f = SPEC | ESTIMATORS[est]
    c = _ctx(t, m, s)
    want = c.render(rays, W, H, SPP, seed=4, flags=f, want_accum=True)
    unflagged = c.render(rays, W, H, SPP, seed=4, flags=ESTIMATORS[est], want_accum=True)
    assert not _same(want, unflagged)
    for extra in (capi.FLAG_PRIMARY_REUSE, capi.flag_chunks(1), capi.flag_chunks(4), 15 | capi.FLAG_PRIMARY_REUSE, 2 | capi.FLAG_PRIMARY_REUSE):
        got = c.render(rays, W, H, SPP, seed=4, flags=f | extra, want_accum=True)
        assert _same(got, want), extra
    c.close()
    for devs in ([0, 0], [0, 0, 0]):
        mc = capi.Context.multi(devs)
        mc.set_scene(t, m)
        mc.set_specular(s)
        got = mc.render(rays, W, H, SPP, seed=4, flags=f, want_accum=True)
        mc.accum_begin(rays=rays, w=W, h=H, seed=4, flags=f)
        mc.accum_step(1)
        img, mean, _ = mc.accum_step(SPP - 1, want_mean=True)
        mc.close()
        assert _same(got, want), devs
        assert _same((img, mean), want), devs


@pytest.mark.gpu
@pytest.mark.parametrize("est", sorted(ESTIMATORS))
@pytest.mark.parametrize("variant", [1, 2, capi.FLAG_ACCEL, 15, 16])
def test_camera_samples_and_device_table(variant, est):
    """camera samples with the flag are the chain of one-sample accumulations over sphip_camera_rays_device's rays (as
    tests/test_hip_camera_samples.py composes them); the table comes from a device pointer here"""
    import torch
    t, m, s = mixed_room()
    cam = view.Camera(40, 26)
    cam.set_delta_mov([0.1, 0.2, 0.3])
    cam.set_delta_rot([0.05, -0.1, 0.0])
    f = SPEC | ESTIMATORS[est] | variant
    c = _ctx(t, m)
    st = torch.cuda.current_stream().cuda_stream
    d_spec = torch.from_numpy(s).to("cuda")
    c.set_specular_device(d_spec.data_ptr(), st)
    torch.cuda.synchronize()
    del d_spec                                            # the table was copied
    c.set_lens(0.06, 2.5)
    img, mean = c.render_camera(cam, 4, seed=11, flags=f | capi.FLAG_CAMERA_SAMPLES, want_accum=True)
    npix = cam.res_x * cam.res_y
    d_rays = torch.empty(npix * 6, dtype=torch.float32, device="cuda")
    d_sum = torch.zeros(npix * 3, dtype=torch.float32, device="cuda")
    d_out = torch.zeros(npix * 4, dtype=torch.uint8, device="cuda")
    d_mean = torch.zeros(npix * 3, dtype=torch.float32, device="cuda")
    for k in range(4):
        c.camera_rays_device(cam, k, d_rays.data_ptr(), seed=11, stream=st)
        c.render_device_accum(d_rays.data_ptr(), npix, k, 1, d_sum.data_ptr(), d_out.data_ptr(), seed=11, flags=f,
                              image_width=cam.res_x, d_out_mean=d_mean.data_ptr(), stream=st)
    torch.cuda.synchronize()
    c.close()
    assert np.array_equal(img, d_out.cpu().numpy().reshape(-1, 4))
    assert np.array_equal(_bits(mean), _bits(d_mean.cpu().numpy().reshape(-1, 3)))


def _seeds_means(c, rays, w, h, spp, flags, seeds):
    return np.stack([c.render(rays, w, h, spp, seed=s, flags=flags, want_accum=True)[1].astype(np.float64) for s in seeds])


def _z_grid(a, b, h, w, tag):
    """the project's criterion (tests/test_hip_mis.py::test_unbiased): over 16 seeds, |z| < 4 for the difference of the image means
    and < 5 in every cell of a 4 x 4 grid"""
    dd = a.reshape(16, h, w, 3).sum(-1) - b.reshape(16, h, w, 3).sum(-1)

    def z(x):
        v = x.reshape(16, -1).mean(1)
        if not v.any():                                   # a cell both estimators render alike in every seed (nothing in view): no difference
            return 0.0
        return v.mean() / (v.std(ddof=1) / 4.0)
    print(f"{tag}: z(image) {z(dd):+.2f}")
    zs = [[z(dd[:, 8 * by:8 * by + 8, 8 * bx:8 * bx + 8]) for bx in range(4)] for by in range(4)]
    for row in zs:
        print("  " + " ".join(f"{v:+6.2f}" for v in row))
    assert abs(z(dd)) < 4, z(dd)
    for by in range(4):
        for bx in range(4):
            assert abs(zs[by][bx]) < 5, (by, bx, zs[by][bx])


@pytest.mark.gpu
@pytest.mark.parametrize("est", sorted(ESTIMATORS))
def test_unbiased_in_p(est):
    """the same (rho, ks) rendered with p = 0.3 and with p = 0.7 everywhere: the difference of the means is noise; 16 seeds x 256
    spp at 32 x 32, the sample count of the MIS test"""
    t, m, s = mixed_room()
    w = h = 32
    rays = _rays(w, h)
    seeds = list(range(100, 116))
    res = []
    for p in (0.3, 0.7):
        sp = s.copy()
        sp[:, 3] = F(p)
        c = _ctx(t, m, sp)
        res.append(_seeds_means(c, rays, w, h, 256, SPEC | ESTIMATORS[est], seeds))
        c.close()
    _z_grid(res[0], res[1], h, w, f"p 0.3 vs 0.7, {est}")


@pytest.mark.gpu
@pytest.mark.parametrize("seed0", [100, 300])
@pytest.mark.parametrize("name", ["mirror_floor", "mixed_room"])
def test_unbiased_plain_vs_mis(name, seed0):
    """plain and NEE|MIS estimate the same image on a mirror scene (same criterion, same sample count), for two disjoint sets of 16
    seeds"""
    t, m, s = SCENES[name]()
    w = h = 32
    rays = _rays(w, h)
    seeds = list(range(seed0, seed0 + 16))
    c = _ctx(t, m, s)
    a = _seeds_means(c, rays, w, h, 256, SPEC | NEE_MIS, seeds)
    b = _seeds_means(c, rays, w, h, 256, SPEC, seeds)
    c.close()
    _z_grid(a, b, h, w, f"{name}: MIS vs plain, seeds {seed0}..{seed0 + 15}")


@pytest.mark.gpu
def test_error_contract():
    t, m, s = mixed_room()
    rays = _rays()
    c = _ctx(t, m)
    L = capi.load()

    def refused(code, fn):
        with pytest.raises(RuntimeError, match=code):
            fn()
        assert L.sphip_last_error(c._h), "sphip_last_error is set"
        c.render(rays, W, H, 1, seed=1)                    # the context stays usable

    refused(E_STATE, lambda: c.render(rays, W, H, 2, seed=1, flags=SPEC))                      # flag without table
    refused(E_STATE, lambda: c.accum_begin(rays=rays, w=W, h=H, seed=1, flags=SPEC))
    c.set_specular(s)
    good = c.render(rays, W, H, 2, seed=1, flags=SPEC, want_accum=True)
    refused(E_INVALID, lambda: c.render(rays, W, H, 1, seed=1, mode=capi.MODE_FLAT, flags=SPEC))   # flag with FLAT
    refused(E_INVALID, lambda: c.render(rays, W, H, 2, seed=1, flags=SPEC | capi.FLAG_NEE))        # flag with NEE alone
    refused(E_INVALID, lambda: c.accum_begin(rays=rays, w=W, h=H, seed=1, flags=SPEC | capi.FLAG_NEE))
    refused(E_INVALID, lambda: c.render(rays, W, H, 2, seed=1, flags=SPEC | 9))                    # an unshipped variant
    refused(E_INVALID, lambda: c.accum_begin(rays=rays, w=W, h=H, seed=1, flags=SPEC | 9))
    for col, bad in ((0, -0.5), (1, np.nan), (2, np.inf), (3, 1.5), (3, -0.25), (3, np.nan)):       # bad table values
        sb = s.copy()
        sb[40, col] = bad
        sb[90, col] = bad
        with pytest.raises(RuntimeError, match=E_INVALID) as e:
            c.set_specular(sb)
        assert "triangle 40 " in str(e.value), str(e.value)
        assert _same(c.render(rays, W, H, 2, seed=1, flags=SPEC, want_accum=True), good)           # the table stays as it was
    # without the flag the table is ignored
    c.set_specular(None)
    refused(E_STATE, lambda: c.render(rays, W, H, 2, seed=1, flags=SPEC))                      # NULL cleared it
    unflagged = c.render(rays, W, H, 2, seed=1, want_accum=True)
    c.set_specular(s)
    assert _same(c.render(rays, W, H, 2, seed=1, want_accum=True), unflagged)
    # set_scene clears the table
    c.set_scene(t, m)
    refused(E_STATE, lambda: c.render(rays, W, H, 2, seed=1, flags=SPEC))
    # set_specular ends an accumulation, in the same way and with the same code as set_scene does
    c.set_specular(s)
    c.accum_begin(rays=rays, w=W, h=H, seed=1, flags=SPEC)
    c.accum_step(2)
    c.set_scene(t, m)
    with pytest.raises(RuntimeError, match=E_STATE) as by_scene:
        c.accum_step(2)
    c.set_specular(s)
    c.accum_begin(rays=rays, w=W, h=H, seed=1, flags=SPEC)
    c.accum_step(2)
    c.set_specular(s)
    with pytest.raises(RuntimeError, match=E_STATE) as by_spec:
        c.accum_step(2)
    assert str(by_spec.value) == str(by_scene.value)
    assert _same(c.render(rays, W, H, 2, seed=1, flags=SPEC, want_accum=True), good)
    c.close()
    # table before scene
    c = capi.Context(0)
    with pytest.raises(RuntimeError, match=E_STATE):
        c.set_specular(s)
    with pytest.raises(RuntimeError, match=E_STATE):
        c.set_specular_device(0)
    assert L.sphip_last_error(c._h)
    c.set_scene(t, m)
    c.set_specular(s)
    assert _same(c.render(rays, W, H, 2, seed=1, flags=SPEC, want_accum=True), good)
    c.close()
    # the device-pointer form on a multi-device context
    mc = capi.Context.multi([0, 0])
    mc.set_scene(t, m)
    with pytest.raises(RuntimeError, match=E_STATE):
        mc.set_specular_device(0)
    assert L.sphip_last_error(mc._h)
    with pytest.raises(RuntimeError, match=E_STATE):
        mc.render(rays, W, H, 2, seed=1, flags=SPEC)
    mc.set_specular(s)
    assert _same(mc.render(rays, W, H, 2, seed=1, flags=SPEC, want_accum=True), good)
    mc.accum_begin(rays=rays, w=W, h=H, seed=1, flags=SPEC)
    mc.accum_step(1)
    mc.set_specular(s)                                   # ends the accumulation of a multi-device context too
    with pytest.raises(RuntimeError, match=E_STATE):
        mc.accum_step(1)
    mc.accum_begin(rays=rays, w=W, h=H, seed=1, flags=SPEC)
    img, mean, _ = mc.accum_step(2, want_mean=True)
    assert _same((img, mean), good)
    mc.close()


@pytest.mark.gpu
def test_cli_and_adapter(tmp_path):
    """spath_cli --spec FILE goes through hip_renderer::set_specular and gives the capi image, one-shot, progressive, with --mis and
    on the camera path; the flat pass is unchanged; a table of the wrong size, a missing file and --nee alone are refused; the
    Python renderer mirrors the adapter"""
    import subprocess
    cli = os.path.join(ROOT, "spath_amd", "host", "build", "spath_cli")
    t, m, s = mixed_room()
    sp, ss = str(tmp_path / "s.bin"), str(tmp_path / "s.spec")
    scene.write_scene(sp, t, m)
    scene.write_specular(ss, s)
    w, h = 40, 24
    cam = view.Camera(w, h)
    rays = np.ascontiguousarray(cam.get_viewport(), dtype=F)
    c = _ctx(t, m, s)
    spec = c.render(rays, w, h, 8, seed=9, flags=SPEC)
    spec_mis = c.render(rays, w, h, 8, seed=9, flags=SPEC | NEE_MIS)
    spec_aa = c.render_camera(cam, 8, seed=9, flags=SPEC | capi.FLAG_CAMERA_SAMPLES)
    plain = c.render(rays, w, h, 8, seed=9)
    flat = c.render(rays, w, h, 1, mode=capi.MODE_FLAT)
    c.close()
    assert len({spec.tobytes(), spec_mis.tobytes(), spec_aa.tobytes(), plain.tobytes()}) == 4
    base = [cli, "--scene", sp, "--w", str(w), "--h", str(h), "--spp", "8", "--seed", "9"]
    for extra, want in ((["--spec", ss], spec), (["--spec", ss, "--progressive", "3"], spec), (["--spec", ss, "--mis"], spec_mis),
                        (["--spec", ss, "--aa"], spec_aa), (["--spec", ss, "--mode", "flat"], flat), ([], plain)):
        out = str(tmp_path / "o.rgba")
        subprocess.run(base + ["--out", out] + extra, check=True, capture_output=True, timeout=120)
        assert open(out, "rb").read() == want.tobytes(), extra
    scene.write_specular(str(tmp_path / "short.spec"), s[:50])
    for bad in (["--spec", str(tmp_path / "short.spec")], ["--spec", str(tmp_path / "none.spec")], ["--spec", ss, "--nee"]):
        r = subprocess.run(base + ["--out", str(tmp_path / "x.rgba")] + bad, capture_output=True, timeout=120)
        assert r.returncode != 0, bad
    from spath_amd import renderer
    r = renderer.HipRenderer(w, h, seed=9)                # the table turns the flag on, as in the adapter; the flat pass stays
    r.set_specular(s)
    out = renderer.Bitmap()
    r.render(renderer.Viewport(w, h, rays), t, m, t.shape[0], 8, out)
    assert np.asarray(out.values).tobytes() == spec.tobytes()
    r.render_flat(renderer.Viewport(w, h, rays), t, m, t.shape[0], 1, out)
    assert np.asarray(out.values).tobytes() == flat.tobytes()
    r.set_specular(None)
    r.render(renderer.Viewport(w, h, rays), t, m, t.shape[0], 8, out)
    assert np.asarray(out.values).tobytes() == plain.tobytes()
    r.close()
