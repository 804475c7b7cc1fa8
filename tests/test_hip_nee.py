"""Next-event estimation (include/spath_hip.h: SPHIP_FLAG_NEE): a light sample and one shadow (any-hit)
ray at each of the first four hits of a path.

The estimator is stated operation by operation in the header, so it is replayed here in numpy: the closest hits of path and
shadow rays through the oracle's strict scan (O.closest_hits; a shadow ray is occluded iff the closest hit that skips its source
triangle lies below tmax), the draws and directions through the oracle's device math, every other step in f32 in the stated
order, the light table in float64 like the host builds it.  STATED TOLERANCE: 0 -- images, means and scan counts bit for bit.

CPU part: the flag's value and the numpy light table on a hand-made scene.
GPU part: the replay for every shipped scan variant and scene kind; unchanged paths; composition with progressive and adaptive
accumulation, primary-hit reuse, sample chunks and multi-device contexts; unbiasedness against the plain estimator and lower
noise; the error contract."""
import os

import numpy as np
import pytest

from oracle import oracle as O
from spath_amd import capi, scene, view

F = np.float32
W, H, SPP = 48, 32, 4
INV_PI = np.array([0x3EA2F983], np.uint32).view(F)[0]
INV_P = np.array([0x40C90FDB], np.uint32).view(F)[0]
MARGIN = F(1.0 - 2.0 ** -10)
TWO_OVER_PI = F(2.0 / np.pi)
E_INVALID = r"\[-1\]"


def many_emitters(n=100):
    """open_clutter(n) with every 5th clutter triangle emitting a colour of its own: many entries in the light table"""
    t, m = scene.open_clutter(n)
    m = m.copy()
    k = np.arange(7, n)[::5]
    j = np.arange(k.size, dtype=F)
    m[k, 3] = F(0.5) + F(0.1) * (j % 3)
    m[k, 4] = F(0.2) + F(0.05) * (j % 4)
    m[k, 5] = F(0.1) * (j % 2)
    return t, m


def small_light_room(n=200):
    """closed_room(n) with its ceiling panel shrunk to 0.5 x 0.5"""
    t, m = scene.closed_room(n)
    t = t.copy()
    for v in range(3):
        t[12:14, 3 * v] *= F(0.25 / 1.5)
        t[12:14, 3 * v + 2] *= F(0.25 / 1.5)
    return scene.flat_normals(t), m


SCENES = {"closed_room_200": lambda: scene.closed_room(200), "open_clutter_100": lambda: scene.open_clutter(100),
          "many_emitters": many_emitters}


def light_table(tris, mats):
    """the host's table in float64: (tri, cdf, ipdf, W)"""
    tris = np.asarray(tris, F).reshape(-1, 12)
    mats = np.asarray(mats, F).reshape(-1, 6)
    idx, cdf, es_l = [], [], []
    W_ = 0.0
    for i in range(tris.shape[0]):
        e = mats[i, 3:6].astype(np.float64)
        es = (e[0] + e[1]) + e[2]
        if not es > 0.0:
            continue
        v = tris[i, :9].astype(np.float64)
        e1, e2 = v[3:6] - v[0:3], v[6:9] - v[0:3]
        cx = e1[1] * e2[2] - e1[2] * e2[1]
        cy = e1[2] * e2[0] - e1[0] * e2[2]
        cz = e1[0] * e2[1] - e1[1] * e2[0]
        w = (0.5 * np.sqrt((cx * cx + cy * cy) + cz * cz)) * es
        if not (w > 0.0 and np.isfinite(w)):
            continue
        W_ = W_ + w
        idx.append(i), cdf.append(W_), es_l.append(es)
    ipdf = np.array([W_ / e for e in es_l], np.float64).astype(F)
    return np.array(idx, np.int64), np.array(cdf, np.float64), ipdf, W_


def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def _philox(seed, pix, smp, depth):
    n = pix.size
    q = np.zeros((n, 5), np.uint32)
    q[:, 0], q[:, 1] = seed & 0xFFFFFFFF, seed >> 32
    q[:, 2], q[:, 3], q[:, 4] = pix, smp, depth
    r = O.device_math(2, q, n).reshape(n, 2)
    return r[:, 0], r[:, 1]


def _unit_vec(n, r1, r2):
    q = np.zeros((n.shape[0], 5), np.float64)
    q[:, :3], q[:, 3], q[:, 4] = n, r1, r2
    return O.device_math(3, q, n.shape[0]).reshape(-1, 3)


def model_samples(rays, tris, mats, seed, s0, n):
    """radiance [npix, n, 3] of global samples s0 .. s0 + n - 1 under NEE, and the scans (path + shadow) they take"""
    tris = np.ascontiguousarray(tris, F).reshape(-1, 12)
    mats = np.ascontiguousarray(mats, F).reshape(-1, 6)
    rays = np.ascontiguousarray(rays, F).reshape(-1, 6)
    npix = rays.shape[0]
    lt, cdf, ipdf, Wt = light_table(tris, mats)
    P = npix * n
    pix = np.repeat(np.arange(npix, dtype=np.uint32), n)
    smp = np.tile(np.arange(s0, s0 + n, dtype=np.uint32), npix)
    o, d = rays[pix, :3].copy(), rays[pix, 3:].copy()
    src = np.full(P, -1, np.int32)
    alive = np.ones(P, bool)
    hidx = np.full((4, P), -1, np.int64)
    hct = np.zeros((4, P), F)
    L = np.zeros((4, P, 3), F)
    scans = 0
    for depth in range(4):
        a = np.flatnonzero(alive)
        if a.size == 0:
            break
        scans += a.size
        idx, dist = O.closest_hits(np.concatenate([o[a], d[a]], 1), tris, src[a])
        hit = idx >= 0
        alive[a[~hit]] = False
        a, idx, dist = a[hit], idx[hit].astype(np.int64), dist[hit]
        nrm = tris[idx, 9:12].copy()
        flip = _dot(nrm, d[a]) > F(0)
        nrm[flip] = nrm[flip] * F(-1)
        x = o[a] + d[a] * dist[:, None]
        if lt.size:
            r3, r4 = _philox(seed, pix[a], smp[a], 8 + depth)
            r5, _ = _philox(seed, pix[a], smp[a], 16 + depth)
            e = np.minimum(np.searchsorted(cdf, r5 * Wt, side="right"), lt.size - 1)
            li = lt[e]
            v0 = tris[li, 0:3]
            e1, e2 = tris[li, 3:6] - v0, tris[li, 6:9] - v0
            ua, ub = np.sqrt(r3).astype(F), r4.astype(F)
            y = (v0 + e1 * (ua * (F(1) - ub))[:, None]) + e2 * (ua * ub)[:, None]
            w = y - x
            dist2 = _dot(w, w)
            ok = (li != idx) & (dist2 > F(0))
            with np.errstate(divide="ignore", invalid="ignore"):
                dd = np.sqrt(dist2)
                wd = w / dd[:, None]
                cx = _dot(wd, nrm)
                cy = np.abs(_dot(wd, tris[li, 9:12]))
                sxz = np.sqrt(wd[:, 0] * wd[:, 0] + wd[:, 2] * wd[:, 2])
                ok &= (cx > F(0)) & (cy > F(0)) & (sxz > F(0))
                tmax = dd * MARGIN
                g = (((cx * cy) / dist2) * ipdf[e]) * (TWO_OVER_PI / sxz)
                Lc = (mats[idx, 0:3] * INV_PI) * (mats[li, 3:6] * g[:, None])
            k = np.flatnonzero(ok)
            scans += k.size
            if k.size:
                sidx, sd = O.closest_hits(np.concatenate([x[k], wd[k]], 1), tris, idx[k].astype(np.int32))
                vis = ~((sidx >= 0) & (sd < tmax[k]))
                L[depth, a[k[vis]]] = Lc[k[vis]]
        r1, r2 = _philox(seed, pix[a], smp[a], depth)
        nd = _unit_vec(nrm, r1, r2)
        hct[depth, a] = _dot(nd, nrm)
        hidx[depth, a] = idx
        o[a], d[a], src[a] = x, nd, idx.astype(np.int32)
    rec = np.zeros((P, 3), F)
    for depth in range(3, -1, -1):
        h = np.flatnonzero(hidx[depth] >= 0)
        m = mats[hidx[depth, h]]
        brdf = m[:, 0:3] * INV_PI
        e = m[:, 3:6] if depth == 0 else np.zeros((h.size, 3), F)
        e = e + L[depth, h]
        rec[h] = e + ((brdf * rec[h]) * hct[depth, h][:, None]) * INV_P
    return rec.reshape(npix, n, 3), scans


def model_render(rays, tris, mats, n, seed):
    """-> (rgba [npix, 4] u8, mean [npix, 3] f32, scans) of a one-shot NEE render of n samples"""
    rec, scans = model_samples(rays, tris, mats, seed, 0, n)
    acc = np.zeros((rec.shape[0], 3), F)
    for s in range(n):
        acc = acc + rec[:, s]
    mean = acc * F(1.0 / n)
    c = np.clip(mean, F(0), F(1)) * F(255) + F(0.5)
    q = np.where(c < 0, 0, np.where(c > 255, 255, c.astype(np.uint32) & 0xFF)).astype(np.uint8)
    rgba = np.zeros((rec.shape[0], 4), np.uint8)
    rgba[:, :3] = q
    return rgba, mean, scans


def _rays(w=W, h=H):
    cam = view.Camera(w, h)
    cam.set_delta_mov((0.1, -0.2, 0.3))
    cam.set_delta_rot((0.05, 0.1, 0.0))
    return np.ascontiguousarray(cam.get_viewport(), dtype=F)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------- CPU part
def test_flag_value():
    assert capi.FLAG_NEE == 0x400
    assert capi.FLAG_NEE & (capi.FLAG_ACCEL | capi.FLAG_PRIMARY_REUSE | 0xFF | 0xFF0000) == 0


def test_light_table_by_hand():
    """two emitters of areas 0.5 and 2 and emittance sums 3 and 1: weights 1.5 and 2, ipdf = W / Esum"""
    t = np.zeros((3, 12), F)
    t[0, :9] = [0, 0, 0, 1, 0, 0, 0, 1, 0]
    t[1, :9] = [0, 0, 0, 2, 0, 0, 0, 2, 0]
    t[2, :9] = [0, 0, 0, 1, 0, 0, 0, 1, 0]
    m = np.zeros((3, 6), F)
    m[0, 3:6] = [1, 1, 1]
    m[2, 3:6] = [0, 0.5, 0.5]
    m[1, 3:6] = 0
    idx, cdf, ipdf, Wt = light_table(t, m)
    assert list(idx) == [0, 2]
    assert list(cdf) == [1.5, 2.0] and Wt == 2.0
    assert list(ipdf) == [F(2.0 / 3.0), F(2.0)]


# ---------------------------------------------------------------------------------------------------------------- GPU part
def _ctx(t, m):
    c = capi.Context(0)
    c.set_scene(t, m)
    return c


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [1, 2, 15, 16])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_model_bit_exact(name, variant):
    t, m = SCENES[name]()
    rays = _rays()
    want_img, want_mean, want_scans = model_render(rays, t, m, SPP, 3)
    c = _ctx(t, m)
    img, mean = c.render(rays, W, H, SPP, seed=3, flags=capi.FLAG_NEE | variant, want_accum=True)
    st = c.stats()
    c.close()
    assert st["kernel_variant"] == variant
    assert np.array_equal(_bits(mean), _bits(want_mean))
    assert np.array_equal(img, want_img)
    assert st["scans_executed"] == want_scans


@pytest.mark.gpu
def test_accel_geometric_parity():
    """the BVH gives the same image up to its rare rounding-noise accepts (test_hip_accel.py's rule: almost every pixel equal)"""
    t, m = scene.closed_room(200)
    rays = _rays()
    c = _ctx(t, m)
    a = c.render(rays, W, H, SPP, seed=3, flags=capi.FLAG_NEE | 16, want_accum=True)[1]
    b = c.render(rays, W, H, SPP, seed=3, flags=capi.FLAG_NEE | capi.FLAG_ACCEL, want_accum=True)[1]
    c.close()
    same = np.all(_bits(a) == _bits(b), axis=1)
    assert same.mean() >= 0.99, same.mean()


@pytest.mark.gpu
def test_paths_unchanged_and_isolated():
    t, m = scene.closed_room(200)
    rays = _rays()
    c = _ctx(t, m)
    plain0 = c.render(rays, W, H, SPP, seed=5, want_accum=True)[1]
    nee = c.render(rays, W, H, SPP, seed=5, flags=capi.FLAG_NEE, want_accum=True)[1]
    plain1 = c.render(rays, W, H, SPP, seed=5, want_accum=True)[1]
    nee1 = c.render(rays, W, H, SPP, seed=5, flags=capi.FLAG_NEE, want_accum=True)[1]
    flat0 = c.render(rays, W, H, 1, mode=capi.MODE_FLAT)
    flat1 = c.render(rays, W, H, 1, mode=capi.MODE_FLAT, flags=capi.FLAG_NEE)
    c.accum_begin(rays=rays, w=W, h=H, seed=5)
    c.accum_step(2)
    g0 = c.accum_gbuffer()
    c.accum_begin(rays=rays, w=W, h=H, seed=5, flags=capi.FLAG_NEE)
    c.accum_step(2)
    g1 = c.accum_gbuffer()
    c.close()
    assert np.array_equal(_bits(plain0), _bits(plain1)) and np.array_equal(_bits(nee), _bits(nee1))
    assert not np.array_equal(_bits(plain0), _bits(nee))
    assert np.array_equal(flat0, flat1)
    assert g0.tobytes() == g1.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [16, 15])
def test_progressive_and_adaptive(variant):
    t, m = many_emitters()
    rays = _rays()
    f = capi.FLAG_NEE | variant
    c = _ctx(t, m)
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
    assert len(np.unique(cnt)) > 1                   # some pixels stopped early
    den = c.accum_denoise()
    assert den.shape == (W * H, 4)
    c.close()


@pytest.mark.gpu
def test_reuse_chunks_multi_device():
    t, m = scene.open_clutter(100)
    rays = _rays()
    c = _ctx(t, m)
    want = c.render(rays, W, H, SPP, seed=4, flags=capi.FLAG_NEE, want_accum=True)
    for extra in (capi.FLAG_PRIMARY_REUSE, capi.flag_chunks(1), capi.flag_chunks(4)):
        got = c.render(rays, W, H, SPP, seed=4, flags=capi.FLAG_NEE | extra, want_accum=True)
        assert np.array_equal(got[0], want[0]) and np.array_equal(_bits(got[1]), _bits(want[1])), extra
    c.close()
    for devs in ([0, 0], [0, 0, 0]):
        mc = capi.Context.multi(devs)
        mc.set_scene(t, m)
        got = mc.render(rays, W, H, SPP, seed=4, flags=capi.FLAG_NEE, want_accum=True)
        mc.close()
        assert np.array_equal(got[0], want[0]) and np.array_equal(_bits(got[1]), _bits(want[1])), devs


def _seeds_means(c, rays, w, h, spp, flags, seeds):
    return np.stack([c.render(rays, w, h, spp, seed=s, flags=flags, want_accum=True)[1].astype(np.float64) for s in seeds])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["open_clutter_100", "small_light_room"])
def test_unbiased(name):
    """16 seeds x 256 spp of each estimator on the same paths: the difference of the means is noise (|z| < 4 for the image mean,
    < 5 in every cell of a 4 x 4 grid)"""
    t, m = scene.open_clutter(100) if name == "open_clutter_100" else small_light_room()
    w = h = 32
    rays = _rays(w, h)
    c = _ctx(t, m)
    seeds = list(range(100, 116))
    a = _seeds_means(c, rays, w, h, 256, capi.FLAG_NEE, seeds).reshape(16, h, w, 3).sum(-1)
    b = _seeds_means(c, rays, w, h, 256, 0, seeds).reshape(16, h, w, 3).sum(-1)
    c.close()
    dd = a - b

    def z(x):
        v = x.reshape(16, -1).mean(1)
        return v.mean() / (v.std(ddof=1) / 4.0)
    assert abs(z(dd)) < 4, z(dd)
    for by in range(4):
        for bx in range(4):
            zc = z(dd[:, 8 * by:8 * by + 8, 8 * bx:8 * bx + 8])
            assert abs(zc) < 5, (by, bx, zc)


@pytest.mark.gpu
def test_lower_noise():
    """small light, 16 spp: the RMS error against a 4096-spp plain reference is at most half the plain estimator's"""
    t, m = small_light_room()
    w = h = 32
    rays = _rays(w, h)
    c = _ctx(t, m)
    ref = c.render(rays, w, h, 4096, seed=77, want_accum=True)[1].astype(np.float64)
    plain = c.render(rays, w, h, 16, seed=1, want_accum=True)[1]
    nee = c.render(rays, w, h, 16, seed=1, flags=capi.FLAG_NEE, want_accum=True)[1]
    c.close()
    rp = np.sqrt(np.mean((plain - ref) ** 2))
    rn = np.sqrt(np.mean((nee - ref) ** 2))
    print(f"small-light room 16 spp: RMS plain {rp:.4f}, NEE {rn:.4f}, ratio {rn / rp:.3f}")
    assert rn <= 0.5 * rp, (rn, rp)


@pytest.mark.gpu
def test_error_contract():
    t, m = scene.closed_room(200)
    rays = _rays()
    for bad in (-0.5, np.nan, np.inf):
        mb = m.copy()
        mb[40, 4] = bad
        c = _ctx(t, mb)
        with pytest.raises(RuntimeError, match=E_INVALID):
            c.render(rays, W, H, 2, seed=1, flags=capi.FLAG_NEE)
        c.render(rays, W, H, 2, seed=1)                   # the plain estimator does not look at it
        c.close()
    # no emitter: black, as without the flag
    m0 = m.copy()
    m0[:, 3:6] = 0
    c = _ctx(t, m0)
    img = c.render(rays, W, H, 2, seed=1, flags=capi.FLAG_NEE)
    assert not img.any()
    # a variant of -DSP_ALL_VARIANTS builds only, or absent from this build
    with pytest.raises(RuntimeError, match=E_INVALID):
        c.render(rays, W, H, 2, seed=1, flags=capi.FLAG_NEE | 9)
    c.close()


@pytest.mark.gpu
def test_cli_and_adapter(tmp_path):
    """spath_cli --nee goes through hip_renderer::set_nee and gives the capi image, one-shot and progressive"""
    import subprocess
    cli = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "spath_amd", "host", "build", "spath_cli")
    t, m = scene.open_clutter(100)
    sp = str(tmp_path / "s.bin")
    scene.write_scene(sp, t, m)
    w, h = 40, 24
    rays = np.ascontiguousarray(view.Camera(w, h).get_viewport(), dtype=F)
    c = _ctx(t, m)
    want = c.render(rays, w, h, 8, seed=9, flags=capi.FLAG_NEE)
    c.close()
    for extra in ([], ["--progressive", "3"]):
        out = str(tmp_path / "o.rgba")
        subprocess.run([cli, "--scene", sp, "--w", str(w), "--h", str(h), "--spp", "8", "--seed", "9", "--nee", "--out", out] + extra,
                       check=True, capture_output=True, timeout=120)
        assert open(out, "rb").read() == want.tobytes(), extra
