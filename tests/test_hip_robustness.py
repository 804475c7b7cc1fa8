"""Inputs far outside the comfortable range: the conservative filter must degrade to 'keep' (never to a wrong
reject), so every scan kernel still agrees bit for bit with the oracle's strict evaluation."""
import numpy as np
import pytest
import torch

import bvh_checks as bc
import bvh_model
from spath_amd import capi, scene, view

pytestmark = pytest.mark.gpu
VARIANTS = [v for v in capi.available_variants() if v != 8]     # 1, 2, 15, 16


def _hits(hip, O, t, rays, tag):
    n = rays.shape[0]
    want_idx, want_d = O.closest_hits(rays, t)
    d_rays = torch.from_numpy(np.ascontiguousarray(rays)).cuda()
    d_idx = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_d = torch.zeros(n, dtype=torch.float32, device="cuda")
    for v in VARIANTS:
        hip.closest_hit_device(d_rays.data_ptr(), n, d_idx.data_ptr(), d_d.data_ptr(), flags=v)
        torch.cuda.synchronize()
        assert np.array_equal(d_idx.cpu().numpy(), want_idx), (tag, v)
        assert np.array_equal(d_d.cpu().numpy().view(np.uint32), want_d.view(np.uint32)), (tag, v)
    return want_idx


def _accel_leg(hip, O, t, rays, tag):
    """variant 8 (the opt-in BVH), which _hits leaves out by design: its walk is held to the oracle ray by ray, every difference
    explained as a rounding-noise accept (bvh_checks.check_walk), with no source triangle and with a random one"""
    nl = bvh_model.n_leaves_for(t.shape[0])
    rng = np.random.default_rng(rays.shape[0])
    for src in (None, rng.integers(-1, t.shape[0], rays.shape[0]).astype(np.int32)):
        with np.errstate(all="ignore"):
            bc.check_walk(O, t, rays, hip.selftest_bvh_walk(rays, src), nl, src=src, tag=f"accel {tag} src={'none' if src is None else 'random'}")


def _rays(rng, n, scale, center):
    o = rng.uniform(-1.4, 1.4, (n, 3)) * [1, 0.5, 1]
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([o * scale + center, d], axis=1).astype(np.float32)


@pytest.mark.parametrize("scale,shift", [(1.0, 0.0), (1e-4, 0.0), (1e4, 0.0), (1.0, 3e4), (1e-3, 5e2), (1e12, 0.0), (1e20, 0.0)])
def test_scaled_and_shifted_scenes(hip, O, scale, shift):
    """The same closed room scaled by 1e-4 .. 1e20 and pushed 3e4 units from the origin (large cancellation in the
    ray moment): at 1e20 the filter's products overflow to inf/NaN and every pair must fall through to the exact test."""
    t, m = scene.closed_room(700)
    t = t.copy()
    t[:, :9] = (t[:, :9].astype(np.float64) * scale + shift).astype(np.float32)
    hip.set_scene(t, m)
    rays = _rays(np.random.default_rng(4), 3000, scale, shift)
    idx = _hits(hip, O, t, rays, (scale, shift))
    _accel_leg(hip, O, t, rays, (scale, shift))
    if scale <= 1e4:                     # beyond ~1e11 the distances exceed MAX_VALUE_DIST = 1e12 and the reference itself reports misses
        assert (idx >= 0).mean() > 0.9


@pytest.mark.parametrize("scale,dir_len", [(1e18, 1e18), (1e19, 1e19), (3e18, 3e19), (1e10, 1e27), (1e-3, 3e38), (1e19, 1.0)])
def test_products_near_float_overflow(hip, O, scale, dir_len):
    """|pos| |dir| around 1e36 .. 1e39: stage-1 products reach the float range.  Below 1e37 nothing can overflow, from
    there on the filter switches itself off for the ray (Dq = inf); either way the hits must be the strict evaluation's."""
    t, m = scene.closed_room(400)
    t = t.copy()
    t[:, :9] = (t[:, :9].astype(np.float64) * scale).astype(np.float32)
    hip.set_scene(t, m)
    rays = _rays(np.random.default_rng(12), 3000, scale, 0.0)
    rays[:, 3:] = (rays[:, 3:].astype(np.float64) * dir_len * np.random.default_rng(13).uniform(0.1, 1.0, (3000, 1))).astype(np.float32)
    _hits(hip, O, t, rays, (scale, dir_len))
    _accel_leg(hip, O, t, rays, (scale, dir_len))


def test_nonfinite_and_degenerate_inputs(hip, O):
    t, m = scene.closed_room(300)
    t = t.copy()
    t[20, 0] = np.inf
    t[21, 4] = np.nan
    t[22, :9] = 0.0                      # a point
    t[23, 3:6] = t[23, 0:3]              # a segment
    hip.set_scene(t, m)
    rng = np.random.default_rng(9)
    rays = _rays(rng, 2000, 1.0, 0.0)
    rays[5, 3:] = 0.0                    # zero direction
    rays[6, 0] = np.nan
    rays[7, 4] = np.inf
    rays[8, 3:] *= 1e-30
    rays[9, 3:] *= 1e30
    _hits(hip, O, t, rays, "nonfinite")
    # and a full render of that scene still equals the oracle
    w, h = 48, 36
    vp = view.Camera(w, h).get_viewport()
    want = O.render_counter(vp, t, m, 3, 2)
    for v in VARIANTS:
        img, acc = hip.render(vp, w, h, 3, seed=2, flags=v, want_accum=True)
        assert np.array_equal(img, want[0]), v
        assert np.array_equal(acc, want[1], equal_nan=True), v


def test_many_samples_and_odd_counts(hip, O, scenes):
    """Sample-split lanes: odd sample counts, one sample, more samples than a byte."""
    t, m = scenes["default"]
    rays = view.Camera(23, 17).get_viewport()
    hip.set_scene(t, m)
    for spp in (1, 2, 3, 255, 257):
        want = O.render_counter(rays, t, m, spp, 11)
        for v in [v for v in VARIANTS if v >= 3]:          # incl. rpl_cylw4s: four consecutive samples of a pixel per lane
            img, acc = hip.render(rays, 23, 17, spp, seed=11, flags=v, want_accum=True)
            assert np.array_equal(img, want[0]) and np.array_equal(acc, want[1]), (spp, v)
            assert hip.stats()["scans_executed"] == want[2]


def test_fuzz_filter_scan_against_exact_scan(hip):
    """Bulk fuzz on the GPU alone: random triangle soups (sizes over five decades, slivers, clustered and
    spread) x random rays; the two-stage scans must return exactly what the exact LDS scan returns.
    About 2.4e9 ray-triangle pairs per kernel variant."""
    rng = np.random.default_rng(2026)
    for it in range(30):
        n = int(rng.integers(65, 3000))
        size = 10.0 ** rng.uniform(-3, 1.5)
        spread = 10.0 ** rng.uniform(-1, 2)
        ctr = rng.normal(size=(n, 1, 3)) * spread
        v = ctr + rng.normal(size=(n, 3, 3)) * size * (10.0 ** rng.uniform(-2, 0, size=(n, 1, 1)))
        if it % 3 == 0:                               # slivers: third vertex almost on the first edge
            v[:, 2] = v[:, 0] + (v[:, 1] - v[:, 0]) * rng.uniform(0, 1, (n, 1)) + rng.normal(size=(n, 3)) * size * 1e-4
        t = np.zeros((n, 12), dtype=np.float32)
        t[:, :9] = v.reshape(n, 9)
        t = scene.flat_normals(t)
        m = np.ones((n, 6), dtype=np.float32)
        hip.set_scene(t, m)
        nr = 40000
        o = rng.normal(size=(nr, 3)) * spread * 1.5
        # aim at random interior/edge/vertex points of random triangles, half of them jittered off the triangle
        bc = rng.dirichlet([0.5, 0.5, 0.5], nr)
        tri = v[rng.integers(0, n, nr)]
        tgt = (tri * bc[:, :, None]).sum(axis=1) + rng.normal(size=(nr, 3)) * size * 0.3 * (rng.random((nr, 1)) < 0.5)
        d = tgt - o
        d /= np.maximum(np.linalg.norm(d, axis=1, keepdims=True), 1e-30)
        rays = np.concatenate([o, d], axis=1).astype(np.float32)
        src = rng.integers(-1, n, nr).astype(np.int32)
        d_rays, d_src = torch.from_numpy(rays).cuda(), torch.from_numpy(src).cuda()
        res = {}
        two_stage = [v for v in VARIANTS if v >= 3]
        for var in [2] + two_stage:
            di = torch.zeros(nr, dtype=torch.int32, device="cuda"); dd = torch.zeros(nr, dtype=torch.float32, device="cuda")
            hip.closest_hit_device(d_rays.data_ptr(), nr, di.data_ptr(), dd.data_ptr(), d_src_idx=d_src.data_ptr(), flags=var)
            torch.cuda.synchronize()
            res[var] = (di.cpu().numpy(), dd.cpu().numpy().view(np.uint32))
        for var in two_stage:
            assert np.array_equal(res[var][0], res[2][0]) and np.array_equal(res[var][1], res[2][1]), (it, var, n, size, spread)
        assert (res[2][0] >= 0).mean() > 0.02, (it, n, size, spread)     # the rays do hit things


def test_sample_chunks_back_off_when_device_memory_is_short():
    """The sample split is an optimisation: with (almost) no free device memory the same render must still succeed,
    with fewer chunks or none, and give the same image."""
    import torch
    from spath_amd import view
    t, m = scene.closed_room(300)
    w, h, spp = 640, 360, 64
    rays = view.Camera(w, h).get_viewport()
    a = capi.Context(0)
    a.set_scene(t, m)
    want_img, want_acc = a.render(rays, w, h, spp, seed=3, want_accum=True)
    assert a.stats()["n_launches"] == 2
    del a
    b = capi.Context(0)
    b.set_scene(t, m)
    b.render(rays, w, h, 1, seed=3)                       # buffers of the unsplit launch are allocated now
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    hog = torch.empty(max(free - (600 << 20), 0), dtype=torch.uint8, device="cuda")      # leave ~600 MB: the full split wants ~950 MB
    try:
        img, acc = b.render(rays, w, h, spp, seed=3, want_accum=True)
        assert np.array_equal(img, want_img) and np.array_equal(acc, want_acc)
    finally:
        del hog
        torch.cuda.empty_cache()


def test_rays_in_the_plane_of_far_triangles_noise_accepts(hip, O):
    """The regime a conservative filter exists for: a ray that lies (to float rounding) in the PLANE of a triangle it passes at a
    distance.  There geom::ray_intersect's a and s.h are both rounding noise and it reports a hit in about 0.5 % of such rays
    (tools/accel_noise_rate.py: 186 556 of 3.4e7; a geometric bounding-volume cull misses every one of them) -- the two-stage scans
    must reproduce each of them: same index, same distance bits as the exact scan and the oracle."""
    t, m = scene.closed_room(3000)
    hip.set_scene(t, m)
    rng = np.random.default_rng(9)
    n = 1 << 20
    v = t[:, :9].reshape(-1, 3, 3).astype(np.float64)
    k = rng.integers(14, t.shape[0], n)
    e1, e2 = v[k, 1] - v[k, 0], v[k, 2] - v[k, 0]
    ab = rng.uniform(-60, 60, (n, 2))
    o = v[k, 0] + e1 * ab[:, :1] + e2 * ab[:, 1:]
    cd = rng.normal(size=(n, 2))
    d = e1 * cd[:, :1] + e2 * cd[:, 1:]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.concatenate([o, d], axis=1).astype(np.float32)
    d_rays = torch.from_numpy(rays).cuda()
    d_idx = torch.zeros(n, dtype=torch.int32, device="cuda"); d_d = torch.zeros(n, dtype=torch.float32, device="cuda")
    res = {}
    two_stage = [v for v in VARIANTS if v >= 3]          # includes the default (16: thinnest error budget of all the filters)
    assert 16 in two_stage
    for var in [2] + two_stage:
        hip.closest_hit_device(d_rays.data_ptr(), n, d_idx.data_ptr(), d_d.data_ptr(), flags=var)
        torch.cuda.synchronize()
        res[var] = (d_idx.cpu().numpy(), d_d.cpu().numpy().view(np.uint32))
    for var in two_stage:
        assert np.array_equal(res[var][0], res[2][0]) and np.array_equal(res[var][1], res[2][1]), var
    # the hits on the ray's own "plane" triangle are the noise accepts: the ray passes it at a distance by construction
    own = res[2][0] == k
    assert own.sum() > 500, own.sum()
    sub = np.flatnonzero(own)[:3000]
    oi, od = O.closest_hits(rays[sub], t)
    assert np.array_equal(oi, res[2][0][sub]) and np.array_equal(od.view(np.uint32), res[2][1][sub])


def test_aimed_rays_at_small_triangles_in_small_scenes():
    """Rays aimed at points of tiny triangles from metres away, unnormalised directions, a few triangles per scene: the regime in
    which a one-ulp error of a half operand of the matrix-pipe stage 1 (rpl_cylm) rejected true hits (found by tools/soak.py: the
    fragment value and its remainder had come from two float->half conversions that round a near-tie differently).  Every
    two-stage scan against the exact-only scan, (index, distance bits), with random idx_source."""
    rng = np.random.default_rng(20260105)
    hip = capi.Context(0)
    two_stage = [v for v in VARIANTS if v >= 3]
    nr = 20000
    for it in range(160):
        n = int(rng.integers(1, 40))
        scale = 10.0 ** rng.uniform(-2.5, 0.5, (n, 1)); ctr = rng.uniform(-2, 2, (n, 3)) * [1, 0.6, 1]
        t = np.zeros((n, 12), dtype=np.float32)
        for k in range(3): t[:, 3 * k:3 * k + 3] = ctr + rng.normal(size=(n, 3)) * scale
        t = scene.flat_normals(t); t[:, 9:12] = np.nan_to_num(t[:, 9:12])
        m = np.full((n, 6), 0.5, dtype=np.float32)
        hip.set_scene(t, m)
        hr = np.concatenate([rng.uniform(-3, 3, (nr, 3)), rng.normal(size=(nr, 3))], axis=1).astype(np.float32)
        v = t[:, :9].reshape(-1, 3, 3); k = rng.integers(0, n, nr * 3 // 4); bw = rng.dirichlet([0.3, 0.3, 0.3], nr * 3 // 4)
        hr[: nr * 3 // 4, 3:] = (v[k] * bw[:, :, None]).sum(1) - hr[: nr * 3 // 4, :3]
        src = rng.integers(-1, n, nr).astype(np.int32)
        d_r, d_s = torch.from_numpy(hr).cuda(), torch.from_numpy(src).cuda()
        oi = torch.zeros(nr, dtype=torch.int32, device="cuda"); od = torch.zeros(nr, dtype=torch.float32, device="cuda")
        res = {}
        for var in [2] + two_stage:
            hip.closest_hit_device(d_r.data_ptr(), nr, oi.data_ptr(), od.data_ptr(), d_src_idx=d_s.data_ptr(), flags=var); torch.cuda.synchronize()
            res[var] = (oi.cpu().numpy().copy(), od.cpu().numpy().view(np.uint32).copy())
        assert (res[2][0] >= 0).mean() > 0.3
        for var in two_stage:
            assert np.array_equal(res[var][0], res[2][0]) and np.array_equal(res[var][1], res[2][1]), (it, n, var)
    hip.close()


def test_extreme_scale_combinations_of_scene_and_direction(hip, O):
    """Scene size and direction length at opposite ends of their ranges (the matrix-pipe stage 1 scales both sides by powers of two;
    the products of the scale factors must not leave the float range), cameras hundreds of scene radii away (its halves would
    overflow: filter off for those rays), and the plain cases in between: every scan against the oracle, bit for bit."""
    rng = np.random.default_rng(77)
    t0, _ = scene.closed_room(300)
    n = 6000
    for scene_scale, dir_scale, far in ((1e-28, 1e-17, 1.0), (1e-28, 1e17, 1.0), (1e25, 1e-17, 1.0), (1e25, 1e10, 1.0), (1e-12, 1e-6, 1.0),
                                       (1.0, 1.0, 700.0), (1.0, 1e-10, 3000.0), (1e-3, 1e3, 1.0e5), (1.0, 1.0, 1.0)):
        t = t0.copy()
        t[:, :9] *= np.float32(scene_scale)
        v = t[:, :9].reshape(-1, 3, 3)
        o = rng.uniform(-1.4, 1.4, (n, 3)) * [1, 0.5, 1] * scene_scale * far
        k = rng.integers(0, t.shape[0], n); bw = rng.dirichlet([0.5, 0.5, 0.5], n)
        d = (v[k] * bw[:, :, None]).sum(1).astype(np.float64) - o                   # aimed at the triangles
        d[n // 2:] = rng.normal(size=(n - n // 2, 3))                               # and random directions
        d = d / np.linalg.norm(d, axis=1, keepdims=True) * dir_scale
        rays = np.concatenate([o, d], axis=1).astype(np.float32)
        with np.errstate(all="ignore"):
            hip.set_scene(t, np.full((t.shape[0], 6), 0.5, dtype=np.float32))
            idx = _hits(hip, O, t, rays, (scene_scale, dir_scale, far))
        if 1e-4 < scene_scale < 1e3 and far <= 1.0:                # (elsewhere the determinant falls under the epsilon of geom.h:204 or overflows: no hits at all)
            assert (idx >= 0).mean() > 0.3, (scene_scale, dir_scale, far)
