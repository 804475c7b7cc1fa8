"""Adaptive sampling (include/spath_hip.h: sphip_accum_begin_adaptive, sphip_accum_counts): a progressive accumulation whose
converged pixels stop after a step, while the rest go on.

Why it can be exact per pixel: the counter RNG is keyed by (seed, global pixel, sample index, depth) and each pixel's f32 sum
is built one sample at a time in sample order, so a pixel that stopped after n samples holds the bits a one-shot render of n
samples gives it.  The decisions are the stated rule on double sums of y = ((double)r + (double)g) + (double)b, so they can be
replayed in numpy from every sample's radiance, which sphip_render_device_accum returns bit for bit (one sample onto a zero sum).
STATED TOLERANCE: 0 -- every comparison below is bit for bit, and the counts must equal the replay exactly.

CPU part: the entry points are declared, bound and exported; a NULL context is an argument error; the numpy model of the rule
gives hand-derived decisions on hand-made sample streams.
GPU part: per-pixel exactness for every kernel variant, chunking, primary-hit reuse and the BVH; the decisions against the
replay; no stop before min_samples; skipped work; isolation and the error contract; multi-device contexts; the Python and C++
front ends; the full-size frame."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from hip_checks import E_INVALID, E_STATE, H, W, cam_rays
from path_model import _bits
from spath_amd import capi, scene, view

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "spath_amd", "host", "build", "spath_cli")
SPLITS = [[4] * 8, [3, 5, 8], [7, 9]]
SCENES = {"closed_room_200": lambda: scene.closed_room(200), "default": scene.default_scene, "open_clutter_100": lambda: scene.open_clutter(100)}


def model(y, split, t, floor, min_samples):
    """The rule of include/spath_hip.h in float64, in the stated order.  y[p, s]: the luminance proxy of sample s of pixel p.
    -> after every step: (counts, n_active, total)."""
    n_pix = y.shape[0]
    counts = np.zeros(n_pix, np.int64)
    s1, s2 = np.zeros(n_pix), np.zeros(n_pix)
    active = np.ones(n_pix, bool)
    total, out = 0, []
    for n in split:
        if active.any():
            for j in range(total, total + n):
                yy = y[active, j]
                s1[active] = s1[active] + yy
                s2[active] = s2[active] + yy * yy
            counts[active] += n
            total += n
            idx = np.flatnonzero(active & (counts >= min_samples))
            nn = counts[idx].astype(np.float64)
            m = s1[idx] / nn
            v = (s2[idx] - s1[idx] * m) / (nn - 1.0)
            r = np.where(m > floor, m, floor)
            d = t * r
            active[idx[v / nn <= d * d]] = False
        out.append((counts.copy(), int(active.sum()), total))
    return out


def _check_pixels(counts, img, mean, one_shot):
    """every pixel's RGBA8 and mean equal those of a one-shot render of its own count (one render per distinct count)"""
    c = counts.ravel()
    for n in np.unique(c):
        want_img, want_mean = one_shot(int(n))
        sel = c == n
        assert np.array_equal(img[sel], want_img[sel]), n
        assert np.array_equal(_bits(mean[sel]), _bits(want_mean[sel])), n


def _cached(render):
    cache = {}

    def get(n):
        if n not in cache:
            cache[n] = render(n)
        return cache[n]
    return get


# ------------------------------------------------------------------------------------------------------------------ CPU part
def test_entry_points_declared_bound_exported():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "spath_hip.h")).read(), flags=re.S)
    lib = C.CDLL(capi.LIB_PATH)
    for name in ("sphip_accum_begin_adaptive", "sphip_accum_counts"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in capi.SYMBOLS and hasattr(lib, name), name
    assert re.search(r"\}\s*sphip_adaptive\s*;", hdr)
    assert [f for f, _ in capi.Adaptive._fields_] == ["rel_error", "floor", "min_samples", "reserved"] and C.sizeof(capi.Adaptive) == 24
    assert hasattr(capi.Context, "accum_counts")


def test_null_context_and_bad_rules_are_argument_errors():
    L = capi.load()
    good = capi.Adaptive(0.1, 0.0, 4, 0)
    counts = (C.c_uint32 * 4)()
    n_active = C.c_uint64(7)
    assert L.sphip_accum_begin_adaptive(None, None, None, 2, 2, 1, 0, C.byref(good)) == -1
    assert L.sphip_accum_begin_adaptive(None, None, None, 2, 2, 1, 0, None) == -1
    for bad in [(0.1, 0.0, 1, 0), (-0.1, 0.0, 4, 0), (float("nan"), 0.0, 4, 0), (float("inf"), 0.0, 4, 0),
                (0.1, -1.0, 4, 0), (0.1, float("nan"), 4, 0), (0.1, 0.0, 4, 1)]:
        assert L.sphip_accum_begin_adaptive(None, None, None, 2, 2, 1, 0, C.byref(capi.Adaptive(*bad))) == -1, bad
    assert L.sphip_accum_counts(None, counts, C.byref(n_active)) == -1 and n_active.value == 7
    assert L.sphip_accum_counts(None, None, None) == -1


def test_model_on_hand_made_streams():
    S = 16
    ones = np.ones(S)
    zeros = np.zeros(S)
    alt = np.tile([0.0, 1.0], S // 2)                  # m = 1/2, v = n/(4(n-1))
    small = np.tile([0.0, 0.02], S // 2)
    outlier = np.ones(S)
    outlier[1] = 5.0
    y = np.stack([ones, zeros, alt, small, outlier])

    def counts(t, floor, mn, split):
        return [list(c) for c, _, _ in model(y, split, t, floor, mn)]
    # constant and zero streams have v = 0: they stop at min_samples, for t = 0 too; alternating 0/1 at t = 1/2 needs
    # v/n <= 1/16: n = 4 gives 1/12, n = 6 gives 1/20; the outlier at t = 0.3: v/n = 1, 1/4, 1/9 against d^2 = .36, .2025, .16
    got = counts(0.5, 0.0, 4, [2, 2, 2, 2])
    assert [g[0] for g in got] == [2, 4, 4, 4] and [g[1] for g in got] == [2, 4, 4, 4]
    assert [g[2] for g in got] == [2, 4, 6, 6]           # a decision at n = 6 exists only because a step ended there
    assert [g[2] for g in counts(0.5, 0.0, 4, [4, 4, 4])] == [4, 8, 8]       # (n = 8: v/n = 1/28)
    assert [g[4] for g in counts(0.3, 0.0, 4, [4, 4, 4, 4])] == [4, 8, 12, 12]
    # t = 0: only streams of zero variance stop
    got = counts(0.0, 0.0, 4, [4, 4, 4, 4])
    assert [g[0] for g in got] == [4, 4, 4, 4] and [g[1] for g in got] == [4, 4, 4, 4]
    assert all(g[2] == g[3] == g[4] == 4 * (i + 1) for i, g in enumerate(got))
    # the floor: a dark noisy stream (m = 0.01) measured relatively needs n = 8 (v/n = 3.3e-5, 1.4e-5 against 2.5e-5); with
    # floor 1 its error is measured against 1 and it stops at min_samples
    assert [g[3] for g in counts(0.5, 0.0, 4, [4, 4, 4])] == [4, 8, 8]
    assert [g[3] for g in counts(0.5, 1.0, 4, [4, 4, 4])] == [4, 4, 4]
    # nothing stops before min_samples, and the active count follows the stops
    out = model(y, [2, 2, 2, 2], 10.0, 0.0, 6)
    assert [a for _, a, _ in out] == [5, 5, 0, 0] and [t for _, _, t in out] == [2, 4, 6, 6]


# ------------------------------------------------------------------------------------------------------------------ GPU part
def _sample_y(hip, rays, w, h, seed, flags, n_total, shard=None):
    """y[p, s] of every pixel and sample, from each sample's radiance (sphip_render_device_accum, one sample onto a zero sum)"""
    import torch
    d_rays = torch.from_numpy(rays).cuda()
    d_sum = torch.zeros((w * h, 3), dtype=torch.float32, device="cuda")
    d_rgba = torch.zeros((w * h, 4), dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    y = np.zeros((w * h, n_total))
    for s in range(n_total):
        d_sum.zero_()
        hip.render_device_accum(d_rays.data_ptr(), w * h, s, 1, d_sum.data_ptr(), d_rgba.data_ptr(), seed=seed, flags=flags,
                                image_width=w, stream=st)
        torch.cuda.synchronize()
        rad = d_sum.cpu().numpy().astype(np.float64)
        y[:, s] = (rad[:, 0] + rad[:, 1]) + rad[:, 2]
    return y


@pytest.mark.gpu
@pytest.mark.parametrize("scene_name", list(SCENES))
@pytest.mark.parametrize("split", SPLITS, ids=["4x8", "3-5-8", "7-9"])
def test_every_pixel_equals_a_one_shot_render_of_its_count(hip, scene_name, split):
    t, m = SCENES[scene_name]()
    _, rays = cam_rays()
    hip.set_scene(t, m)
    seed, rule = 0x5EED, (0.25, 0.05, 3)
    plain = _cached(lambda n: hip.render(rays, W, H, n, seed=seed, want_accum=True))
    accel = _cached(lambda n: hip.render(rays, W, H, n, seed=seed, flags=capi.FLAG_ACCEL, want_accum=True))
    runs = [v | ch for v in [0] + capi.available_variants() for ch in (capi.flag_chunks(1), 0, capi.flag_chunks(8))]
    runs += [capi.FLAG_PRIMARY_REUSE, capi.FLAG_PRIMARY_REUSE | capi.flag_chunks(8), capi.FLAG_ACCEL]
    first = None
    for flags in runs:
        is_accel = (flags & capi.FLAG_ACCEL) or (flags & 0xff) == capi.kernel_variants()["accel_lbvh"]
        one_shot = accel if is_accel else plain
        hip.accum_begin(rays=rays, w=W, h=H, seed=seed, flags=flags, adaptive=rule)
        seq = []
        for n in split:
            img, mean, tot = hip.accum_step(n, want_mean=True)
            counts, n_active = hip.accum_counts()
            assert counts.shape == (H, W) and counts.max() == tot and n_active <= int((counts == tot).sum())
            _check_pixels(counts, img, mean, one_shot)
            seq.append((counts, n_active, tot))
        # the decisions do not depend on the variant, chunking or primary-hit reuse (the BVH may differ by its stated noise)
        if not is_accel:
            if first is None:
                first = seq
            for (c0, a0, t0), (c1, a1, t1) in zip(first, seq):
                assert np.array_equal(c0, c1) and a0 == a1 and t0 == t1, flags


@pytest.mark.gpu
@pytest.mark.parametrize("split", SPLITS, ids=["4x8", "3-5-8", "7-9"])
def test_decisions_are_the_rule(hip, split):
    t, m = scene.closed_room(200)
    _, rays = cam_rays()
    hip.set_scene(t, m)
    seed = 77
    y = _sample_y(hip, rays, W, H, seed, 0, sum(split))
    partial = 0
    for rule in [(0.05, 0.05, 2), (0.2, 0.05, 4), (0.5, 0.0, 3), (1.0, 0.2, 2)]:
        want = model(y, split, *rule)
        hip.accum_begin(rays=rays, w=W, h=H, seed=seed, adaptive=rule)
        for n, (wc, wa, wt) in zip(split, want):
            _, tot = hip.accum_step(n)
            counts, n_active = hip.accum_counts()
            assert np.array_equal(counts.ravel(), wc) and n_active == wa and tot == wt, (rule, n)
        partial += 0 < want[-1][1] < W * H
    assert partial, "no rule stopped some but not all pixels"


@pytest.mark.gpu
def test_no_stop_before_min_samples(hip):
    t, m = scene.closed_room(200)
    _, rays = cam_rays()
    hip.set_scene(t, m)
    for flags in (0, capi.FLAG_PRIMARY_REUSE, capi.flag_chunks(1)):
        plain, adaptive = [], []
        for rule in (None, (1e6, 1.0, 17)):                  # would stop everything, but not before 17 samples
            hip.accum_begin(rays=rays, w=W, h=H, seed=3, flags=flags, adaptive=rule)
            for n in (3, 5, 8):
                img, mean, tot = hip.accum_step(n, want_mean=True)
                (plain if rule is None else adaptive).append((img, _bits(mean), tot, hip.stats()["scans_executed"], hip.accum_counts()))
        for p, a in zip(plain, adaptive):
            assert np.array_equal(p[0], a[0]) and np.array_equal(p[1], a[1]) and p[2] == a[2] and p[3] == a[3]
            assert np.array_equal(p[4][0], a[4][0]) and p[4][1] == a[4][1] == W * H and np.all(a[4][0] == a[2])


@pytest.mark.gpu
def test_stopped_pixels_skip_work(hip):
    import torch
    t, m = scene.open_clutter(100)
    _, rays = cam_rays()
    hip.set_scene(t, m)
    d_rays = torch.from_numpy(rays).cuda()
    d_idx = torch.zeros(W * H, dtype=torch.int32, device="cuda")
    d_dist = torch.zeros(W * H, dtype=torch.float32, device="cuda")
    hip.closest_hit_device(d_rays.data_ptr(), W * H, d_idx.data_ptr(), d_dist.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    escaped = d_idx.cpu().numpy() < 0
    assert 0 < escaped.sum() < W * H
    # a tight rule: the escaping pixels (radiance exactly 0 on every sample) stop at min_samples, and no later step traces them
    hip.accum_begin(rays=rays, w=W, h=H, seed=5, adaptive=(0.01, 0.0, 4))
    for n in (2, 2, 2, 2):
        hip.accum_step(n)
    counts, n_active = hip.accum_counts()
    assert np.all(counts.ravel()[escaped] == 4)
    assert n_active < W * H
    img, tot = hip.accum_step(2)
    adaptive_scans = hip.stats()["scans_executed"]
    hip.accum_begin(rays=rays, w=W, h=H, seed=5)
    for n in (2, 2, 2, 2, 2):
        hip.accum_step(n)
    plain_scans = hip.stats()["scans_executed"]
    assert adaptive_scans < plain_scans
    # a loose rule: every pixel stops at min_samples; the next step renders nothing
    hip.accum_begin(rays=rays, w=W, h=H, seed=5, adaptive=(1e6, 0.0, 4))
    hip.accum_step(3)
    img, mean, tot = hip.accum_step(1, want_mean=True)
    counts, n_active = hip.accum_counts()
    assert tot == 4 and n_active == 0 and np.all(counts == 4)
    img2, mean2, tot2 = hip.accum_step(5, want_mean=True)
    st = hip.stats()
    assert tot2 == 4 and st["scans_executed"] == 0
    assert np.array_equal(img2, img) and np.array_equal(_bits(mean2), _bits(mean))
    want_img, want_mean = hip.render(rays, W, H, 4, seed=5, want_accum=True)
    assert np.array_equal(img2, want_img) and np.array_equal(_bits(mean2), _bits(want_mean))


@pytest.mark.gpu
def test_isolation_and_state(hip):
    t, m = scene.closed_room(200)
    hip.set_scene(t, m)
    _, rays = cam_rays()
    cam2, rays2 = cam_rays(37, 21, ((0.0, 0.2, 0.1), (0.0, 0.3, 0.0)))
    rule, split = (0.3, 0.05, 3), [3, 5, 8]
    runs = []
    for interleave in (False, True):
        hip.accum_begin(rays=rays, w=W, h=H, seed=9, adaptive=rule)
        out = []
        for n in split:
            img, mean, tot = hip.accum_step(n, want_mean=True)
            out.append((img, _bits(mean), tot) + hip.accum_counts())
            if interleave:
                hip.render(rays2, 37, 21, 13, seed=123, want_accum=True)
                hip.render_camera(cam2, 6, seed=77, want_accum=True)
                hip.render(rays2, 37, 21, 1, seed=1, mode=capi.MODE_FLAT)
        runs.append(out)
    for a, b in zip(*runs):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] and np.array_equal(a[3], b[3]) and a[4] == b[4]
    # a plain begin after an adaptive one is plain again
    hip.accum_begin(rays=rays, w=W, h=H, seed=9)
    img, tot = hip.accum_step(4)
    counts, n_active = hip.accum_counts()
    assert tot == 4 and n_active == W * H and np.all(counts == 4) and np.array_equal(img, hip.render(rays, W, H, 4, seed=9))

    fresh = capi.Context(0)
    with pytest.raises(capi.SpathHipError, match=E_STATE):
        fresh.accum_counts()                                                        # nothing begun
    with pytest.raises(capi.SpathHipError, match=E_STATE):
        fresh.accum_begin(rays=rays, w=W, h=H, adaptive=rule)                       # no scene
    fresh.set_scene(t, m)
    for bad in [(0.1, 0.0, 1), (-0.1, 0.0, 4), (float("nan"), 0.0, 4), (0.1, float("inf"), 4), (0.1, -0.5, 4)]:
        with pytest.raises(capi.SpathHipError, match=E_INVALID):
            fresh.accum_begin(rays=rays, w=W, h=H, adaptive=bad)
    rb = capi.Adaptive(0.1, 0.0, 4, 3)
    assert fresh._L.sphip_accum_begin_adaptive(fresh._h, rays.ctypes.data, None, W, H, 1, 0, C.byref(rb)) == -1   # reserved != 0
    with pytest.raises(capi.SpathHipError, match=E_INVALID):
        fresh.accum_begin(w=W, h=H, adaptive=rule)                                  # neither rays nor cam
    fresh.accum_begin(rays=rays, w=W, h=H, seed=2, adaptive=rule)
    with pytest.raises(capi.SpathHipError, match=E_INVALID):
        fresh.accum_step(0)
    fresh.accum_step(4)
    fresh.set_scene(*scene.closed_room(100))
    with pytest.raises(capi.SpathHipError, match=E_STATE):
        fresh.accum_step(1)                                                         # the scene changed under the sums
    fresh.close()


@pytest.mark.gpu
@pytest.mark.parametrize("devices", [[0], [0, 0], [0, 0, 0]])
def test_multi_device_equals_single_context(hip, devices):
    t, m = scene.open_clutter(300)
    hip.set_scene(t, m)
    mc = capi.Context.multi(devices)
    mc.set_scene(t, m)
    rule = (0.3, 0.05, 3)
    for (w, h) in [(61, 37), (16, 5)]:
        cam, rays = cam_rays(w, h)
        hip.accum_begin(rays=rays, w=w, h=h, seed=21, adaptive=rule)
        want = []
        for n in [2, 3, 1, 4]:
            img, mean, tot = hip.accum_step(n, want_mean=True)
            want.append((img, _bits(mean), tot) + hip.accum_counts())
        for begin in (lambda: mc.accum_begin(rays=rays, w=w, h=h, seed=21, adaptive=rule),
                      lambda: mc.accum_begin(cam=cam, seed=21, adaptive=rule)):
            begin()
            for n, wv in zip([2, 3, 1, 4], want):
                img, mean, tot = mc.accum_step(n, want_mean=True)
                counts, n_active = mc.accum_counts()
                assert np.array_equal(img, wv[0]) and np.array_equal(_bits(mean), wv[1]) and tot == wv[2]
                assert np.array_equal(counts, wv[3]) and n_active == wv[4]
    mc.close()


@pytest.mark.gpu
def test_python_renderer_matches_capi(hip):
    from spath_amd.renderer import Bitmap, HipRenderer, Viewport
    t, m = scene.closed_room(200)
    rule = (0.3, 0.05, 3)
    with pytest.raises(ValueError):
        HipRenderer(W, H, adaptive=rule)                                            # needs progressive=True
    r = HipRenderer(W, H, progressive=True, adaptive=rule, seed=4)
    vp, out = Viewport(), Bitmap()
    r.get_viewport(vp)
    hip.set_scene(t, m)
    hip.accum_begin(rays=vp.rays, w=W, h=H, seed=4, adaptive=rule)
    for n in (2, 3, 4):
        r.render(vp, t, m, len(t), n, out)
        want, _ = hip.accum_step(n)
        assert np.array_equal(out.values, want)
        c_r, a_r = r.adaptive_counts()
        c_h, a_h = hip.accum_counts()
        assert np.array_equal(c_r, c_h) and a_r == a_h
    r.close()


def _read_pgm16(path):
    data = open(path, "rb").read()
    mt = re.match(rb"P5\s+(\d+)\s+(\d+)\s+(\d+)\s", data)
    w, h, mx = (int(v) for v in mt.groups())
    assert mx == 65535
    return np.frombuffer(data[mt.end():], dtype=">u2").reshape(h, w)


@pytest.mark.gpu
def test_cli_adaptive_matches_capi(hip, tmp_path):
    t, m = scene.closed_room(300)
    sp = os.path.join(tmp_path, "s.bin")
    scene.write_scene(sp, t, m)
    w, h = 40, 30
    img_p, cnt_p = os.path.join(tmp_path, "a.rgba"), os.path.join(tmp_path, "c.pgm")
    p = subprocess.run([CLI, "--scene", sp, "--w", str(w), "--h", str(h), "--spp", "16", "--seed", "9", "--progressive", "4",
                        "--adaptive", "0.3,0.05,4", "--out", img_p, "--counts-out", cnt_p], check=True, capture_output=True, text=True, timeout=120)
    steps = [l for l in p.stdout.splitlines() if l.strip().startswith("step ")]
    assert len(steps) == 4 and all("pixels active" in l for l in steps)
    rays = np.ascontiguousarray(view.Camera(w, h).get_viewport(), dtype=np.float32)
    hip.set_scene(t, m)
    hip.accum_begin(rays=rays, w=w, h=h, seed=9, adaptive=(0.3, 0.05, 4))
    for _ in range(4):
        img, _ = hip.accum_step(4)
    counts, _ = hip.accum_counts()
    assert open(img_p, "rb").read() == img.tobytes()
    assert np.array_equal(_read_pgm16(cnt_p), np.minimum(counts, 65535))
    # bad values are refused before anything renders
    bad = subprocess.run([CLI, "--scene", sp, "--w", "8", "--h", "8", "--progressive", "2", "--adaptive", "x"], capture_output=True, timeout=60)
    assert bad.returncode != 0


@pytest.mark.gpu
def test_full_size_frame(hip):
    t, m = scene.closed_room(10000)
    hip.set_scene(t, m)
    w, h = 1920, 1080
    rays = np.ascontiguousarray(view.Camera(w, h).get_viewport(), dtype=np.float32)
    hip.accum_begin(rays=rays, w=w, h=h, seed=1, adaptive=(0.5, 0.1, 4))
    rng = np.random.default_rng(1)
    sample = rng.choice(w * h, 4096, replace=False)
    one_shot = _cached(lambda n: hip.render(rays, w, h, n, seed=1, want_accum=True))
    actives = []
    for n in (4, 4, 4, 4):
        img, mean, tot = hip.accum_step(n, want_mean=True)
        counts, n_active = hip.accum_counts()
        st = hip.stats()
        assert st["kernel_variant"] == capi.kernel_variants()["rpl_cylm"] and st["n_pixels"] == w * h
        actives.append(n_active)
        c = counts.ravel()[sample]
        for k in np.unique(c):
            want_img, want_mean = one_shot(int(k))
            sel = sample[c == k]
            assert np.array_equal(img[sel], want_img[sel]) and np.array_equal(_bits(mean[sel]), _bits(want_mean[sel])), k
    assert actives[-1] < w * h and all(a >= b for a, b in zip(actives, actives[1:]))
