"""Progressive rendering (include/spath_hip.h: sphip_render_device_accum, sphip_accum_begin, sphip_accum_step): samples
accumulated over several calls give, after every call, exactly the image and mean of one render of all of them so far.

Why it can be exact: the counter RNG is keyed by (seed, global pixel, sample index, depth), and every kernel adds the samples
to an f32 sum one at a time in sample order; a step starts from the running sum and continues the sample indices.
STATED TOLERANCE: 0 -- every comparison below is bit for bit, against one-shot renders of the library and (default variant)
against the oracle.

CPU part: the new entry points are declared, bound and exported, and a NULL context is an argument error, not a crash.
GPU part: steps against one-shot renders for every kernel variant, chunking, primary-hit reuse and the BVH; the device-pointer
form on shards; camera begin; isolation from renders in between; multi-device contexts; the error contract; the full-size
production kernel; the Python and C++ front ends."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from hip_checks import E_INVALID, E_STATE, H, W, cam_rays
from spath_amd import capi, scene, view

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "spath_amd", "host", "build", "spath_cli")
SPLITS = [[1] * 6, [3, 5, 8], [7, 9]]
SCENES = {"closed_room_200": lambda: scene.closed_room(200), "default": scene.default_scene, "open_clutter_100": lambda: scene.open_clutter(100)}


def _check_steps(ctx, one_shot, split, on_step=None):
    """ctx holds a begun accumulation; after each step its outputs equal one_shot(cumulative)."""
    total = 0
    for n in split:
        img, mean, tot = ctx.accum_step(n, want_mean=True)
        total += n
        assert tot == total
        want_img, want_mean = one_shot(total)
        assert np.array_equal(img, want_img), (split, total)
        assert np.array_equal(mean.view(np.uint32), want_mean.view(np.uint32)), (split, total)
        if on_step:
            on_step(total, img, mean)


# ------------------------------------------------------------------------------------------------------------------ CPU part
def test_new_entry_points_declared_bound_exported():
    import re
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "spath_hip.h")).read(), flags=re.S)
    lib = C.CDLL(capi.LIB_PATH)
    for name in ("sphip_render_device_accum", "sphip_accum_begin", "sphip_accum_step"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in capi.SYMBOLS and hasattr(lib, name), name
    assert hasattr(capi.Context, "render_device_accum") and hasattr(capi.Context, "accum_begin") and hasattr(capi.Context, "accum_step")


def test_null_context_is_an_argument_error():
    L = capi.load()
    buf = (C.c_uint8 * 16)()
    total = C.c_uint64(7)
    assert L.sphip_accum_begin(None, None, None, 2, 2, 1, 0) == -1
    assert L.sphip_accum_step(None, 1, buf, None, C.byref(total)) == -1 and total.value == 7
    assert L.sphip_render_device_accum(None, None, 4, None, 2, 0, 1, 1, 0, None, None, None, None) == -1


# ------------------------------------------------------------------------------------------------------------------ GPU part
@pytest.fixture(scope="module")
def oracle_cache(O):
    cache = {}

    def get(name, t, m, rays, total, seed):
        key = (name, total, seed, rays.shape[0])
        if key not in cache:
            img, acc, _ = O.render_counter(rays, t, m, total, seed)
            cache[key] = (img, acc)
        return cache[key]
    return get


@pytest.mark.gpu
@pytest.mark.parametrize("scene_name", list(SCENES))
@pytest.mark.parametrize("split", SPLITS, ids=["ones", "3-5-8", "7-9"])
def test_steps_equal_one_shot_for_every_variant_and_chunking(hip, oracle_cache, scene_name, split):
    t, m = SCENES[scene_name]()
    _, rays = cam_rays()
    hip.set_scene(t, m)
    seed = 0x5EED
    for variant in [0] + capi.available_variants():
        for chunks in (capi.flag_chunks(1), 0, capi.flag_chunks(8)):
            flags = variant | chunks
            hip.accum_begin(rays=rays, w=W, h=H, seed=seed, flags=flags)

            def one_shot(total):
                img, acc = hip.render(rays, W, H, total, seed=seed, flags=flags, want_accum=True)
                if variant == 0:
                    o_img, o_acc = oracle_cache(scene_name, t, m, rays, total, seed)
                    assert np.array_equal(img, o_img) and np.array_equal(acc.view(np.uint32), o_acc.view(np.uint32)), (flags, total)
                return img, acc
            _check_steps(hip, one_shot, split)


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [capi.FLAG_PRIMARY_REUSE, capi.FLAG_ACCEL, capi.FLAG_PRIMARY_REUSE | capi.flag_chunks(8)],
                         ids=["primary_reuse", "accel", "primary_reuse_chunks8"])
def test_steps_equal_one_shot_with_flags(hip, flags):
    t, m = scene.closed_room(200)
    _, rays = cam_rays()
    hip.set_scene(t, m)
    for split in SPLITS:
        hip.accum_begin(rays=rays, w=W, h=H, seed=3, flags=flags)
        _check_steps(hip, lambda total: hip.render(rays, W, H, total, seed=3, flags=flags, want_accum=True), split)


@pytest.mark.gpu
@pytest.mark.parametrize("g", [2, 3])
def test_device_form_on_shards(hip, g):
    import torch
    t, m = scene.closed_room(200)
    _, rays = cam_rays()
    hip.set_scene(t, m)
    seed, steps = 11, [3, 5, 2]
    tr = capi.plan_tile_rows(H, g)
    st = torch.cuda.current_stream().cuda_stream
    shards = []
    for r in range(g):
        sh, n = capi.plan_shard(W, H, g, tr, r)
        k = np.arange(n, dtype=np.int64)
        pix = sh[0] + (k // sh[1]) * sh[2] + (k % sh[1])
        shards.append(dict(sh=sh, n=n, pix=pix, rays=torch.from_numpy(rays[pix]).cuda(),
                           sum=torch.full((n, 3), float("nan"), dtype=torch.float32, device="cuda"),      # stale contents: must not leak in
                           rgba=torch.zeros((n, 4), dtype=torch.uint8, device="cuda"),
                           mean=torch.zeros((n, 3), dtype=torch.float32, device="cuda")))
    base = 0
    for n_s in steps:
        for s in shards:
            hip.render_device_accum(s["rays"].data_ptr(), s["n"], base, n_s, s["sum"].data_ptr(), s["rgba"].data_ptr(), seed=seed,
                                    shard=s["sh"], image_width=W, d_out_mean=s["mean"].data_ptr(), stream=st)
        torch.cuda.synchronize()
        base += n_s
        img = np.zeros((W * H, 4), dtype=np.uint8)
        mean = np.zeros((W * H, 3), dtype=np.float32)
        for s in shards:
            img[s["pix"]] = s["rgba"].cpu().numpy()
            mean[s["pix"]] = s["mean"].cpu().numpy()
        want_img, want_mean = hip.render(rays, W, H, base, seed=seed, want_accum=True)
        assert np.array_equal(img, want_img) and np.array_equal(mean.view(np.uint32), want_mean.view(np.uint32)), base
    # a sum buffer full of NaN used at sample_base 0: the fresh result (also without the mean output)
    s = shards[0]
    s["sum"].fill_(float("nan"))
    hip.render_device_accum(s["rays"].data_ptr(), s["n"], 0, 4, s["sum"].data_ptr(), s["rgba"].data_ptr(), seed=seed,
                            shard=s["sh"], image_width=W, stream=st)
    torch.cuda.synchronize()
    want_img, want_mean = hip.render(rays, W, H, 4, seed=seed, want_accum=True)
    assert np.array_equal(s["rgba"].cpu().numpy(), want_img[s["pix"]])
    assert np.array_equal((s["sum"].cpu().numpy() * np.float32(0.25)).view(np.uint32), want_mean[s["pix"]].view(np.uint32))


@pytest.mark.gpu
def test_camera_begin_equals_rays_begin(hip):
    t, m = scene.open_clutter(100)
    hip.set_scene(t, m)
    cam, rays = cam_rays(W, H, ((0.3, 0.1, -0.5), (0.1, -0.25, 0.0)))
    cam.set_delta_focal(0.5)
    rays = np.ascontiguousarray(cam.get_viewport(), dtype=np.float32)
    results = []
    hip.accum_begin(rays=rays, w=W, h=H, seed=5)
    _check_steps(hip, lambda total: hip.render(rays, W, H, total, seed=5, want_accum=True), [2, 3, 4],
                 on_step=lambda total, img, mean: results.append((img, mean)))
    hip.accum_begin(cam=cam, seed=5)
    for (n, (img, mean)) in zip([2, 3, 4], results):
        i2, m2, _ = hip.accum_step(n, want_mean=True)
        assert np.array_equal(i2, img) and np.array_equal(m2.view(np.uint32), mean.view(np.uint32))


@pytest.mark.gpu
def test_renders_between_steps_do_not_disturb_the_accumulation(hip):
    t, m = scene.closed_room(200)
    hip.set_scene(t, m)
    _, rays = cam_rays()
    cam2, rays2 = cam_rays(37, 21, ((0.0, 0.2, 0.1), (0.0, 0.3, 0.0)))
    hip.accum_begin(rays=rays, w=W, h=H, seed=9)

    def interleave(total, img, mean):
        hip.render(rays2, 37, 21, 13, seed=123, want_accum=True)                # other size, spp and seed
        hip.render_camera(cam2, 6, seed=77, want_accum=True)
        hip.render(rays2, 37, 21, 1, seed=1, mode=capi.MODE_FLAT)
    one_shot = lambda total: hip.render(rays, W, H, total, seed=9, want_accum=True)
    _check_steps(hip, one_shot, [3, 5, 8], on_step=interleave)


@pytest.mark.gpu
@pytest.mark.parametrize("devices", [[0, 0], [0, 0, 0]])
def test_multi_device_steps_equal_single_context_one_shot(hip, devices):
    t, m = scene.open_clutter(300)
    hip.set_scene(t, m)
    mc = capi.Context.multi(devices)
    mc.set_scene(t, m)
    for (w, h) in [(61, 37), (16, 5)]:
        cam, rays = cam_rays(w, h)
        for begin in (lambda: mc.accum_begin(rays=rays, w=w, h=h, seed=21), lambda: mc.accum_begin(cam=cam, seed=21)):
            begin()
            total = 0
            for n in [2, 3, 1]:
                img, mean, tot = mc.accum_step(n, want_mean=True)
                total += n
                want_img, want_mean = hip.render(rays, w, h, total, seed=21, want_accum=True)
                assert tot == total and np.array_equal(img, want_img) and np.array_equal(mean.view(np.uint32), want_mean.view(np.uint32))
                st = mc.stats()
                assert 1 <= st["n_devices"] <= len(devices) and st["gather_kind"] == capi.GATHER_PEER      # as test_multi_device.py
            img, tot = mc.accum_step(4)                                          # RGBA8 only
            assert np.array_equal(img, hip.render(rays, w, h, total + 4, seed=21))
    mc.close()


@pytest.mark.gpu
def test_error_contract(hip):
    t, m = scene.default_scene()
    _, rays = cam_rays()
    fresh = capi.Context(0)
    with pytest.raises(capi.SpathHipError, match=E_STATE):
        fresh.accum_begin(rays=rays, w=W, h=H)                                  # before any scene
    fresh.set_scene(t, m)
    with pytest.raises(capi.SpathHipError, match=E_STATE):
        fresh.accum_step(1)                                                      # no accumulation begun
    with pytest.raises(capi.SpathHipError, match=E_INVALID):
        fresh.accum_begin(w=W, h=H)                                              # neither rays nor cam
    cam = view.Camera(W, H)
    with pytest.raises(capi.SpathHipError, match=E_INVALID):
        fresh.accum_begin(rays=rays, cam=cam, w=W, h=H)                          # both
    fresh.accum_begin(rays=rays, w=W, h=H, seed=2)
    with pytest.raises(capi.SpathHipError, match=E_INVALID):
        fresh.accum_step(0)
    fresh.accum_step(5)
    with pytest.raises(capi.SpathHipError, match=E_INVALID):
        fresh.accum_step((1 << 31) - 5)                                          # total would reach 2^31
    assert fresh._L.sphip_accum_step(fresh._h, 1, None, None, None) == -1        # NULL out_rgba
    # argument errors leave the accumulation intact
    img, tot = fresh.accum_step(2)
    assert tot == 7 and np.array_equal(img, fresh.render(rays, W, H, 7, seed=2))
    fresh.set_scene(*scene.closed_room(100))
    with pytest.raises(capi.SpathHipError, match=E_STATE):
        fresh.accum_step(1)                                                      # the scene changed under the sum
    fresh.accum_begin(rays=rays, w=W, h=H, seed=2)                               # a new begin recovers
    img, tot = fresh.accum_step(3)
    assert tot == 3 and np.array_equal(img, fresh.render(rays, W, H, 3, seed=2))
    # device form: null sum, a total reaching 2^31, and a multi-device context
    import torch
    d_rays = torch.from_numpy(rays).cuda()
    d_sum = torch.zeros((W * H, 3), dtype=torch.float32, device="cuda")
    d_rgba = torch.zeros((W * H, 4), dtype=torch.uint8, device="cuda")
    with pytest.raises(capi.SpathHipError, match=E_INVALID):
        fresh.render_device_accum(d_rays.data_ptr(), W * H, 0, 1, 0, d_rgba.data_ptr())
    with pytest.raises(capi.SpathHipError, match=E_INVALID):
        fresh.render_device_accum(d_rays.data_ptr(), W * H, (1 << 31) - 2, 2, d_sum.data_ptr(), d_rgba.data_ptr())
    torch.cuda.synchronize()
    fresh.close()
    mc = capi.Context.multi([0, 0])
    mc.set_scene(t, m)
    with pytest.raises(capi.SpathHipError, match=E_STATE):
        mc.render_device_accum(d_rays.data_ptr(), W * H, 0, 1, d_sum.data_ptr(), d_rgba.data_ptr())
    with pytest.raises(capi.SpathHipError, match=E_STATE):
        mc.accum_step(1)
    mc.close()


@pytest.mark.gpu
def test_full_size_production_kernel(hip):
    t, m = scene.closed_room(10000)
    hip.set_scene(t, m)
    w, h = 1920, 1080
    rays = np.ascontiguousarray(view.Camera(w, h).get_viewport(), dtype=np.float32)
    want_img, want_mean = hip.render(rays, w, h, 8, seed=1, want_accum=True)
    want_scans = hip.stats()["scans_executed"]
    hip.accum_begin(rays=rays, w=w, h=h, seed=1)
    scans = 0
    for _ in range(4):
        img, mean, tot = hip.accum_step(2, want_mean=True)
        st = hip.stats()
        scans += st["scans_executed"]
        assert st["kernel_variant"] == capi.kernel_variants()["rpl_cylm"] and st["n_pixels"] == w * h
    assert tot == 8 and scans == want_scans
    assert np.array_equal(img, want_img) and np.array_equal(mean.view(np.uint32), want_mean.view(np.uint32))


@pytest.mark.gpu
def test_python_renderer_progressive(hip):
    from spath_amd.renderer import Bitmap, HipRenderer, Viewport
    t, m = scene.closed_room(200)
    r = HipRenderer(W, H, progressive=True, seed=4)
    vp, out = Viewport(), Bitmap()
    r.get_viewport(vp)
    hip.set_scene(t, m)
    total = 0
    for n in (2, 3, 1):
        r.render(vp, t, m, len(t), n, out)
        total += n
        assert np.array_equal(out.values, hip.render(vp.rays, W, H, total, seed=4))
    r.render_flat(vp, t, m, len(t), 1, out)                                       # not accumulated, does not disturb
    r.render(vp, t, m, len(t), 2, out)
    assert np.array_equal(out.values, hip.render(vp.rays, W, H, total + 2, seed=4))
    r.set_delta_mov((0.1, 0.0, 0.0))                                             # a new viewport restarts
    r.get_viewport(vp)
    r.render(vp, t, m, len(t), 3, out)
    assert np.array_equal(out.values, hip.render(vp.rays, W, H, 3, seed=4))
    t2, m2 = scene.open_clutter(100)                                             # a new scene restarts
    hip.set_scene(t2, m2)
    r.render(vp, t2, m2, len(t2), 2, out)
    assert np.array_equal(out.values, hip.render(vp.rays, W, H, 2, seed=4))
    r.render(vp, t2, m2, len(t2), 2, out)
    assert np.array_equal(out.values, hip.render(vp.rays, W, H, 4, seed=4))
    # own viewport: keyed on the camera
    r.render_own_viewport(t2, m2, len(t2), 3, out)
    r.render_own_viewport(t2, m2, len(t2), 2, out)
    assert np.array_equal(out.values, hip.render(vp.rays, W, H, 5, seed=4))
    r.set_delta_rot((0.0, 0.2, 0.0))
    r.render_own_viewport(t2, m2, len(t2), 2, out)
    r.get_viewport(vp)
    assert np.array_equal(out.values, hip.render(vp.rays, W, H, 2, seed=4))
    r.close()
    plain = HipRenderer(W, H, seed=4)                                            # default: every call starts from nothing
    plain.render(vp, t2, m2, len(t2), 2, out)
    plain.render(vp, t2, m2, len(t2), 2, out)
    assert np.array_equal(out.values, hip.render(vp.rays, W, H, 2, seed=4))
    plain.close()


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [[], ["--device-viewport"], ["--devices", "0,0"]], ids=["rays", "device_viewport", "two_shards"])
def test_cli_progressive_writes_the_same_bytes(tmp_path, extra):
    sp = os.path.join(tmp_path, "s.bin")
    scene.write_scene(sp, *scene.closed_room(300))
    a, b = os.path.join(tmp_path, "a.rgba"), os.path.join(tmp_path, "b.rgba")
    base = [CLI, "--scene", sp, "--w", "40", "--h", "30", "--spp", "16", "--seed", "9", "--mov", "0.1", "0.2", "-0.3"] + extra
    subprocess.run(base + ["--out", a], check=True, capture_output=True, timeout=120)
    p = subprocess.run(base + ["--progressive", "3", "--out", b], check=True, capture_output=True, text=True, timeout=120)
    steps = [l for l in p.stdout.splitlines() if l.strip().startswith("step ")]
    assert len(steps) == 6 and "(16 so far)" in steps[-1] and " 1 spp" in steps[-1]
    assert open(a, "rb").read() == open(b, "rb").read()
