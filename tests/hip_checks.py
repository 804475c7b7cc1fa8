"""What the estimator tests share on the GPU side (tests/test_hip_nee.py, test_hip_mis.py, test_hip_specular.py, test_hip_smooth.py,
test_hip_dielectric.py, test_hip_environment.py, test_hip_glossy.py; the helpers also serve test_hip_camera_samples.py,
test_hip_adaptive.py, test_hip_progressive.py and test_hip_denoise.py): the rays, the contexts and their flags, the scenes the
replay (tests/path_model.py) is held to, the two fixtures, and one check per composition of an estimator flag with the rest of the
library.  A check takes a context with the feature's tables installed and the flag word; the test picks the scene and the flags,
closes the context and keeps the asserts that are its own.

Not a test module."""
import ctypes as C
import os

import numpy as np
import pytest

from path_model import F, _bits
from spath_amd import capi, scene, view

W, H, SPP = 48, 32, 4
REPLAY_SEED = 3
E_INVALID, E_STATE = r"\[-1\]", r"\[-3\]"
NEE_MIS = capi.FLAG_NEE | capi.FLAG_MIS
ESTIMATORS = {"plain": 0, "mis": NEE_MIS}        # the estimators that take a specular table or vertex normals, by path_model's names
MOVES = ((0.1, -0.2, 0.3), (0.05, 0.1, 0.0))


# ---------------------------------------------------------------------------------------------------------------- helpers
def cam_rays(w=W, h=H, moves=MOVES):
    """-> (camera after one move and one turn, its viewport's rays)"""
    cam = view.Camera(w, h)
    cam.set_delta_mov(moves[0])
    cam.set_delta_rot(moves[1])
    return cam, np.ascontiguousarray(cam.get_viewport(), dtype=F)


def rays(w=W, h=H, moves=MOVES):
    return cam_rays(w, h, moves)[1]


def ctx(t, m, spec=None, vn=None, devs=None, glass=None, env=None, rough=None):
    """a context (a multi-device one over devs) with the scene, the tables and the map given"""
    c = capi.Context(0) if devs is None else capi.Context.multi(devs)
    c.set_scene(t, m)
    for table, setter in ((spec, c.set_specular), (vn, c.set_vertex_normals), (glass, c.set_dielectric), (env, c.set_environment),
                          (rough, c.set_roughness)):
        if table is not None:
            setter(table)
    return c


def table_flags(spec=None, vn=None, glass=None, env=None, rough=None):
    """the flags that turn on the steps of the tables and the map given"""
    return sum(flag for table, flag in ((spec, capi.FLAG_SPECULAR), (vn, capi.FLAG_SMOOTH), (glass, capi.FLAG_DIELECTRIC),
                                        (env, capi.FLAG_ENVIRONMENT), (rough, capi.FLAG_GLOSSY)) if table is not None)


def same(a, b):
    """(image, mean) pairs equal bit for bit"""
    return np.array_equal(a[0], b[0]) and np.array_equal(_bits(a[1]), _bits(b[1]))


def seeds_means(c, rays, w, h, spp, flags, seeds):
    return np.stack([c.render(rays, w, h, spp, seed=s, flags=flags, want_accum=True)[1].astype(np.float64) for s in seeds])


def z_grid(a, b, h, w, tag, alike_is_zero=False):
    """the project's criterion for two estimators of one image: over 16 seeds, |z| < 4 for the difference of the image means and < 5 in
    every cell of a 4 x 4 grid.  alike_is_zero: a cell both render alike in every seed (nothing in view) has no difference, z = 0"""
    dd = a.reshape(16, h, w, 3).sum(-1) - b.reshape(16, h, w, 3).sum(-1)

    def z(x):
        v = x.reshape(16, -1).mean(1)
        if alike_is_zero and not v.any():
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


def _tiles(c):
    """(tiles, triangles per tile) of the stream the context built: which shape of the default scan really ran"""
    t = C.c_uint32(0)
    c._check(c._L.sphip_selftest_stage1(c._h, None, 0, None, None, None, C.byref(t)), "sphip_selftest_stage1")
    return t.value & 0xFFFFF, (t.value >> 20) & 0x7FF            # (bit 31: octet bits)


def set_device_table(setter, table):
    """a table through the device-pointer form of its setter, which copies it"""
    import torch
    st = torch.cuda.current_stream().cuda_stream
    d = torch.from_numpy(table).to("cuda")
    setter(d.data_ptr(), st)
    torch.cuda.synchronize()


@pytest.fixture(autouse=True, scope="module")
def _torch_first():
    """torch's device runtime is brought up before the library's first context, as conftest.py's hip fixture does"""
    import torch
    torch.cuda.is_available()


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


# ---------------------------------------------------------------------------------------------------------------- scenes
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


def mirror_floor():
    """the default scene with its two floor triangles pure mirrors"""
    t, m = scene.default_scene()
    s = np.zeros((t.shape[0], 4), F)
    s[1:3] = (0.9, 0.8, 0.7, 1.0)
    return t, m, s


def mixed_table(t, m, s=None):
    """a mixed specular table, p in (0.2, 0.8) and ks by a fixed pattern over the index: over every triangle, or on top of s over the
    non-emitters that s leaves diffuse"""
    j = np.arange(t.shape[0], dtype=F)
    x = np.zeros((t.shape[0], 4), F) if s is None else s.copy()
    k = np.ones(t.shape[0], bool) if s is None else (m[:, 3:6].sum(1) == 0) & (s[:, 3] == 0)
    x[k, 0] = (F(0.3) + F(0.1) * (j % 5))[k]
    x[k, 1] = (F(0.2) + F(0.15) * (j % 4))[k]
    x[k, 2] = (F(0.5) + F(0.05) * (j % 7))[k]
    x[k, 3] = (F(0.2) + F(0.1) * (j % 7))[k]
    return x


def mixed_room():
    """closed_room(200) with every triangle mixed"""
    t, m = scene.closed_room(200)
    return t, m, mixed_table(t, m)


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


def hand_scene():
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
    r = np.array([[-1, 1, 0, a, -a, 0],           # reflects at the origin into (a, a, 0): reaches the emitter at (2, 2, 0)
                  [1, 1, 0, -a, -a, 0],           # reflects into (-a, a, 0): the black triangle at (-2, 2, 0), then out
                  [0, 1, 0, 0, -1, 0]], F)        # reflects straight up: nothing there
    return t, m, s, r


SPHERE_C, SPHERE_R = (0.0, -0.35, -0.9), 0.5


def sphere_scene(mirror):
    """default_scene plus icosphere(1) (80 triangles) in front of the pyramid, under the light: a pure mirror or diffuse"""
    t0, m0 = scene.default_scene()
    ts, ms = scene.icosphere(1, SPHERE_C, SPHERE_R, (0.1, 0.1, 0.1, 0, 0, 0) if mirror else (0.8, 0.7, 0.6, 0, 0, 0))
    t, m = np.concatenate([t0, ts]), np.concatenate([m0, ms])
    s = np.zeros((t.shape[0], 4), F)
    if mirror:
        s[7:] = (0.9, 0.85, 0.8, 1.0)
    vn = scene.vertex_normals(t, which=np.arange(7, t.shape[0]))
    return t, m, s, vn


def bad_room():
    """closed_room(200) with vertex_normals over everything at crease_deg = 180: the box's corners average three walls, which gives
    deliberately bad normals and so many terminations"""
    t, m = scene.closed_room(200)
    return t, m, np.zeros((t.shape[0], 4), F), scene.vertex_normals(t, 180.0)


NEE_SCENES = {"closed_room_200": lambda: scene.closed_room(200), "open_clutter_100": lambda: scene.open_clutter(100),
              "many_emitters": many_emitters}
SPECULAR_SCENES = {"mirror_floor": mirror_floor, "mixed_room": mixed_room, "facing_mirrors": facing_mirrors}
SMOOTH_SCENES = {"mirror_sphere": lambda: sphere_scene(True), "diffuse_sphere": lambda: sphere_scene(False), "bad_room": bad_room}


def smooth_case(name, mixed):
    t, m, s, vn = SMOOTH_SCENES[name]()
    return t, m, (mixed_table(t, m, s) if mixed else s), vn


# ---------------------------------------------------------------------------------------------------------------- checks
def check_progressive_adaptive_denoise(c, f):
    """every step of an accumulation is the one-shot render of its total; under an adaptive rule every pixel is the one-shot render of
    its own count; denoising repeats.  -> the pixels' counts; the accumulation is still open"""
    r = rays()
    one = {n: c.render(r, W, H, n, seed=9, flags=f, want_accum=True) for n in (3, 8, 16)}
    c.accum_begin(rays=r, w=W, h=H, seed=9, flags=f)
    for n in (3, 5, 8):
        img, mean, tot = c.accum_step(n, want_mean=True)
        assert same((img, mean), one[tot]), tot
    c.accum_begin(rays=r, w=W, h=H, seed=9, flags=f, adaptive=(0.3, 0.05, 4))
    for n in (4, 4, 8):
        img, mean, _ = c.accum_step(n, want_mean=True)
    cnt = c.accum_counts()[0].ravel()
    for n in np.unique(cnt):
        want = one.get(int(n)) or c.render(r, W, H, int(n), seed=9, flags=f, want_accum=True)
        sel = cnt == n
        assert same((img[sel], mean[sel]), (want[0][sel], want[1][sel])), n
    den0, den1 = c.accum_denoise(), c.accum_denoise()
    assert den0.shape == (W * H, 4) and np.array_equal(den0, den1)
    return cnt


def check_reuse_chunks_multi_device(t, m, f, extras, spec=None, vn=None, unflag=0, each_multi=None):
    """primary-hit reuse, sample chunks, the variants in `extras`, and multi-device contexts (one-shot and in two steps) give the
    single context's render; without the bits `unflag` the image is another.  each_multi(mc): the test's own asserts on each
    multi-device context after its accumulation"""
    r = rays()
    c = ctx(t, m, spec, vn)
    want = c.render(r, W, H, SPP, seed=4, flags=f, want_accum=True)
    if unflag:
        assert not same(want, c.render(r, W, H, SPP, seed=4, flags=f & ~unflag, want_accum=True))
    for extra in (capi.FLAG_PRIMARY_REUSE, capi.flag_chunks(1), capi.flag_chunks(4)) + tuple(extras):
        assert same(c.render(r, W, H, SPP, seed=4, flags=f | extra, want_accum=True), want), extra
    c.close()
    for devs in ([0, 0], [0, 0, 0]):
        mc = ctx(t, m, spec, vn, devs)
        got = mc.render(r, W, H, SPP, seed=4, flags=f, want_accum=True)
        mc.accum_begin(rays=r, w=W, h=H, seed=4, flags=f)
        mc.accum_step(1)
        img, mean, _ = mc.accum_step(SPP - 1, want_mean=True)
        if each_multi:
            each_multi(mc)
        mc.close()
        assert same(got, want), devs
        assert same((img, mean), want), devs


def check_camera_samples(c, f):
    """camera samples with the flags f are the chain of one-sample accumulations over sphip_camera_rays_device's rays (as
    tests/test_hip_camera_samples.py composes them)"""
    import torch
    cam = view.Camera(40, 26)
    cam.set_delta_mov([0.1, 0.2, 0.3])
    cam.set_delta_rot([0.05, -0.1, 0.0])
    st = torch.cuda.current_stream().cuda_stream
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
    assert same((img, mean), (d_out.cpu().numpy().reshape(-1, 4), d_mean.cpu().numpy().reshape(-1, 3)))


def _check_camera_renders_alike(c, cam, f, flag):
    """camera renders with and without `flag` are alike bit for bit, scans included, with and without camera samples"""
    for extra in (0, capi.FLAG_CAMERA_SAMPLES):
        want = c.render_camera(cam, SPP, seed=6, flags=f | extra, want_accum=True)
        ws = c.stats()["scans_executed"]
        got = c.render_camera(cam, SPP, seed=6, flags=f | extra | flag, want_accum=True)
        assert same(got, want) and c.stats()["scans_executed"] == ws, extra


def check_zero_table_is_no_flag(c, f, flag):
    """c holds a table that changes nothing: the render with `flag` is the one without, bit for bit, scans included, from rays and,
    with and without camera samples, from a camera"""
    r = rays()
    cam = view.Camera(40, 26)
    cam.set_delta_mov([0.1, 0.2, 0.3])
    c.set_lens(0.05, 2.5)
    want = c.render(r, W, H, SPP, seed=6, flags=f, want_accum=True)
    ws = c.stats()["scans_executed"]
    got = c.render(r, W, H, SPP, seed=6, flags=f | flag, want_accum=True)
    assert same(got, want) and c.stats()["scans_executed"] == ws
    _check_camera_renders_alike(c, cam, f, flag)


def check_accel_parity(c, f):
    """the BVH gives variant 16's image up to its rare rounding-noise accepts (test_hip_accel.py's rule: at least 99 % of the pixels
    equal).  -> the BVH's mean; the context's stats are those of the BVH render"""
    r = rays()
    a = c.render(r, W, H, SPP, seed=3, flags=f | 16, want_accum=True)[1]
    b = c.render(r, W, H, SPP, seed=3, flags=f | capi.FLAG_ACCEL, want_accum=True)[1]
    share = np.all(_bits(a) == _bits(b), axis=1).mean()
    print("BVH agrees with variant 16 in", share, "of the pixels")
    assert share >= 0.99, share
    return b


def check_both_block_shapes(c, shape, f, flag, want, zero):
    """variant 16 in the forced shape: the replay `want` = (image, mean, scans) under f | flag, primary-hit reuse, a progressive and
    an adaptive split and camera samples against it, and, after zero(c) has installed a table that changes nothing, zero table = no
    flag; the tile size of the stream says which shape ran"""
    r = rays()
    got = c.render(r, W, H, SPP, seed=REPLAY_SEED, flags=f | flag, want_accum=True)
    st = c.stats()
    assert _tiles(c)[1] == shape and st["kernel_variant"] == 16
    assert same(got, want[:2]) and st["scans_executed"] == want[2]
    assert same(c.render(r, W, H, SPP, seed=REPLAY_SEED, flags=f | flag | capi.FLAG_PRIMARY_REUSE, want_accum=True), got)
    for adaptive in (None, (0.0, 0.0, 0xFFFFFFFF)):                # a rule that never stops a pixel
        c.accum_begin(rays=r, w=W, h=H, seed=REPLAY_SEED, flags=f | flag, adaptive=adaptive)
        c.accum_step(1)
        img, mean, _ = c.accum_step(SPP - 1, want_mean=True)
        assert same((img, mean), got), adaptive
    cam = view.Camera(40, 26)
    cam.set_delta_mov([0.1, 0.2, 0.3])
    ca = c.render_camera(cam, SPP, seed=6, flags=f | flag | capi.FLAG_CAMERA_SAMPLES, want_accum=True)
    c.accum_begin(cam=cam, seed=6, flags=f | flag | capi.FLAG_CAMERA_SAMPLES)
    c.accum_step(2)
    img, mean, _ = c.accum_step(SPP - 2, want_mean=True)
    assert same((img, mean), ca)
    zero(c)
    _check_camera_renders_alike(c, cam, f, flag)
    assert _tiles(c)[1] == shape
