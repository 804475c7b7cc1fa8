"""Per-sample camera rays (include/spath_hip.h: SPHIP_FLAG_CAMERA_SAMPLES): a box-filtered position in the
pixel and, with a lens, a point on a thin lens, drawn for every (pixel, sample) inside the path-tracing kernels.

The ray is stated operation by operation in the header, so it is replayed here in numpy (f32, the draws and sincos through the
oracle's device math).  STATED TOLERANCE: 0 for the rays and for every composition (images and means bit for bit); the statistical
part compares pixel means with the coverage of an edge integrated over the pixel box and the lens disk (5 sigma plus the quadrature
error).

CPU part: the flag's value, the header, the model's geometry (every lens point of a pixel sample aims at one point in focus).
GPU part: rays bit for bit; composition with one-sample device accumulation for every shipped variant, plain, NEE and MIS; step
splits, sample chunks, multi-device contexts, adaptive accumulation; antialiasing and depth of field against quadrature; the error
contract; the CLI and the adapter."""
import os

import numpy as np
import pytest

import hip_checks as hc
from hip_checks import E_INVALID, _torch_first  # noqa: F401 (_torch_first: a fixture)
from oracle import oracle as O
from path_model import _bits, _philox
from spath_amd import capi, scene, view

F = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
VARIANTS = (1, 2, capi.FLAG_ACCEL, 15, 16)
ESTIMATORS = {"plain": 0, "nee": capi.FLAG_NEE, "mis": capi.FLAG_NEE | capi.FLAG_MIS}
CAM = capi.FLAG_CAMERA_SAMPLES


def view_consts(cam):
    """the host's ViewArgs constants (view.h:101-108, as spath_amd.view.Camera.get_viewport computes them)"""
    w, h = cam.res_x, cam.res_y
    x_size = F(np.float64(w) / np.float64(h))
    x_max = F(np.float64(x_size) / 2.0)
    x_step = x_size / F(w)
    y_max = F(np.float64(F(1.0)) / 2.0)
    y_step = F(1.0) / F(h)
    return x_max, x_step, y_max, y_step


def model_rays(cam, seed, sample, aperture=0.0, focus_dist=0.0):
    """[res_x * res_y, 6] f32: the rays of global sample `sample` as the header states them"""
    w, h = cam.res_x, cam.res_y
    n = w * h
    p = np.arange(n, dtype=np.uint32)
    i, j = (p % w).astype(F), (p // w).astype(F)
    smp = np.full(n, sample, np.uint32)
    x_max, x_step, y_max, y_step = view_consts(cam)
    r1, r2 = _philox(seed, p, smp, 24)
    cx = (x_max - x_step * i) - x_step * r1.astype(F)
    cy = (y_max - y_step * j) - y_step * r2.astype(F)
    cz = np.zeros(n, F)
    tx, ty, tz = cx + F(0), cy + F(0), cz + F(cam.focal)
    if aperture > 0:
        r3, r4 = _philox(seed, p, smp, 25)
        rho = F(aperture) * np.sqrt(r3).astype(F)
        phi = ((r4 * np.pi) * 2.0).astype(F)
        sc = O.device_math(0, phi, n).reshape(n, 2)
        ox, oy, oz = cx + rho * sc[:, 1], cy + rho * sc[:, 0], np.zeros(n, F)
        k = F(focus_dist) / F(cam.focal)
        gx, gy, gz = (cx + tx * k) - ox, (cy + ty * k) - oy, (cz + tz * k) - oz
    else:
        ox, oy, oz = cx, cy, cz
        gx, gy, gz = tx, ty, tz
    ln = np.sqrt((gx * gx + gy * gy) + gz * gz)
    dx, dy, dz = cam.rel_move(gx / ln, gy / ln, gz / ln)
    X, Y, Z = cam.rel_move(ox, oy, oz)
    out = np.stack([X + cam.pos[0], Y + cam.pos[1], Z + cam.pos[2], dx, dy, dz], axis=-1).astype(F)
    return np.ascontiguousarray(out)


def cameras():
    """default, moved + rotated, and a changed focal length; odd sizes"""
    a = view.Camera(37, 23)
    b = view.Camera(48, 32)
    b.set_delta_mov([0.3, -0.2, 0.5])
    b.set_delta_rot([0.11, -0.27, 0.0])
    c = view.Camera(21, 30, focal=1.5)
    c.set_delta_rot([-0.05, 0.4, 0.0])
    c.set_delta_mov([-0.4, 0.1, 0.2])
    return [a, b, c]


# ---------------------------------------------------------------------------------------------------------------- CPU part
def test_flag_value_and_header():
    assert capi.FLAG_CAMERA_SAMPLES == 0x1000
    assert CAM & (capi.FLAG_NEE | capi.FLAG_MIS | capi.FLAG_ACCEL | capi.FLAG_PRIMARY_REUSE | 0xFF | 0xFF0000) == 0
    hdr = open(os.path.join(ROOT, "include", "spath_hip.h")).read()
    assert "SPHIP_FLAG_CAMERA_SAMPLES = 0x1000" in hdr and "sphip_lens;" in hdr
    assert "sphip_set_lens" in capi.SYMBOLS and "sphip_camera_rays_device" in capi.SYMBOLS
    assert [f for f, _ in capi.Lens._fields_] == ["aperture", "focus_dist", "reserved"]


def test_model_focus_geometry():
    """every lens point of one pixel position aims at the pinhole ray's point at local z = focus_dist (float64 check of the
    model's algebra: the plane in focus is sharp)"""
    cam = view.Camera(16, 12)
    focus = 3.0
    sharp = model_rays(cam, 5, 0, 0.0, 0.0).astype(np.float64)
    # the same jittered positions (same seed and sample), many lens points: the ray at local z = focus is that of the pinhole ray
    for s_ap in (0.05, 0.3):
        lens = model_rays(cam, 5, 0, s_ap, focus).astype(np.float64)
        for r in (sharp, lens):
            t = (focus - (r[:, 2] - cam.pos[2])) / r[:, 5]
            r[:, :3] = r[:, :3] + r[:, 3:] * t[:, None]
        assert np.abs(lens[:, :2] - sharp[:, :2]).max() < 1e-5
    lens = model_rays(cam, 5, 0, 0.3, focus)
    assert not np.array_equal(lens[:, :3], sharp[:, :3].astype(F))        # the origins do move on the lens


# ---------------------------------------------------------------------------------------------------------------- GPU part
def _torch():
    import torch
    return torch


def _dev_rays(c, cam, seed, sample):
    torch = _torch()
    d = torch.empty(cam.res_x * cam.res_y * 6, dtype=torch.float32, device="cuda")
    c.camera_rays_device(cam, sample, d.data_ptr(), seed=seed, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return d.cpu().numpy().reshape(-1, 6)


@pytest.mark.gpu
def test_rays_bit_exact():
    c = capi.Context(0)
    for cam in cameras():
        for lens in ((0.0, 0.0), (0.04, 2.5), (0.25, 1.2)):
            c.set_lens(*lens)
            for seed, sample in ((1, 0), (0x123456789ABC, 7), (42, 123457)):
                got = _dev_rays(c, cam, seed, sample)
                want = model_rays(cam, seed, sample, *lens)
                assert np.array_equal(_bits(got), _bits(want)), (cam.res_x, lens, seed, sample)
    c.set_lens()
    cam = cameras()[1]
    assert not np.array_equal(_dev_rays(c, cam, 3, 0), _dev_rays(c, cam, 3, 1))
    c.close()


def _chain(c, cam, n, seed, flags):
    """n one-sample sphip_render_device_accum calls (sample_base = s) over sphip_camera_rays_device(s) -> (rgba, mean)"""
    torch = _torch()
    npix = cam.res_x * cam.res_y
    st = torch.cuda.current_stream().cuda_stream
    d_rays = torch.empty(npix * 6, dtype=torch.float32, device="cuda")
    d_sum = torch.zeros(npix * 3, dtype=torch.float32, device="cuda")
    d_out = torch.zeros(npix * 4, dtype=torch.uint8, device="cuda")
    d_mean = torch.zeros(npix * 3, dtype=torch.float32, device="cuda")
    for s in range(n):
        c.camera_rays_device(cam, s, d_rays.data_ptr(), seed=seed, stream=st)
        c.render_device_accum(d_rays.data_ptr(), npix, s, 1, d_sum.data_ptr(), d_out.data_ptr(), seed=seed, flags=flags,
                              image_width=cam.res_x, d_out_mean=d_mean.data_ptr(), stream=st)
    torch.cuda.synchronize()
    return d_out.cpu().numpy().reshape(-1, 4), d_mean.cpu().numpy().reshape(-1, 3)


def _cam():
    cam = view.Camera(40, 26)
    cam.set_delta_mov([0.1, 0.2, 0.3])
    cam.set_delta_rot([0.05, -0.1, 0.0])
    return cam


@pytest.mark.gpu
@pytest.mark.parametrize("est", sorted(ESTIMATORS))
@pytest.mark.parametrize("variant", VARIANTS)
def test_composition(variant, est):
    t, m = scene.closed_room(200)
    cam = _cam()
    f = variant | ESTIMATORS[est]
    c = hc.ctx(t, m)
    c.set_lens(0.06, 2.5)
    img, mean = c.render_camera(cam, 4, seed=11, flags=f | CAM, want_accum=True)
    st = c.stats()
    want_img, want_mean = _chain(c, cam, 4, 11, f)
    plain = c.render_camera(cam, 4, seed=11, flags=f, want_accum=True)[1]
    c.close()
    assert st["kernel_variant"] == (8 if variant == capi.FLAG_ACCEL else variant)
    assert np.array_equal(_bits(mean), _bits(want_mean)) and np.array_equal(img, want_img)
    assert not np.array_equal(_bits(mean), _bits(plain))


@pytest.mark.gpu
@pytest.mark.parametrize("est", ["plain", "mis"])
def test_steps_chunks_multi_device(est):
    t, m = scene.open_clutter(100)
    cam = _cam()
    f = ESTIMATORS[est] | CAM
    c = hc.ctx(t, m)
    c.set_lens(0.05, 3.0)
    one = {n: c.render_camera(cam, n, seed=4, flags=f, want_accum=True) for n in (1, 3, 6, 8)}
    for extra in (capi.flag_chunks(1), capi.flag_chunks(4), 15):
        got = c.render_camera(cam, 8, seed=4, flags=f | extra, want_accum=True)
        assert np.array_equal(got[0], one[8][0]) and np.array_equal(_bits(got[1]), _bits(one[8][1])), extra
    c.accum_begin(cam=cam, seed=4, flags=f)
    c.set_lens(0.3, 1.0)                                  # applies from the next begin: this accumulation keeps its lens
    for n in (1, 2, 3, 2):
        img, mean, tot = c.accum_step(n, want_mean=True)
        assert np.array_equal(img, one[tot][0]) and np.array_equal(_bits(mean), _bits(one[tot][1])), tot
    c.close()
    for devs in ([0, 0], [0, 0, 0]):
        mc = capi.Context.multi(devs)
        mc.set_scene(t, m)
        mc.set_lens(0.05, 3.0)
        got = mc.render_camera(cam, 8, seed=4, flags=f, want_accum=True)
        assert np.array_equal(got[0], one[8][0]) and np.array_equal(_bits(got[1]), _bits(one[8][1])), devs
        mc.accum_begin(cam=cam, seed=4, flags=f)
        for n in (3, 3):
            img, mean, tot = mc.accum_step(n, want_mean=True)
            assert np.array_equal(img, one[tot][0]) and np.array_equal(_bits(mean), _bits(one[tot][1])), (devs, tot)
        mc.close()


@pytest.mark.gpu
def test_adaptive():
    """an adaptive accumulation with camera samples: every pixel holds exactly the image of its own count, and the counts do not
    depend on the variant, the number of devices or the NEE form"""
    t, m = scene.closed_room(200)
    cam = _cam()
    counts = {}
    for variant in (16, 15, 2, 1):
        c = hc.ctx(t, m)
        c.set_lens(0.05, 3.0)
        c.accum_begin(cam=cam, seed=9, flags=variant | CAM, adaptive=(0.3, 0.05, 4))
        for n in (4, 4, 8):
            img, mean, _ = c.accum_step(n, want_mean=True)
        cnt = c.accum_counts()[0].ravel()
        counts[variant] = cnt
        for n in np.unique(cnt):
            want = c.render_camera(cam, int(n), seed=9, flags=variant | CAM, want_accum=True)
            sel = cnt == n
            assert np.array_equal(img[sel], want[0][sel]) and np.array_equal(_bits(mean[sel]), _bits(want[1][sel])), (variant, n)
        c.close()
    assert len(np.unique(counts[16])) > 1
    for v in (15, 2, 1):
        assert np.array_equal(counts[v], counts[16]), v
    mc = capi.Context.multi([0, 0])
    mc.set_scene(t, m)
    mc.set_lens(0.05, 3.0)
    mc.accum_begin(cam=cam, seed=9, flags=CAM, adaptive=(0.3, 0.05, 4))
    for n in (4, 4, 8):
        mc.accum_step(n)
    assert np.array_equal(mc.accum_counts()[0].ravel(), counts[16])
    mc.close()


# ---- meaning: one emissive triangle with zero reflectance, so a sample's radiance is Le when its primary ray hits it, else 0
EDGE_C, EDGE_M = 0.1, 0.37               # the triangle covers world x - EDGE_M * y > EDGE_C of its plane (around the view)


def edge_scene(depth):
    """one triangle in the plane world z = -3 + depth (local z = depth for the default camera), Le = 1, reflectance 0"""
    z = -3.0 + depth
    L = 60.0
    tris = np.zeros((1, 12), F)
    tris[0, 0:3] = (EDGE_C - EDGE_M * L, -L, z)
    tris[0, 3:6] = (EDGE_C + EDGE_M * L, L, z)
    tris[0, 6:9] = (EDGE_C + 40 * L, 0.0, z)
    tris = scene.flat_normals(tris)
    mats = np.array([[0, 0, 0, 1, 1, 1]], F)
    return tris, mats


def _below(A, B, T):
    """P(A u + B v < T) for u, v uniform on [0, 1), A and B nonzero (the CDF of a sum of two uniforms)"""
    T = T - np.minimum(A, 0) - np.minimum(B, 0)
    A, B = np.abs(A), np.abs(B)
    R = lambda x: np.maximum(x, 0.0) ** 2
    return np.clip((R(T) - R(T - A) - R(T - B) + R(T - A - B)) / (2 * A * B), 0.0, 1.0)


def coverage(cam, depth, aperture, focus, k):
    """per pixel, in float64: the fraction of (pixel box x lens disk) whose ray hits the edge scene; the lens by a k x k midpoint
    rule in (r3, r4), the pixel box exactly.  A ray from o = cur + l (l on the lens) through the point in focus F = cur (1 + k) +
    (0, 0, focus), k = focus / focal, meets local z = depth at cur (1 + depth / focal) + l (1 - depth / focus)"""
    w, h = cam.res_x, cam.res_y
    x_max, x_step, y_max, y_step = [np.float64(v) for v in view_consts(cam)]
    f = np.float64(cam.focal)
    al = 1.0 + depth / f
    be = (1.0 - depth / focus) if aperture > 0 else 0.0
    p = np.arange(w * h)
    X0 = x_max - x_step * (p % w)
    Y0 = y_max - y_step * (p // w)
    # hit <=> (X - EDGE_M Y) > EDGE_C with X = al (X0 - x_step u) + be lx, Y = al (Y0 - y_step v) + be ly
    #     <=> al x_step u - al EDGE_M y_step v < al (X0 - EDGE_M Y0) + be (lx - EDGE_M ly) - EDGE_C
    A = al * x_step
    B = -al * EDGE_M * y_step
    q = (np.arange(k) + 0.5) / k
    r3, r4 = np.meshgrid(q, q, indexing="ij")
    rho = aperture * np.sqrt(r3.ravel())
    phi = 2 * np.pi * r4.ravel()
    lt = be * (rho * np.cos(phi) - EDGE_M * rho * np.sin(phi))           # [lens points]
    T = (al * (X0 - EDGE_M * Y0) - EDGE_C)[:, None] + lt[None, :]
    return _below(A, B, T).mean(axis=1)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["pinhole", "in_focus", "defocused"])
def test_meaning(case):
    depth = 2.0
    aperture, focus = {"pinhole": (0.0, 0.0), "in_focus": (0.12, depth), "defocused": (0.12, 6.0)}[case]
    cam = view.Camera(32, 24)
    t, m = edge_scene(depth)
    N = 2048
    c = hc.ctx(t, m)
    c.set_lens(aperture, focus)
    plain = c.render_camera(cam, 16, seed=2, want_accum=True)[1][:, 0]
    mean = c.render_camera(cam, N, seed=2, flags=CAM, want_accum=True)[1][:, 0].astype(np.float64)
    c.close()
    assert np.all((plain == 0) | (plain == 1))                           # without the flag: 0 or Le
    mid = (mean > 0) & (mean < 1)
    assert mid.sum() >= 20, mid.sum()                                    # the edge pixels take intermediate values
    cov = coverage(cam, depth, aperture, focus, 96)
    qerr = np.abs(cov - coverage(cam, depth, aperture, focus, 48)) + 1e-6
    pe = np.clip(cov, 1.0 / N, 1 - 1.0 / N)
    sig = np.sqrt(pe * (1 - pe) / N)
    z = np.abs(mean - cov) / (sig + qerr / 5)
    assert z.max() <= 5.0, (z.max(), np.argmax(z), mean[np.argmax(z)], cov[np.argmax(z)])
    partial = ((cov > 0.01) & (cov < 0.99)).sum()
    if case == "defocused":                                              # a wider transition than the sharp edge
        sharp = coverage(cam, depth, 0.0, 0.0, 1)
        assert partial > 1.5 * ((sharp > 0.01) & (sharp < 0.99)).sum()
    if case == "in_focus":                                               # in focus: the lens does not matter
        assert np.abs(cov - coverage(cam, depth, 0.0, 0.0, 1)).max() < 1e-9


@pytest.mark.gpu
def test_error_contract():
    torch = _torch()
    t, m = scene.closed_room(200)
    cam = _cam()
    n = cam.res_x * cam.res_y
    rays = view.Camera(cam.res_x, cam.res_y).get_viewport()
    c = hc.ctx(t, m)
    with pytest.raises(RuntimeError, match=E_INVALID):                   # paths that take rays
        c.render(rays, cam.res_x, cam.res_y, 2, seed=1, flags=CAM)
    with pytest.raises(RuntimeError, match=E_INVALID):
        c.accum_begin(rays=rays, w=cam.res_x, h=cam.res_y, seed=1, flags=CAM)
    with pytest.raises(RuntimeError, match=E_INVALID):
        c.accum_begin(rays=rays, w=cam.res_x, h=cam.res_y, seed=1, flags=CAM, adaptive=(0.3, 0.05, 4))
    d_rays = torch.from_numpy(rays).cuda()
    d_out = torch.zeros(n * 4, dtype=torch.uint8, device="cuda")
    d_sum = torch.zeros(n * 3, dtype=torch.float32, device="cuda")
    with pytest.raises(RuntimeError, match=E_INVALID):
        c.render_device(d_rays.data_ptr(), n, 2, d_out.data_ptr(), seed=1, flags=CAM)
    with pytest.raises(RuntimeError, match=E_INVALID):
        c.render_device_accum(d_rays.data_ptr(), n, 0, 2, d_sum.data_ptr(), d_out.data_ptr(), seed=1, flags=CAM)
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match=E_INVALID):                   # with primary-hit reuse
        c.render_camera(cam, 2, seed=1, flags=CAM | capi.FLAG_PRIMARY_REUSE)
    with pytest.raises(RuntimeError, match=E_INVALID):
        c.accum_begin(cam=cam, seed=1, flags=CAM | capi.FLAG_PRIMARY_REUSE)
    for v in (3, 9):                                                     # other variants
        with pytest.raises(RuntimeError, match=E_INVALID):
            c.render_camera(cam, 2, seed=1, flags=CAM | v)
    for bad in ((-0.1, 2.0), (np.nan, 2.0), (np.inf, 2.0), (0.1, 0.0), (0.1, -1.0), (0.1, np.nan), (0.1, np.inf)):
        with pytest.raises(RuntimeError, match=E_INVALID):
            c.set_lens(*bad)
    with pytest.raises(RuntimeError, match=E_INVALID):
        c.set_lens(0.1, 2.0, reserved=1)
    c.set_lens(0.0, np.nan)                                              # aperture 0: the focus distance is not used
    c.set_lens(0.1, 2.0)
    # flat mode ignores the flag; the G-buffer stays that of the pixel-centre rays
    flat0 = c.render_camera(cam, 1, mode=capi.MODE_FLAT)
    flat1 = c.render_camera(cam, 1, mode=capi.MODE_FLAT, flags=CAM)
    assert np.array_equal(flat0, flat1)
    c.accum_begin(cam=cam, seed=1)
    c.accum_step(2)
    g0 = c.accum_gbuffer()
    c.accum_begin(cam=cam, seed=1, flags=CAM)
    c.accum_step(2)
    g1 = c.accum_gbuffer()
    assert g0.tobytes() == g1.tobytes()
    # scans_executed keeps its meaning: the path scans (no pre-pass, no extra scans for the rays)
    c.render_camera(cam, 3, seed=1, flags=1)
    s_plain = c.stats()["scans_executed"]
    c.render_camera(cam, 3, seed=1, flags=1 | CAM)
    s_cam = c.stats()["scans_executed"]
    assert n * 3 <= s_cam <= n * 3 * 5 and n * 3 <= s_plain <= n * 3 * 5
    c.close()
    mc = capi.Context.multi([0, 0])
    mc.set_scene(t, m)
    with pytest.raises(RuntimeError, match=r"\[-3\]"):                   # device pointers: single-device contexts only
        mc.camera_rays_device(cam, 0, d_rays.data_ptr())
    with pytest.raises(RuntimeError, match=E_INVALID):
        mc.render(rays, cam.res_x, cam.res_y, 2, seed=1, flags=CAM)
    mc.close()


@pytest.mark.gpu
def test_cli_and_adapter(tmp_path):
    """spath_cli --aa / --lens A,F go through hip_renderer::set_camera_samples / set_lens on the camera path and give the capi image,
    one-shot and progressive; malformed lens values are refused"""
    import subprocess
    cli = os.path.join(ROOT, "spath_amd", "host", "build", "spath_cli")
    t, m = scene.open_clutter(100)
    sp = str(tmp_path / "s.bin")
    scene.write_scene(sp, t, m)
    w, h = 40, 24
    cam = view.Camera(w, h)
    c = hc.ctx(t, m)
    aa = c.render_camera(cam, 8, seed=9, flags=CAM)
    c.set_lens(0.05, 2.5)
    dof = c.render_camera(cam, 8, seed=9, flags=CAM)
    dof_mis = c.render_camera(cam, 8, seed=9, flags=CAM | capi.FLAG_NEE | capi.FLAG_MIS)
    plain = c.render_camera(cam, 8, seed=9)
    c.close()
    assert len({aa.tobytes(), dof.tobytes(), plain.tobytes()}) == 3
    base = [cli, "--scene", sp, "--w", str(w), "--h", str(h), "--spp", "8", "--seed", "9"]
    for extra, want in ((["--aa"], aa), (["--lens", "0.05,2.5"], dof), (["--aa", "--lens", "0.05,2.5", "--progressive", "3"], dof),
                        (["--lens", "0.05,2.5", "--mis"], dof_mis), ([], plain)):
        out = str(tmp_path / "o.rgba")
        subprocess.run(base + ["--out", out] + extra, check=True, capture_output=True, timeout=120)
        assert open(out, "rb").read() == want.tobytes(), extra
    for bad in ("0.05", "-0.1,2", "0.1,0", "0.1,-2", "a,b", "0.1,2x", "nan,2"):
        r = subprocess.run(base + ["--out", str(tmp_path / "x.rgba"), "--lens", bad], capture_output=True, timeout=120)
        assert r.returncode != 0, bad
