"""The display transform on the GPU (include/spath_hip.h "display transform"): k_lum_histogram and k_display
against tests/display_model.py with STATED TOLERANCE 0 (counts equal, RGBA8 equal, floats equal bit for bit; a NaN equals a NaN), the
identity that anchors the transform to the renders' resolve, sphip_accum_display against its stateless composition, what the calls
leave alone, their refusals and extents, and the point of the feature: an auto-exposed image does not change with the light's power."""
import ctypes as C

import numpy as np
import pytest

import display_model as D
import hip_checks as hc
from hip_checks import _torch_first  # noqa: F401  (fixture)
from spath_amd import capi, scene
from test_hip_extents import held

pytestmark = pytest.mark.gpu

F = np.float32
SIZES = {1: (1, 1), 63: (9, 7), 1040: (40, 26)}          # 40 x 26: no multiple of a quad, a wave or a workgroup
FLAT = 256 * 256                                          # a constant image: every lane of every wave in one bin
CURVES = (D.CLAMP, D.REINHARD, D.FILMIC)
ENCODES = (D.LINEAR, D.SRGB)
BIG = np.finfo(F).max


@pytest.fixture(scope="module")
def T():
    return capi.srgb_thresholds()


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def sync():
    import torch
    torch.cuda.synchronize()


def same_floats(a, b):
    """bit for bit, a NaN equal to any NaN (the host's default NaN and the device's differ in the sign bit)"""
    a, b = np.asarray(a, F), np.asarray(b, F)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


def gpu_histogram(c, img, offset=0):
    import torch
    img = np.asarray(img, F).reshape(-1, 3)
    buf = torch.zeros(img.size + offset, dtype=torch.float32, device="cuda")
    buf[offset:] = dev(img.ravel())
    d_hist = torch.full((D.BINS,), 0xABCD, dtype=torch.int32, device="cuda")          # the call zeroes it
    c.luminance_histogram_device(img.shape[0], buf.data_ptr() + 4 * offset, d_hist.data_ptr(), stream())
    sync()
    return d_hist.cpu().numpy().view(np.uint32)


def gpu_display(c, img, params, want_rgb=True, offset=0):
    """offset: floats / pixels by which every buffer is moved off its 16-byte alignment"""
    import torch
    img = np.asarray(img, F).reshape(-1, 3)
    n = img.shape[0]
    buf = torch.zeros(img.size + offset, dtype=torch.float32, device="cuda")
    buf[offset:] = dev(img.ravel())
    d_rgba = torch.zeros(n + offset, dtype=torch.int32, device="cuda")
    d_rgb = torch.zeros(n * 3 + offset, dtype=torch.float32, device="cuda")
    c.display_device(n, buf.data_ptr() + 4 * offset, d_rgba.data_ptr() + 4 * offset, d_out_rgb=(d_rgb.data_ptr() + 4 * offset) if want_rgb else 0,
                     params=params, stream=stream())
    sync()
    rgba = d_rgba[offset:].cpu().numpy().view(np.uint8).reshape(n, 4)
    return rgba, (d_rgb[offset:].cpu().numpy().reshape(n, 3) if want_rgb else None)


def edge_pixels():
    """green-only pixels whose luminance is exactly a bin edge, one ulp below it and one above, for a few edges"""
    rows = []
    for b in (9, 1000, 1016, 1017, 2033):
        edge = np.array([b << 20], np.uint32).view(F)[0]
        g0 = F(np.float64(edge) / np.float64(F(0.7152)))
        cand = g0.view(np.uint32) + np.arange(-8, 9)
        cand = cand.astype(np.uint32).view(F)
        px = np.zeros((cand.size, 3), F)
        px[:, 1] = cand
        lb = D.lum(px).view(np.uint32)
        for want in (edge.view(np.uint32) - 1, edge.view(np.uint32), edge.view(np.uint32) + 1):
            hit = np.nonzero(lb == want)[0]
            assert hit.size, (b, want)
            rows.append(px[hit[0]])
    return np.array(rows, F)


def specials(T):
    den = F(5e-39)                                                      # a denormal of bin 3; the smallest ones share bin 0
    rows = [[0, 0, 0], [-0.0, -0.0, -0.0], [-1, -2, -3], [-1, 5, 0.25], [np.nan, 1, 1], [1, np.nan, 0.5], [np.inf, 0, 0], [np.inf, np.inf, np.inf],
            [-np.inf, 1, 1], [den, den, den], [0, F(1.4e-45), 0], [0, 8e-39, 0], [BIG, BIG, BIG], [BIG, 0, 0], [0, 0, BIG], [1, 1, 1], [4, 4, 4], [5, 4.5, 100],
            [1e10, 1e10, 1e10], [1e30, 1e30, 1e30], [0.18, 0.18, 0.18], [1e-6, 2e-6, 3e-6]]
    below = np.nextafter(T, F(-np.inf))
    tt = np.concatenate([T, below, F([0, 1, np.nextafter(F(1), F(2))])])          # 513 values: 171 pixels
    return np.concatenate([np.asarray(rows, F), tt.reshape(-1, 3), edge_pixels()])


def image(n, T, seed=0, with_specials=True):
    rng = np.random.default_rng(seed)
    img = F(2.0 ** rng.uniform(-14, 7, (n, 3)))
    if with_specials:
        s = specials(T)
        k = min(n, s.shape[0])
        img[:k] = s[:k]
    return img


# ---------------------------------------------------------------------------------------------------------------- histogram
@pytest.mark.parametrize("n", sorted(SIZES))
def test_histogram_equals_the_model(ctx, T, n):
    for seed, sp in ((0, True), (1, False)):
        img = image(n, T, seed, sp)
        got = gpu_histogram(ctx, img)
        assert np.array_equal(got, D.histogram(img)), n
        assert int(got.sum()) == n


def test_histogram_of_a_constant_image(ctx):
    for value in ((0.5, 0.25, 2.0), (0, 0, 0), (np.nan, 0, 0)):
        img = np.tile(F(value), (FLAT, 1))
        got = gpu_histogram(ctx, img)
        b = int(D.bins(img[:1])[0])
        assert got[b] == FLAT and int(got.sum()) == FLAT, value
    # two and five levels in stripes and interleaved: the aggregation rounds and the plain adds both run
    for levels in (2, 5, 9):
        img = np.tile(F(2.0) ** np.arange(levels, dtype=F)[:, None], (1, 3))[np.arange(FLAT) % levels]
        assert np.array_equal(gpu_histogram(ctx, img), D.histogram(img)), levels


def test_histogram_of_mixed_values(ctx, T):
    img = np.concatenate([specials(T), image(1040, T, 2, False)])
    h = D.histogram(img)
    assert h[0] >= 6 and h[2040] >= 2 and h[1:8].sum() >= 2 and h[2039] + h[2040] >= 3       # what the image is for
    got = gpu_histogram(ctx, img)
    assert np.array_equal(got, h)
    assert int(got.sum()) == img.shape[0]
    # an image that is not 16-byte aligned takes the scalar loads: the same counts
    assert np.array_equal(gpu_histogram(ctx, img, offset=1), h)
    assert np.array_equal(gpu_histogram(ctx, img[:63], offset=3), D.histogram(img[:63]))


# ---------------------------------------------------------------------------------------------------------------- transform
@pytest.mark.parametrize("n", sorted(SIZES) + [FLAT])
def test_transform_equals_the_model(ctx, T, n):
    img = image(n, T, 3) if n != FLAT else np.concatenate([specials(T), np.tile(F((0.3, 0.6, 1.7)), (FLAT - specials(T).shape[0], 1))])
    for curve in CURVES:
        for enc in ENCODES:
            for E, white in ((1.0, 4.0), (0.37, 1.5), (6.5, 100.0)):
                p = {"exposure": E, "white": white, "curve": curve, "encode": enc}
                rgba, rgb = gpu_display(ctx, img, p)
                want_rgba, want_rgb = D.display(img, T, E, white, curve, enc)
                assert np.array_equal(rgba, want_rgba), (n, p)
                assert same_floats(rgb, want_rgb), (n, p)
                assert np.array_equal(gpu_display(ctx, img, p, want_rgb=False)[0], want_rgba), (n, p)


def test_transform_with_unaligned_buffers(ctx, T):
    img = image(1040, T, 4)
    for off in (1, 2, 3):
        for enc in ENCODES:
            p = {"exposure": 0.9, "white": 2.0, "curve": D.REINHARD, "encode": enc}
            rgba, rgb = gpu_display(ctx, img, p, offset=off)
            want_rgba, want_rgb = D.display(img, T, 0.9, 2.0, D.REINHARD, enc)
            assert np.array_equal(rgba, want_rgba) and same_floats(rgb, want_rgb), (off, enc)


def test_every_threshold_and_the_float_below_it(ctx, T):
    """with E = 1 and the clamp curve the table's own values reach the search: T[k] encodes as k, the float below as k - 1"""
    below = np.nextafter(T, F(-np.inf))
    img = np.stack([T, below, np.full(255, np.nan, F)], axis=1)
    rgba, _ = gpu_display(ctx, img, {"exposure": 1.0, "curve": D.CLAMP, "encode": D.SRGB})
    k = np.arange(1, 256)
    assert np.array_equal(rgba[:, 0], k) and np.array_equal(rgba[:, 1], k - 1) and not rgba[:, 2].any() and not rgba[:, 3].any()


# ---------------------------------------------------------------------------------------------------------------- accumulations
W, H = SIZES[1040]
IDENTITY = {"exposure": 1.0, "white": 4.0, "curve": D.CLAMP, "encode": D.LINEAR}
ADAPTIVE = (0.3, 0.05, 4)


@pytest.fixture(scope="module")
def room():
    t, m = scene.closed_room(200)
    c = hc.ctx(t, m)
    yield c
    c.close()


def begin(c, kind, seed=3):
    """-> the (image, mean) of the step that follows the begin; kind: plain, adaptive (some pixels stopped) or reprojected"""
    cam, _ = hc.cam_rays(W, H)
    if kind == "adaptive":
        c.accum_begin(cam=cam, seed=seed, adaptive=ADAPTIVE)
        c.accum_step(4)
        img, mean, _ = c.accum_step(4, want_mean=True)
        counts, active = c.accum_counts()
        assert 0 < active < W * H, "the rule is to have stopped some pixels and not all"
        return img, mean
    c.accum_begin(cam=cam, seed=seed)
    img, mean, _ = c.accum_step(3, want_mean=True)
    if kind == "reprojected":
        cam2, _ = hc.cam_rays(W, H, ((0.12, -0.2, 0.28), (0.05, 0.1, 0.0)))
        c.accum_reproject(cam2, seed + 100)
        img, mean, _ = c.accum_step(2, want_mean=True)
        assert c.accum_history().max() > 0
    else:
        assert kind == "plain"
    return img, mean


@pytest.mark.parametrize("kind", ["plain", "adaptive", "reprojected"])
def test_identity_settings_give_the_steps_own_pixels(room, kind):
    img, mean = begin(room, kind)
    rgba, _ = gpu_display(room, mean, IDENTITY)
    assert np.array_equal(rgba, img)
    got, rgb, e = room.accum_display(IDENTITY, want_rgb=True)
    assert np.array_equal(got, img) and e == 1.0
    assert same_floats(rgb, D.clamp01(mean))


def stateless(c, image_f, p, m):
    """histogram -> exposure -> display on device pointers -> (rgba, rgb, exposure)"""
    import torch
    d = dict(p)
    if m is not None:
        d_hist = torch.zeros(D.BINS, dtype=torch.int32, device="cuda")
        d_img = dev(image_f)
        c.luminance_histogram_device(image_f.shape[0], d_img.data_ptr(), d_hist.data_ptr(), stream())
        sync()
        d["exposure"] = capi.exposure_from_histogram(d_hist.cpu().numpy().view(np.uint32), m)
    rgba, rgb = gpu_display(c, image_f, d)
    return rgba, rgb, capi.Display.make(d).exposure


def denoised_stateless(c, mean, params):
    """sphip_denoise_device on the mean with the accumulation's G-buffer, no variance (a plain or reprojected accumulation)"""
    import torch
    g = dev(c.accum_gbuffer().view(np.uint8))
    d_mean = dev(mean)
    d_rgba = torch.zeros(W * H, dtype=torch.int32, device="cuda")
    d_rgb = torch.zeros(W * H * 3, dtype=torch.float32, device="cuda")
    c.denoise_device(W, H, d_mean.data_ptr(), g.data_ptr(), d_rgba.data_ptr(), d_out_rgb=d_rgb.data_ptr(), params=params, stream=stream())
    sync()
    return d_rgb.cpu().numpy().reshape(-1, 3)


@pytest.mark.parametrize("kind", ["plain", "adaptive", "reprojected"])
def test_stateful_equals_stateless(room, kind):
    _, mean = begin(room, kind)
    dn = {"iterations": 2}
    for denoise in (None, dn):
        if denoise is None:
            src = mean
        elif kind == "adaptive":                       # the variance-guided filter: sphip_accum_denoise's own float output
            src = room.accum_denoise(dn, want_rgb=True)[1]
        else:
            src = denoised_stateless(room, mean, dn)
        for p in ({}, {"curve": D.REINHARD, "white": 2.0, "encode": D.LINEAR}, {"curve": D.CLAMP, "exposure": 3.0}):
            for m in (None, (0.18, 0.5, 0.95), (0.3, 0.0, 1.0)):
                got = room.accum_display(p, metering=m, denoise=denoise, want_rgb=True)
                want = stateless(room, src, p, m)
                assert np.array_equal(got[0], want[0]), (kind, denoise, p, m)
                assert same_floats(got[1], want[1]), (kind, denoise, p, m)
                assert F(got[2]).view(np.uint32) == F(want[2]).view(np.uint32), (kind, denoise, p, m, got[2], want[2])
                if m is not None:
                    assert got[2] == D.exposure(D.histogram(src), *m)
                assert np.array_equal(room.accum_display(p, metering=m, denoise=denoise)[0], want[0])


@pytest.mark.parametrize("kind", ["plain", "adaptive", "reprojected"])
def test_the_accumulation_is_untouched(room, kind):
    begin(room, kind)
    want = room.accum_step(2, want_mean=True)
    want_counts = room.accum_counts()[0]
    begin(room, kind)
    room.accum_display({}, metering=True, want_rgb=True)
    room.accum_display({}, metering=True, denoise=True)
    got = room.accum_step(2, want_mean=True)
    assert hc.same(got[:2], want[:2]) and got[2] == want[2]
    assert np.array_equal(room.accum_counts()[0], want_counts)


# ---------------------------------------------------------------------------------------------------------------- refusals
BAD_DISPLAY = {
    "exposure zero": {"exposure": 0.0}, "exposure negative": {"exposure": -1.0}, "exposure inf": {"exposure": np.inf}, "exposure nan": {"exposure": np.nan},
    "white zero": {"white": 0.0}, "white negative": {"white": -4.0}, "white inf": {"white": np.inf}, "white nan": {"white": np.nan},
    "curve": {"curve": 3}, "encode": {"encode": 2},
}
BAD_METERING = ((0.0, 0.5, 0.95), (np.nan, 0.5, 0.95), (np.inf, 0.5, 0.95), (0.18, -0.1, 0.95), (0.18, 0.5, 1.5), (0.18, 0.5, 0.5), (0.18, 0.9, 0.2),
                (0.18, np.nan, 0.95))


def _reserved(cls, field="reserved", index=None):
    x = cls.defaults()
    if index is None:
        setattr(x, field, 1)
    else:
        getattr(x, field)[index] = 1
    return x


def test_refusals_of_the_device_calls(ctx, T):
    import torch
    img = image(63, T, 5)
    d_img = dev(img)
    out = torch.full((63,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    hist = torch.full((D.BINS,), 7, dtype=torch.int32, device="cuda")
    bad = [capi.Display.make(v) for v in BAD_DISPLAY.values()] + [_reserved(capi.Display, index=0), _reserved(capi.Display, index=1)]
    for p in bad:
        assert D.check_display(p.exposure, p.white, p.curve, p.encode, tuple(p.reserved)) != "ok"
        with pytest.raises(capi.SpathHipError, match=hc.E_INVALID):
            ctx.display_device(63, d_img.data_ptr(), out.data_ptr(), params=p, stream=stream())
    L, h = ctx._L, ctx._h
    good = capi.Display.defaults()
    assert L.sphip_display_device(h, None, 63, d_img.data_ptr(), out.data_ptr(), None, None) == -1
    assert L.sphip_display_device(h, C.byref(good), 63, None, out.data_ptr(), None, None) == -1
    assert L.sphip_display_device(h, C.byref(good), 63, d_img.data_ptr(), None, None, None) == -1
    assert L.sphip_display_device(h, C.byref(good), 0, d_img.data_ptr(), out.data_ptr(), None, None) == -1
    assert L.sphip_display_device(None, C.byref(good), 63, d_img.data_ptr(), out.data_ptr(), None, None) == -1
    assert L.sphip_luminance_histogram_device(h, 0, d_img.data_ptr(), hist.data_ptr(), None) == -1
    assert L.sphip_luminance_histogram_device(h, 63, None, hist.data_ptr(), None) == -1
    assert L.sphip_luminance_histogram_device(h, 63, d_img.data_ptr(), None, None) == -1
    assert L.sphip_luminance_histogram_device(None, 63, d_img.data_ptr(), hist.data_ptr(), None) == -1
    sync()
    assert (out.cpu().numpy() == 0x5A5A5A5A).all() and (hist.cpu().numpy() == 7).all()


def test_device_calls_need_a_single_device_context(T):
    import torch
    mc = capi.Context.multi([0, 0])
    d_img = dev(image(63, T, 5))
    out = torch.zeros(63, dtype=torch.int32, device="cuda")
    hist = torch.zeros(D.BINS, dtype=torch.int32, device="cuda")
    with pytest.raises(capi.SpathHipError, match=hc.E_STATE):
        mc.display_device(63, d_img.data_ptr(), out.data_ptr())
    with pytest.raises(capi.SpathHipError, match=hc.E_STATE):
        mc.luminance_histogram_device(63, d_img.data_ptr(), hist.data_ptr())
    mc.close()


def test_refusals_of_accum_display_change_nothing():
    t, m = scene.closed_room(200)
    c = hc.ctx(t, m)
    cam, _ = hc.cam_rays(W, H)
    c._accum_shape = (W, H)
    with pytest.raises(capi.SpathHipError, match=hc.E_STATE):           # no accumulation
        c.accum_display()
    c.accum_begin(cam=cam, seed=3)
    with pytest.raises(capi.SpathHipError, match=hc.E_STATE):           # before the first step, as sphip_accum_denoise
        c.accum_display()
    with pytest.raises(capi.SpathHipError, match=hc.E_STATE):
        c.accum_denoise()
    c.accum_step(2)
    for p in list(BAD_DISPLAY.values()) + [_reserved(capi.Display, index=0)]:
        with pytest.raises(capi.SpathHipError, match=hc.E_INVALID):
            c.accum_display(p)
    for mt in [capi.Metering(*[float(x) for x in v], 0) for v in BAD_METERING] + [_reserved(capi.Metering)]:
        with pytest.raises(capi.SpathHipError, match=hc.E_INVALID):
            c.accum_display({}, metering=mt)
    for dn in ({"iterations": 9}, {"sigma_depth": 0.0}, {"sigma_lum": np.nan}, _reserved(capi.Denoise, index=1)):
        with pytest.raises(capi.SpathHipError, match=hc.E_INVALID):
            c.accum_display({}, denoise=dn)
    good = capi.Display.defaults()
    out = np.zeros((W * H, 4), np.uint8)
    assert c._L.sphip_accum_display(c._h, None, None, None, out.ctypes.data, None, None) == -1
    assert c._L.sphip_accum_display(c._h, C.byref(good), None, None, None, None, None) == -1
    assert c._L.sphip_accum_display(None, C.byref(good), None, None, out.ctypes.data, None, None) == -1
    assert not out.any()
    got = c.accum_step(2, want_mean=True)
    c.accum_begin(cam=cam, seed=3)
    c.accum_step(2)
    assert hc.same(got[:2], c.accum_step(2, want_mean=True)[:2])
    c.set_scene(t, m)                                                   # a scene since the begin
    with pytest.raises(capi.SpathHipError, match=hc.E_STATE):
        c.accum_display()
    c.close()


# ---------------------------------------------------------------------------------------------------------------- extents
@pytest.mark.parametrize("n", [1, 63, 257, 1040])
def test_extents(ctx, T, n):
    img = image(n, T, 6)
    held(ctx, lambda p, st: ctx.luminance_histogram_device(n, p("mean"), p("hist"), st), {"mean": img}, {"hist": D.BINS * 4}, what="histogram n %d" % n)
    for enc in ENCODES:
        for with_rgb in (False, True):
            outs = {"rgba": n * 4, **({"rgb": n * 12} if with_rgb else {})}
            held(ctx, lambda p, st: ctx.display_device(n, p("mean"), p("rgba"), d_out_rgb=p("rgb") if with_rgb else 0,
                                                       params={"curve": D.FILMIC, "encode": enc, "exposure": 0.7}, stream=st),
                 {"mean": img}, outs, what="display n %d encode %d rgb %d" % (n, enc, with_rgb))


# ---------------------------------------------------------------------------------------------------------------- multi-device
def _multi_equals_single(devices):
    t, m = scene.closed_room(200)
    cam, _ = hc.cam_rays(W, H)
    out = []
    for devs in (None, devices):
        c = hc.ctx(t, m, devs=devs)
        got = []
        for adaptive in (None, ADAPTIVE):
            c.accum_begin(cam=cam, seed=3, adaptive=adaptive)
            c.accum_step(4)
            c.accum_step(4)
            for denoise in (None, {"iterations": 2}):
                got.append(c.accum_display({}, metering=True, denoise=denoise, want_rgb=True))
                got.append(c.accum_display({"curve": D.REINHARD, "encode": D.LINEAR, "exposure": 2.0}, denoise=denoise, want_rgb=True))
        c.close()
        out.append(got)
    for a, b in zip(*out):
        assert np.array_equal(a[0], b[0]) and same_floats(a[1], b[1]) and a[2] == b[2]


def test_several_shards_on_one_device_give_the_single_device_bytes():
    _multi_equals_single([0, 0, 0])


def test_multi_device_gives_the_single_device_bytes():
    import torch
    n = torch.cuda.device_count()
    if n < 2:
        pytest.skip("one GPU on this box")
    _multi_equals_single(list(range(n)))


# ---------------------------------------------------------------------------------------------------------------- the point
def test_auto_exposure_does_not_change_with_the_lights_power():
    """An open scene lit by the sky alone, 32 x 32 at 4 spp.  The map times 8 scales every sample, every sum and every mean by exactly 8
    (a power of two, nothing near the ends of the exponent range: checked below), which moves every pixel up 24 bins and the metered
    exposure down to exactly 1/8: the auto-exposed RGBA8 is the same, byte for byte.  The clamp-only image is not: it saturates."""
    t, m = scene.open_clutter(100)
    m = m.copy()
    m[:, 3:6] = 0                                                       # the sky is the only light
    env = scene.sky_environment(16)
    cam, _ = hc.cam_rays(32, 32)
    shown, clamped, means, exposures = [], [], [], []
    for scale in (1.0, 8.0):
        c = hc.ctx(t, m, env=F(env * F(scale)))
        c.accum_begin(cam=cam, seed=3, flags=capi.FLAG_ENVIRONMENT)
        img, mean, _ = c.accum_step(4, want_mean=True)
        out, e = c.accum_display({}, metering=True)
        shown.append(out), clamped.append(img), means.append(mean), exposures.append(e)
        c.close()
    b1, b8 = D.bins(means[0]), D.bins(means[1])
    lit = b1 > 0
    assert lit.sum() > 512, "most of the frame sees the sky, directly or by a bounce"
    assert b1[lit].min() >= 8 + 24 and b8.max() < 2040 - 24 and np.isfinite(means[1]).all()      # no denormal, no overflow, with room
    assert np.array_equal(means[1].view(np.uint32), F(means[0] * F(8)).view(np.uint32))
    assert np.array_equal(b8[lit], b1[lit] + 24) and not b8[~lit].any()
    assert exposures[1] == exposures[0] / 8 and exposures[0] == D.exposure(D.histogram(means[0]))
    assert np.array_equal(shown[0], shown[1])
    assert shown[0][:, :3].max() > 128 and len(np.unique(shown[0][:, 0])) > 32       # a picture, not a sheet
    sat1, sat8 = int((clamped[0][:, :3] == 255).sum()), int((clamped[1][:, :3] == 255).sum())
    print("saturated channels of the clamp-only image: x1 %d, x8 %d; exposure x1 %g" % (sat1, sat8, exposures[0]))
    assert sat8 > sat1
    assert not np.array_equal(clamped[0], clamped[1])
