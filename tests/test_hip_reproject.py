"""Temporal reprojection on the GPU (include/spath_hip.h "temporal reprojection"): the kernels against the numpy
statement (tests/reproject_model.py) with tolerance 0, the stateful calls against their composition from the stateless ones, the
refusals, the extents, and what a history buys.  Parameters are explicit wherever a result depends on them; the library's defaults
appear only where the test is about them."""
import ctypes as C

import numpy as np
import pytest

import hip_checks as hc
import reproject_model as M
from hip_checks import _torch_first  # noqa: F401  (fixture)
from model_primitives import F
from spath_amd import capi, scene

pytestmark = pytest.mark.gpu

FRAMES = ((1, 1), (7, 5), (64, 4), (65, 3), (40, 26))
SCENES = {"closed_room": lambda: scene.closed_room(300), "open_clutter": lambda: scene.open_clutter(100)}
PARAMS = (24.0, 0.9, 0.02)                                       # explicit: a cap inside the range of the random history counts
LOOSE_NORMAL = (1e9, -1.0, 0.001)                                # no cap, every normal passes: the plane test alone tells surfaces apart
PARAM_SETS = (PARAMS, LOOSE_NORMAL)
POISONED = "poisoned"                                            # the pair "pan" with one ray whose hit point overflows: `nonfinite`
NEE_MIS = hc.NEE_MIS


def guarded(fn, what):
    """a device error ends the session: nothing more is started on the GPU"""
    try:
        return fn()
    except capi.SpathHipError as e:
        if "[-2]" in str(e):
            pytest.exit("device error in %s: %s" % (what, e), returncode=3)
        raise


def up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).ravel().copy()).to("cuda")


def zeros(nbytes):
    import torch
    return torch.zeros(nbytes, dtype=torch.uint8, device="cuda")


def down(t, dtype, shape=(-1,)):
    return t.cpu().numpy().view(dtype).reshape(shape)


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def sync():
    import torch
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- 1. kernel = model
def model_case(scene_name, w, h, pair, tm):
    """the inputs of one case and what the model makes of them"""
    t, m = tm
    prev, cur = M.camera_pair("pan" if pair == POISONED else pair, w, h)
    rp, rc = (np.ascontiguousarray(c.get_viewport(), F) for c in (prev, cur))
    gp, gc = M.gbuffer(rp, t, m)[0], M.gbuffer(rc, t, m)[0]
    n = w * h
    if pair == POISONED:
        hit = np.flatnonzero(gc["mat"] >= 0)
        if hit.size:
            rc[hit[0], 3] = 1e38                                 # P.x = inf; the turned previous view keeps c.z = +inf: fx is NaN
    rng = np.random.default_rng([w, h, sorted(M.PAIRS).index(pair) if pair in M.PAIRS else 99, len(scene_name)])
    mean_prev = (rng.random((n, 3)) * 4).astype(F)
    hist_prev = np.where(rng.random(n) < 0.2, 0, rng.random(n) * 40).astype(F)
    k = {"prev": prev, "rc": rc, "gc": gc, "rp": rp, "gp": gp, "mean_prev": mean_prev, "hist_prev": hist_prev}
    for ps in PARAM_SETS:                                        # -> mean, hist, pixel codes, tap codes
        k[ps] = M.reproject(ps, prev, w, h, rc, gc, rp, gp, mean_prev, hist_prev)[:4]
    k["mean"], k["hist"], k["code"], k["tap"] = k[PARAMS]
    return k


@pytest.fixture(scope="module")
def cases():
    """every case's inputs and model outputs, computed once; and the condition on them, checked before the GPU is asked"""
    out = {}
    for name, make in SCENES.items():
        tm = make()
        for w, h in FRAMES:
            for pair in tuple(M.PAIRS) + (POISONED,):
                out[name, w, h, pair] = model_case(name, w, h, pair, tm)
    codes = np.concatenate([c[ps][2] for c in out.values() for ps in PARAM_SETS])
    taps = np.concatenate([c[ps][3].ravel() for c in out.values() for ps in PARAM_SETS])
    for k, word in enumerate(M.PIXEL_CODES):
        assert (codes == k).any(), "no pixel is `%s`" % word
    for k, word in enumerate(M.TAP_CODES):
        assert (taps == k).any(), "no tap is `%s`" % word
    hits = codes != M.MISS
    assert (codes == M.TAKEN).sum() * 4 >= hits.sum(), "fewer than a quarter of the camera-hit pixels are taken"
    return out


def run_reproject(c, params, k, w, h):
    n = w * h
    d = {key: up(k[key]) for key in ("rc", "gc", "rp", "gp", "mean_prev", "hist_prev")}
    om, oh = zeros(n * 12), zeros(n * 4)
    guarded(lambda: c.reproject_device(params, k["prev"], w, h, d["rc"].data_ptr(), d["gc"].data_ptr(), d["rp"].data_ptr(), d["gp"].data_ptr(),
                                       d["mean_prev"].data_ptr(), d["hist_prev"].data_ptr(), om.data_ptr(), oh.data_ptr(), stream()), "reproject_device")
    sync()
    return down(om, F, (n, 3)), down(oh, F)


@pytest.fixture(scope="module")
def bare():
    """a context without a scene: the two stateless calls need none"""
    c = capi.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("frame", FRAMES, ids=lambda f: "%dx%d" % f)
@pytest.mark.parametrize("name", sorted(SCENES))
def test_kernel_is_the_model(bare, cases, name, frame):
    w, h = frame
    for pair in tuple(M.PAIRS) + (POISONED,):
        k = cases[name, w, h, pair]
        for ps in PARAM_SETS:
            mean, hist = run_reproject(bare, ps, k, w, h)
            assert mean.tobytes() == k[ps][0].tobytes(), (name, frame, pair, ps, "mean")
            assert hist.tobytes() == k[ps][1].tobytes(), (name, frame, pair, ps, "hist")


# ---------------------------------------------------------------------------------------------------------------- 2. resolve = model
RESOLVE_FRAMES = {1: (1, 1), 63: (9, 7), 65: (13, 5), 1040: (40, 26)}


@pytest.fixture(scope="module")
def room():
    t, m = scene.closed_room(300)
    c = hc.ctx(t, m)
    yield c, t, m
    c.close()


@pytest.mark.parametrize("n", sorted(RESOLVE_FRAMES))
def test_resolve_is_the_model(room, n):
    c, _, _ = room
    w, h = RESOLVE_FRAMES[n]
    rays = hc.cam_rays(w, h)[1]
    d_rays, d_sum, d_rgba, d_mean = up(rays), zeros(n * 12), zeros(n * 4), zeros(n * 12)
    guarded(lambda: c.render_device_accum(d_rays.data_ptr(), n, 0, 3, d_sum.data_ptr(), d_rgba.data_ptr(), seed=5, image_width=w,
                                          d_out_mean=d_mean.data_ptr(), stream=stream()), "render_device_accum")
    sync()
    s, plain_rgba, plain_mean = down(d_sum, F, (n, 3)), down(d_rgba, np.uint8, (n, 4)), down(d_mean, F, (n, 3))
    rng = np.random.default_rng(n)
    hm = rng.random((n, 3)).astype(F)
    hh = np.where(np.arange(n) % 3 == 1, 0, 1 + rng.random(n) * 30).astype(F)
    for hist in (None, hh, np.zeros(n, F)):                      # no history, a history in two pixels of three, one of zeros
        o_rgba, o_mean = zeros(n * 4), zeros(n * 12)
        d_hm, d_hh = (up(hm), up(hist)) if hist is not None else (None, None)
        guarded(lambda: c.temporal_resolve_device(n, d_sum.data_ptr(), 3, o_rgba.data_ptr(), o_mean.data_ptr(),
                                                  d_hist_mean=d_hm.data_ptr() if d_hm is not None else 0,
                                                  d_hist=d_hh.data_ptr() if d_hh is not None else 0, stream=stream()), "temporal_resolve_device")
        sync()
        got_rgba, got_mean = down(o_rgba, np.uint8, (n, 4)), down(o_mean, F, (n, 3))
        want = M.blend(s, 3, hm if hist is not None else None, hist)
        assert got_mean.tobytes() == want.tobytes() and got_rgba.tobytes() == M.rgba(want).tobytes()
        plain = np.ones(n, bool) if hist is None else hist == 0
        assert plain.any() or n == 1
        assert got_mean[plain].tobytes() == plain_mean[plain].tobytes() and got_rgba[plain].tobytes() == plain_rgba[plain].tobytes()
    # either output alone
    o_rgba = zeros(n * 4)
    c.temporal_resolve_device(n, d_sum.data_ptr(), 3, o_rgba.data_ptr(), 0, stream=stream())
    sync()
    assert down(o_rgba, np.uint8, (n, 4)).tobytes() == plain_rgba.tobytes()


# ---------------------------------------------------------------------------------------------------------------- 3. stateful = composition
W3, H3 = 40, 26
N3 = W3 * H3
SEEDS3 = (11, 12, 13)


def views3():
    """three views: the tests' base view, a pan of a few pixels, then a small turn"""
    a, b = M.camera_pair("pan", W3, H3)
    c = M.camera_pair("pan", W3, H3)[1]
    c.set_delta_rot((0.0, 0.05, 0.0))
    return a, b, c


def stateful(c, flags, params, want_all=True):
    """the sequence through the accumulation -> [(rgba, mean, total) per step], history, G-buffer"""
    v = views3()
    steps = []
    c.accum_begin(cam=v[0], seed=SEEDS3[0], flags=flags)
    for k in (3, 2):
        steps.append(guarded(lambda: c.accum_step(k, want_mean=True), "accum_step"))
    guarded(lambda: c.accum_reproject(v[1], SEEDS3[1], params), "accum_reproject")
    for k in (2, 1):
        steps.append(guarded(lambda: c.accum_step(k, want_mean=True), "accum_step"))
    guarded(lambda: c.accum_reproject(v[2], SEEDS3[2], params), "accum_reproject")
    steps.append(guarded(lambda: c.accum_step(2, want_mean=True), "accum_step"))
    return steps, c.accum_history(), c.accum_gbuffer()


def composed(c, flags, params):
    """the same from the stateless calls -> the same"""
    v = views3()
    st = stream()
    steps = []
    hmean = hist = None                                          # the history attached to the current view (device tensors)
    prev = None                                                  # (camera, rays, G-buffer) of the view being left
    pair = None
    for view_k, (cam, seed, splits) in enumerate(zip(v, SEEDS3, ((3, 2), (2, 1), (2,)))):
        rays, gbuf = zeros(N3 * 24), zeros(N3 * 32)
        c.viewport_device(cam, rays.data_ptr(), st)
        guarded(lambda: c.gbuffer_device(rays.data_ptr(), N3, gbuf.data_ptr(), flags=flags, stream=st), "gbuffer_device")
        if prev is not None:
            hmean, hist = zeros(N3 * 12), zeros(N3 * 4)
            guarded(lambda: c.reproject_device(params, prev[0], W3, H3, rays.data_ptr(), gbuf.data_ptr(), prev[1].data_ptr(), prev[2].data_ptr(),
                                               pair[0].data_ptr(), pair[1].data_ptr(), hmean.data_ptr(), hist.data_ptr(), st), "reproject_device")
        d_sum, total = zeros(N3 * 12), 0
        for k in splits:
            o_rgba, o_mean = zeros(N3 * 4), zeros(N3 * 12)
            guarded(lambda: c.render_device_accum(rays.data_ptr(), N3, total, k, d_sum.data_ptr(), o_rgba.data_ptr(), seed=seed, flags=flags,
                                                  image_width=W3, d_out_mean=o_mean.data_ptr(), stream=st), "render_device_accum")
            total += k
            if hist is not None:
                c.temporal_resolve_device(N3, d_sum.data_ptr(), total, o_rgba.data_ptr(), o_mean.data_ptr(), d_hist_mean=hmean.data_ptr(),
                                          d_hist=hist.data_ptr(), stream=st)
            sync()
            steps.append((down(o_rgba, np.uint8, (N3, 4)), down(o_mean, F, (N3, 3)), total))
        # what this view hands on: its blended mean, and its history count plus its samples (an f32 addition)
        own = down(hist, F) if hist is not None else np.zeros(N3, F)
        pair = (up(steps[-1][1]), up((own + F(total)).astype(F)))
        prev = (cam, rays, gbuf)
    return steps, own, down(gbuf, capi.gbuffer_dtype())


def same_steps(a, b):
    return len(a) == len(b) and all(x[0].tobytes() == y[0].tobytes() and x[1].tobytes() == y[1].tobytes() and x[2] == y[2] for x, y in zip(a, b))


@pytest.mark.parametrize("flags", (0, NEE_MIS), ids=("plain", "nee_mis"))
def test_stateful_is_the_composition(flags):
    t, m = scene.closed_room(300)
    a, b = hc.ctx(t, m), hc.ctx(t, m)
    try:
        got, want = stateful(a, flags, PARAMS), composed(b, flags, PARAMS)
        assert same_steps(got[0], want[0])
        assert [s[2] for s in got[0]] == [3, 5, 2, 3, 2]                     # total_out counts the new samples only
        assert got[1].tobytes() == want[1].tobytes() and (got[1] > 0).sum() > N3 // 2
        assert got[2].tobytes() == want[2].tobytes()
        # the G-buffer is the model's for the last view (what the calibration on the CPU stands on)
        g = M.gbuffer(np.ascontiguousarray(views3()[2].get_viewport(), F), t, m)[0]
        assert got[2].tobytes() == g.tobytes()
        # the denoiser filters the blended mean: K = 0 returns it as it stands
        img, rgb = a.accum_denoise(dict(iterations=0), want_rgb=True)
        assert img.tobytes() == got[0][-1][0].tobytes() and rgb.tobytes() == got[0][-1][1].tobytes()
        # ... and with K > 0 it is the stateless filter of that mean, without variance
        img5 = a.accum_denoise(dict(iterations=2, normal_log2=2, sigma_depth=0.2, sigma_lum=4.0))
        d_mean, d_g, o = up(got[0][-1][1]), up(got[2]), zeros(N3 * 4)
        b.denoise_device(W3, H3, d_mean.data_ptr(), d_g.data_ptr(), o.data_ptr(), params=dict(iterations=2, normal_log2=2, sigma_depth=0.2, sigma_lum=4.0),
                         stream=stream())
        sync()
        assert img5.tobytes() == down(o, np.uint8, (N3, 4)).tobytes()
        # a plain begin drops the history
        a.accum_begin(cam=views3()[0], seed=SEEDS3[0], flags=flags)
        assert not a.accum_history().any()
        assert same_steps([a.accum_step(3, want_mean=True)], got[0][:1])
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("flags", (0, NEE_MIS), ids=("plain", "nee_mis"))
def test_without_history_the_frame_is_the_plain_accumulation(flags):
    t, m = scene.closed_room(300)
    a, b = hc.ctx(t, m), hc.ctx(t, m)
    try:
        v = views3()
        b.accum_begin(cam=v[1], seed=SEEDS3[1], flags=flags)
        plain = [b.accum_step(2, want_mean=True), b.accum_step(1, want_mean=True)]
        # max_history = 0: no history is taken over, the whole frame is the plain accumulation at the new view and seed
        for params, whole in (((0.0, 0.9, 0.02), True), (None, False)):          # None: the library's defaults
            a.accum_begin(cam=v[0], seed=SEEDS3[0], flags=flags)
            a.accum_step(5)
            a.accum_reproject(v[1], SEEDS3[1], params)
            got = [a.accum_step(2, want_mean=True), a.accum_step(1, want_mean=True)]
            none = a.accum_history() == 0
            assert none.all() if whole else (none.any() and not none.all())
            for x, y in zip(got, plain):
                assert x[0][none].tobytes() == y[0][none].tobytes() and x[1][none].tobytes() == y[1][none].tobytes() and x[2] == y[2]
    finally:
        a.close()
        b.close()


# ---------------------------------------------------------------------------------------------------------------- 4. refusals
GOOD = (8.0, 0.9, 0.02)


def reproject_rc(c, cam, params, seed=9, reserved=0, null_cam=False, null_params=False):
    """sphip_accum_reproject's status itself"""
    p = capi.Reproject(*[float(x) for x in params], reserved)
    ca = capi.CameraArgs.from_camera(cam)
    return c._L.sphip_accum_reproject(c._h, None if null_cam else C.byref(ca), seed, None if null_params else C.byref(p))


def next_step(c):
    try:
        return c.accum_step(1, want_mean=True)
    except capi.SpathHipError as e:
        return str(e)[:40]


def test_refusals_change_nothing():
    t, m = scene.closed_room(300)
    w, h = 16, 12
    cam, cam2 = M.camera_pair("pan", w, h)
    other = M.camera_pair("pan", w + 1, h)[1]
    rays = np.ascontiguousarray(cam.get_viewport(), F)
    E_INVALID, E_STATE = -1, -3

    def live(c):
        c.accum_begin(cam=cam, seed=4, flags=0)
        c.accum_step(2)

    def stale(c):
        live(c)
        c.set_scene(t, m)

    def stale_by_setter(c):
        live(c)
        c.set_specular(np.zeros((t.shape[0], 4), F))

    def from_rays(c):
        c.accum_begin(rays=rays, w=w, h=h, seed=4)
        c.accum_step(2)

    def adaptive(c):
        c.accum_begin(cam=cam, seed=4, adaptive=(0.05, 0.01, 2))
        c.accum_step(2)

    def unstepped(c):
        c.accum_begin(cam=cam, seed=4)

    nan, inf = float("nan"), float("inf")
    table = [(None, lambda c: None, {}, E_STATE), (None, stale, {}, E_STATE), (None, stale_by_setter, {}, E_STATE), (None, from_rays, {}, E_STATE), (None, adaptive, {}, E_STATE),
             (None, unstepped, {}, E_STATE), ([0, 0], live, {}, E_STATE),
             (None, live, {"null_cam": True}, E_INVALID), (None, live, {"null_params": True}, E_INVALID), (None, live, {"cam": other}, E_INVALID),
             (None, live, {"reserved": 1}, E_INVALID)]
    table += [(None, live, {"params": p}, E_INVALID) for p in ((-1.0, 0.9, 0.02), (nan, 0.9, 0.02), (inf, 0.9, 0.02), (8.0, 1.5, 0.02), (8.0, -1.5, 0.02),
                                                                (8.0, nan, 0.02), (8.0, 0.9, -0.5), (8.0, 0.9, nan), (8.0, 0.9, inf))]
    for devs, setup, kw, code in table:
        a, b = hc.ctx(t, m, devs=devs), hc.ctx(t, m, devs=devs)
        try:
            setup(a)
            setup(b)
            kw = dict(kw)
            rc = reproject_rc(a, kw.pop("cam", cam2), kw.pop("params", GOOD), **kw)
            assert rc == code, (setup.__name__, kw, rc, a._L.sphip_last_error(a._h))
            x, y = next_step(a), next_step(b)
            if isinstance(x, str) or isinstance(y, str):
                assert x == y
            else:
                assert same_steps([x], [y])
        finally:
            a.close()
            b.close()
    # the stateless calls
    c = capi.Context(0)
    try:
        k = model_case("closed_room", 7, 5, "pan", (t, m))
        for bad in ((-1.0, 0.9, 0.02), (8.0, 2.0, 0.02), (8.0, 0.9, nan)):
            with pytest.raises(capi.SpathHipError, match=hc.E_INVALID):
                run_reproject(c, bad, k, 7, 5)
        with pytest.raises(capi.SpathHipError, match=hc.E_INVALID):
            run_reproject(c, GOOD, k, 5, 7)                                      # not the previous camera's frame
        with pytest.raises(capi.SpathHipError, match=hc.E_INVALID):
            c.temporal_resolve_device(35, 0, 3, 0, 0)
        with pytest.raises(capi.SpathHipError, match=hc.E_STATE):
            c.accum_history()
    finally:
        c.close()


# ---------------------------------------------------------------------------------------------------------------- 5. extents
BAND = 4096
FILLS = (0xFF, 0x00, 0xA5)


class Separate:
    """every region a tensor of its own"""
    def __init__(self, inputs, outputs):
        self.t = {k: up(v) for k, v in inputs.items()}
        self.t.update({k: zeros(n) for k, n in outputs.items()})

    def ptr(self, name):
        return self.t[name].data_ptr()

    def get(self, name):
        return self.t[name].cpu().numpy()

    def intact(self):
        return True


class Carved:
    """every region inside one allocation filled with one byte value; regions start on 256-byte boundaries, as separate allocations do,
    with at least BAND bytes of the fill before, between and behind them (the method of tests/test_hip_extents.py)"""
    def __init__(self, inputs, outputs, fill):
        import torch
        self.fill, self.off, self.size = fill, {}, {}
        pos = BAND
        for k, n in list((k, np.ascontiguousarray(v).nbytes) for k, v in inputs.items()) + list(outputs.items()):
            self.off[k], self.size[k] = pos, n
            pos = (pos + n + BAND + 255) // 256 * 256
        self.buf = torch.full((pos,), fill, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 256 == 0
        for k, v in inputs.items():
            self.buf[self.off[k]:self.off[k] + self.size[k]] = up(v)

    def ptr(self, name):
        return self.buf.data_ptr() + self.off[name]

    def get(self, name):
        return self.buf[self.off[name]:self.off[name] + self.size[name]].cpu().numpy()

    def intact(self):
        hst = self.buf.cpu().numpy()
        outside = np.ones(hst.size, bool)
        for k in self.off:
            outside[self.off[k]:self.off[k] + self.size[k]] = False
        return bool((hst[outside] == self.fill).all())


def held(fn, inputs, outputs, what):
    """fn(ptr, stream) on separate tensors and on the three carvings: bands intact, outputs equal"""
    want = None
    for fill in (None,) + FILLS:
        mem = Separate(inputs, outputs) if fill is None else Carved(inputs, outputs, fill)
        sync()
        guarded(lambda: fn(mem.ptr, stream()), what)
        sync()
        got = {k: mem.get(k) for k in outputs}
        assert mem.intact(), "%s: a byte outside the stated extents changed (fill 0x%02x)" % (what, fill)
        if want is None:
            want = got
            continue
        for k in want:
            assert np.array_equal(got[k], want[k]), "%s: output %s depends on what surrounds the buffers (fill 0x%02x)" % (what, k, fill)
    return want


@pytest.mark.parametrize("n", sorted(RESOLVE_FRAMES))
def test_extents(bare, n):
    w, h = RESOLVE_FRAMES[n]
    t, m = SCENES["open_clutter"]()
    outs = None
    for pair in ("pan", "turn_off_frame"):
        k = model_case("open_clutter", w, h, pair, (t, m))
        inputs = {key: k[key] for key in ("rc", "gc", "rp", "gp", "mean_prev", "hist_prev")}
        outs = held(lambda p, st: bare.reproject_device(PARAMS, k["prev"], w, h, p("rc"), p("gc"), p("rp"), p("gp"), p("mean_prev"), p("hist_prev"),
                                                        p("om"), p("oh"), st), inputs, {"om": n * 12, "oh": n * 4}, "reproject_device " + pair)
        assert outs["om"].tobytes() == k["mean"].tobytes() and outs["oh"].tobytes() == k["hist"].tobytes()
    rng = np.random.default_rng(n)
    s, hm = (rng.random((n, 3)) * 9).astype(F), rng.random((n, 3)).astype(F)
    hh = np.where(np.arange(n) % 2 == 0, 0, 7).astype(F)
    held(lambda p, st: bare.temporal_resolve_device(n, p("sum"), 3, p("rgba"), p("mean"), d_hist_mean=p("hm"), d_hist=p("hh"), stream=st),
         {"sum": s, "hm": hm, "hh": hh}, {"rgba": n * 4, "mean": n * 12}, "temporal_resolve_device")
    held(lambda p, st: bare.temporal_resolve_device(n, p("sum"), 3, 0, p("mean"), stream=st), {"sum": s}, {"mean": n * 12},
         "temporal_resolve_device without history or rgba")


# ---------------------------------------------------------------------------------------------------------------- 6. it helps
QUALITY_BOUND = 0.4099                                           # sqrt(0.1680 * 1): tools/reproject_calibrate.py ratios


def test_a_history_helps(room):
    """closed_room(300), NEE|MIS, 32x32, the pair "pan": 16 spp of history at the old view, 4 new samples at the new one, against 4096
    samples of the new view under another seed.  Over the pixels with history, per seed, the mean squared error of the blend over that
    of the 4 new samples alone stays below QUALITY_BOUND: the geometric mean of 1 and the worst of the eight ratios measured with the
    numpy statements (tools/reproject_calibrate.py; DESIGN.md section 5.19 lists them).  The ideal, ignoring resampling bias, is 4/20."""
    c, t, m = room
    w = h = 32
    n = w * h
    prev, cur = M.camera_pair("pan", w, h)
    params = capi.Reproject.defaults()
    ref = c.render_camera(cur, 4096, seed=987654321, flags=NEE_MIS, want_accum=True)[1].astype(np.float64)
    ratios = []
    for seed in range(1, 9):
        c.accum_begin(cam=cur, seed=seed + 1000, flags=NEE_MIS)
        alone = c.accum_step(4, want_mean=True)[1]
        c.accum_begin(cam=prev, seed=seed, flags=NEE_MIS)
        c.accum_step(16)
        c.accum_reproject(cur, seed + 1000, params)
        blend = c.accum_step(4, want_mean=True)[1]
        has = c.accum_history() > 0
        assert has.sum() > n // 2
        mse = lambda a: float(((a[has].astype(np.float64) - ref[has]) ** 2).mean())
        ratios.append(mse(blend) / mse(alone))
    print("ratios", " ".join("%.4f" % r for r in ratios), "bound", QUALITY_BOUND)
    assert all(r < QUALITY_BOUND for r in ratios), ratios


# ---------------------------------------------------------------------------------------------------------------- 7. the hosts
def test_hosts_reproject_where_they_would_restart(tmp_path):
    """HipRenderer.set_reproject and spath_cli --reproject --then-move give the bytes of the C calls they stand for: a begin and a step at
    the first view, sphip_accum_reproject under seed + 1 at the moved camera, a step there; and both refuse an adaptive rule with the
    library's message."""
    import os
    import subprocess
    from spath_amd import renderer, view
    from test_host_adapter import CLI
    t, m = scene.closed_room(300)
    w, h, mv = 40, 26, (0.25, -0.125, 0.5)
    c = hc.ctx(t, m)
    cam = view.Camera(w, h)
    c.accum_begin(cam=cam, seed=7)
    first, _ = c.accum_step(4)
    cam.set_delta_mov(mv)
    c.accum_reproject(cam, 8, GOOD)
    second, total = c.accum_step(2)
    plain = c.render_camera(cam, 2, seed=8)
    c.close()
    assert total == 2 and not np.array_equal(second, plain)
    r = renderer.HipRenderer(w, h, seed=7, progressive=True)
    try:
        r.set_reproject(GOOD)
        out = renderer.Bitmap()
        r.render_own_viewport(t, m, t.shape[0], 4, out)
        assert out.values.tobytes() == first.tobytes()
        r.set_delta_mov(mv)
        r.render_own_viewport(t, m, t.shape[0], 2, out)
        assert out.values.tobytes() == second.tobytes()
        r.set_viewport_size(w + 2, h)                                            # a resize begins anew
        r.render_own_viewport(t, m, t.shape[0], 1, out)
        assert not r.ctx.accum_history().any()
    finally:
        r.close()
    r = renderer.HipRenderer(w, h, progressive=True, adaptive=(0.05, 0.1, 4))
    try:
        with pytest.raises(capi.SpathHipError, match="needs a plain accumulation, not an adaptive one"):
            r.set_reproject(GOOD)
    finally:
        r.close()
    sp, a, b = (os.path.join(tmp_path, f) for f in ("s.bin", "a.rgba", "b.rgba"))
    scene.write_scene(sp, t, m)
    base = [CLI, "--scene", sp, "--w", str(w), "--h", str(h), "--seed", "7", "--spp", "4", "--progressive", "4", "--reproject", "8,0.9,0.02",
            "--then-move", ",".join(str(x) for x in mv), "--spp-after", "2"]
    p = subprocess.run(base + ["--out", a, "--first-out", b], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    assert np.fromfile(a, dtype=np.uint8).tobytes() == second.tobytes() and np.fromfile(b, dtype=np.uint8).tobytes() == first.tobytes()
    p = subprocess.run(base + ["--adaptive", "0.05"], capture_output=True, text=True)
    assert p.returncode == 1 and "needs a plain accumulation, not an adaptive one" in p.stderr
