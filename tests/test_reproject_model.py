"""tests/reproject_model.py (the numpy statement of temporal reprojection) held to closed forms, on the CPU:
a view reprojects onto itself, a sideways move shifts a facing wall by whole pixels, one hand-made case per reason code, the cap, the
bits of the blend without history, and the rules of the parameters."""
import numpy as np
import pytest

import reproject_model as M
from hip_checks import MOVES
from model_primitives import F
from spath_amd import scene, view

W, H = 24, 16
U = 2.0 ** -24                                                   # unit roundoff of f32


def cameras(w=W, h=H):
    """the default camera, the one of hip_checks.cam_rays after its move, and after its move and its turn"""
    a, b, c = view.Camera(w, h), view.Camera(w, h), view.Camera(w, h)
    b.set_delta_mov(MOVES[0])
    c.set_delta_mov(MOVES[0])
    c.set_delta_rot(MOVES[1])
    return a, b, c


SCENES = {"closed_room": lambda: scene.closed_room(100), "open_clutter": lambda: scene.open_clutter(100)}


@pytest.fixture(scope="module")
def views():
    """per scene and camera: the f32 rays, their G-buffer and the pixel grid"""
    out = {}
    for name, make in SCENES.items():
        t, m = make()
        for k, cam in enumerate(cameras()):
            rays = np.ascontiguousarray(cam.get_viewport(), F)
            out[name, k] = (cam, rays, M.gbuffer(rays, t, m)[0])
    return out


def grid(w=W, h=H):
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    return x.ravel().astype(np.float64), y.ravel().astype(np.float64)


@pytest.mark.parametrize("name", sorted(SCENES))
@pytest.mark.parametrize("k", range(3))
def test_float64_form_maps_a_view_onto_itself(views, name, k):
    cam, _, g = views[name, k]
    hit = g["mat"] >= 0
    assert hit.sum() > W * H // 4
    cz, fx, fy = M.project(M.viewport64(cam)[hit], g["dist"][hit], cam, np.float64)
    x, y = grid()
    assert (cz > 0).all()
    assert np.abs(fx - x[hit]).max() < 1e-9 and np.abs(fy - y[hit]).max() < 1e-9


@pytest.mark.parametrize("name", sorted(SCENES))
@pytest.mark.parametrize("k", range(3))
def test_f32_form_maps_a_view_onto_itself_within_its_rounding(views, name, k):
    """The bound, in pixels, to first order in u = 2^-24, for a frame whose steps are s = 1 / H in both directions.

    R bounds every world-space magnitude of the chain (|pos|, |P| and |P - pos| by their 1-norms, and the hit distance).  Errors in c, the
    hit point in the previous camera's space, each at most k u R:
        the ray's origin: rel_move of the plane point (2 stages x 3 roundings on at most sqrt(2) x_max) and + pos (1)      <=  1 + 9 x_max / R  <= 10
        the ray's direction: 3 squares, 2 sums, sqrt, 3 quotients, rel_move (6 sqrt(2)): at most 18 u, times the distance   18
        P = o + d * dist (2), v = P - pos (1)                                                                                3
        the two inverse rotations: 2 stages x 3 roundings x sqrt(2)                                                          9
        the rotations are built from f32 cos and sin: |cos^2 + sin^2 - 1| <= 2 u per rotation, forward and inverse          8
    so |dc| <= 48 u R.  qz >= focal, |sx| <= x_max for a pixel of the frame:
        |dsx| <= |dc| (focal / qz) + |sx| |dc| / qz + 3 u |sx|  <=  48 u R (1 + x_max / focal) + 3 u x_max
    The plane point of pixel x itself carries 3 roundings on x_max, xo - sx one more, the division one on fx <= W:
        |fx - x| <= (48 u R (1 + x_max / focal) + 7 u x_max) / s + u W"""
    cam, rays, g = views[name, k]
    hit = g["mat"] >= 0
    cz, fx, fy = M.project(rays[hit], g["dist"][hit], cam, F)
    assert fx.dtype == F and fy.dtype == F
    P = rays[hit, :3].astype(np.float64) + rays[hit, 3:6].astype(np.float64) * g["dist"][hit].astype(np.float64)[:, None]
    pos1 = float(np.abs(cam.pos.astype(np.float64)).sum())
    R = max(float(np.abs(P).sum(1).max()) + pos1, float(g["dist"][hit].max()))
    x_max, s, focal = (W / H) / 2.0, 1.0 / H, float(cam.focal)
    bound = (48 * U * R * (1 + x_max / focal) + 7 * U * x_max) / s + U * W
    x, y = grid()
    ex, ey = np.abs(fx.astype(np.float64) - x[hit]).max(), np.abs(fy.astype(np.float64) - y[hit]).max()
    print(f"{name} camera {k}: R = {R:.2f}, bound {bound:.3e} pixels, measured {ex:.3e} {ey:.3e}")
    assert bound < 0.01                                          # far below what a bilinear footprint notices
    assert (cz > 0).all() and ex <= bound and ey <= bound


def wall(z=5.0, half=200.0):
    """a wall facing the default camera: one triangle in the plane z that covers the frame (no inner edge for a ray to slip through)"""
    tris = np.array([(-half, -half, z) + (half, -half, z) + (0, half, z) + (0, 0, -1)], F)
    mats = np.array([[0.5, 0.5, 0.5, 0, 0, 0]], F)
    return tris, mats


@pytest.mark.parametrize("k", (1, 3, -2))
def test_a_sideways_move_of_k_pixel_steps_shifts_a_facing_wall_by_k_pixels(k):
    """Default camera at z = -3 with focal 2 and the wall at z = 5: a point of the wall is 8 in front of the view plane, so a sideways
    move by D shifts its image by D * focal / (8 + focal) = D / 5; k pixel steps of 1 / h are D = 5 k / h.  Moved along +x, the new
    view's pixel x sees what the old view's pixel x - k saw (the plane coordinate falls as x grows)."""
    w, h = 12, 16
    t, m = wall()
    prev, cur = view.Camera(w, h), view.Camera(w, h)
    cur.set_delta_mov((5.0 * k / h, 0.0, 0.0))
    gp = M.gbuffer(np.ascontiguousarray(prev.get_viewport(), F), t, m)[0]
    gc = M.gbuffer(np.ascontiguousarray(cur.get_viewport(), F), t, m)[0]
    assert (gp["mat"] == 0).all() and (gc["mat"] == 0).all()
    n = w * h
    mean_prev = np.stack([np.arange(n), np.arange(n) * 2.0, np.full(n, 7.0)], 1).astype(F)
    hist_prev = (1 + np.arange(n) % 5).astype(F)
    mean, hist, code, tap, tapq, (fx, fy) = M.reproject((1e9, 0.5, 0.01), prev, w, h, M.viewport64(cur), gc, M.viewport64(prev), gp, mean_prev,
                                                        hist_prev, T=np.float64)
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    x, y = x.ravel(), y.ravel()
    assert np.abs(fx - (x - k)).max() < 1e-5 and np.abs(fy - y).max() < 1e-5
    src = x - k
    inside = (src >= 0) & (src < w)
    assert (code[inside] == M.TAKEN).all()
    assert (code[(src < -1) | (src > w)] == M.REJECTED).all()
    q = y[inside] * w + src[inside]
    assert np.abs(mean[inside] - mean_prev[q]).max() < 1e-2 and np.abs(hist[inside] - hist_prev[q]).max() < 1e-3


# ---------------------------------------------------------------------------------------------------------------- one case per code
def hand(**over):
    """A 2 x 2 frame of the default camera facing the wall z = 5, every pixel with a history of 4; pixel 0 of the current view is then
    set by the caller.  Its hit point (1.25, 1.25, 5) is the previous pixel 0's, exactly: c = (1.25, 1.25, 8), qz = 10, sx = sy = 0.25,
    xo = yo = 0.25, so fx = fy = 0, tx = ty = 0: tap (0, 0) has weight 1 and the three others weight 0."""
    w = h = 2
    cam = view.Camera(w, h)
    rays_prev = np.ascontiguousarray(cam.get_viewport(), F)
    gp = np.zeros(4, M.GBUF)
    gp["n"], gp["mat"] = (0, 0, -1), 0
    gp["dist"] = ((F(5) - rays_prev[:, 2]) / rays_prev[:, 5]).astype(F)
    gc = gp.copy()
    rays_cur = rays_prev.copy()
    rays_cur[0] = (1.25, 1.25, 0, 0, 0, 1)
    gc["dist"][0] = 5
    s = {"params": (8.0, 0.5, 0.01), "rays_cur": rays_cur, "gc": gc, "rays_prev": rays_prev, "gp": gp,
         "mean_prev": np.arange(12, dtype=F).reshape(4, 3) + F(1), "hist_prev": np.full(4, 4, F), "cam": cam}
    for key, (field, value) in over.items():
        if field is None:
            s[key][0] = value
        else:
            s[key][field][0] = value
    mean, hist, code, tap, tapq, f = M.reproject(s["params"], s["cam"], w, h, s["rays_cur"], s["gc"], s["rays_prev"], s["gp"], s["mean_prev"],
                                                 s["hist_prev"])
    return mean[0], hist[0], code[0], list(tap[0]), s


def test_taken_and_weight():
    mean, hist, code, tap, s = hand()
    assert code == M.TAKEN and tap == [M.COUNTED, M.WEIGHT, M.WEIGHT, M.WEIGHT]
    assert mean.tobytes() == s["mean_prev"][0].tobytes() and hist == F(4)


def nothing(mean, hist):
    return mean.tobytes() == np.zeros(3, F).tobytes() and hist.tobytes() == F(0).tobytes()


def test_miss():
    mean, hist, code, tap, _ = hand(gc=("mat", -1))
    assert code == M.MISS and tap == [M.NOT_VISITED] * 4 and nothing(mean, hist)


def test_behind():
    mean, hist, code, tap, _ = hand(rays_cur=(None, (0, 0, -4, 0, 0, 1)), gc=("dist", 0))      # c.z = -1
    assert code == M.BEHIND and tap == [M.NOT_VISITED] * 4 and nothing(mean, hist)


def test_nonfinite():
    mean, hist, code, tap, _ = hand(rays_cur=(None, (0, 0, 0, 3e38, 0, 1)), gc=("dist", 1))    # c.x * focal overflows, c.z = 4
    assert code == M.NONFINITE and tap == [M.NOT_VISITED] * 4 and nothing(mean, hist)


def test_outside():
    mean, hist, code, tap, _ = hand(rays_cur=(None, (100, 1.25, 0, 0, 0, 1)))
    assert code == M.REJECTED and tap == [M.OUTSIDE] * 4 and nothing(mean, hist)
    # a footprint half on the frame: c.x = 2.5, sx = 0.5, fx = -0.5 keeps the column x = 0 alone
    mean, hist, code, tap, s = hand(rays_cur=(None, (2.5, 1.25, 0, 0, 0, 1)))
    assert code == M.TAKEN and tap == [M.OUTSIDE, M.COUNTED, M.OUTSIDE, M.WEIGHT] and mean.tobytes() == s["mean_prev"][0].tobytes()


def test_nohist():
    mean, hist, code, tap, _ = hand(hist_prev=(None, 0))
    assert code == M.REJECTED and tap[0] == M.NOHIST and nothing(mean, hist)


def test_mat():
    mean, hist, code, tap, _ = hand(gp=("mat", 7))
    assert code == M.REJECTED and tap[0] == M.MAT and nothing(mean, hist)


def test_normal():
    mean, hist, code, tap, _ = hand(gc=("n", (1, 0, 0)))
    assert code == M.REJECTED and tap[0] == M.NORMAL and nothing(mean, hist)
    assert hand(gc=("n", (0, np.sqrt(0.75), -0.5)))[2] == M.TAKEN                              # dot3 = 0.5 >= normal_min: the bound counts


def test_plane():
    mean, hist, code, tap, s = hand(gp=("dist", 9.5))                                          # the previous hit lies about 1.4 behind the wall
    assert code == M.REJECTED and tap[0] == M.PLANE and nothing(mean, hist)


def test_cap():
    assert hand(hist_prev=(None, 100))[1] == F(8)                # max_history = 8
    assert hand(hist_prev=(None, 8))[1] == F(8) and hand(hist_prev=(None, 7.5))[1] == F(7.5)
    s = hand()[4]
    s["params"] = (0.0, 0.5, 0.01)                               # a cap of 0 takes no history over: the pixel is taken with count 0
    mean, hist, code, *_ = M.reproject(s["params"], s["cam"], 2, 2, s["rays_cur"], s["gc"], s["rays_prev"], s["gp"], s["mean_prev"], s["hist_prev"])
    assert code[0] == M.TAKEN and hist[0].tobytes() == F(0).tobytes()


def test_blend_without_history_is_the_plain_resolve_in_bits():
    rng = np.random.default_rng(5)
    s = (rng.random((257, 3)) * 40).astype(F)
    hm = rng.random((257, 3)).astype(F)
    for n in (1, 3, 7, 1000):
        want = s * F(1.0 / n)
        assert want.dtype == F
        assert M.blend(s, n).tobytes() == want.tobytes()
        assert M.blend(s, n, hm, np.zeros(257, F)).tobytes() == want.tobytes()
        h = np.where(np.arange(257) % 3 == 0, 0, 5).astype(F)
        got = M.blend(s, n, hm, h)
        assert got[h == 0].tobytes() == want[h == 0].tobytes()
        mixed = ((F(5) * hm + s) / (F(5) + F(n))).astype(F)
        assert got[h > 0].tobytes() == mixed[h > 0].tobytes()
        pm, ph = M.history_pair(s, n, hm, h)
        assert pm.tobytes() == got.tobytes() and ph.tobytes() == (h + F(n)).tobytes()


def test_param_rules_are_the_headers():
    ok = M.check_params
    assert ok(0.0, -1.0, 0.0) == "ok" and ok(32.0, 1.0, 3.0e38) == "ok" and ok(3.0e38, 0.0, 0.0) == "ok"
    assert ok(-1e-6, 0.9, 0.02) == "max_history" and ok(np.inf, 0.9, 0.02) == "max_history" and ok(np.nan, 0.9, 0.02) == "max_history"
    assert ok(8.0, -1.0001, 0.02) == "normal_min" and ok(8.0, 1.0001, 0.02) == "normal_min" and ok(8.0, np.nan, 0.02) == "normal_min"
    assert ok(8.0, 0.9, -1e-6) == "plane_tol" and ok(8.0, 0.9, np.inf) == "plane_tol" and ok(8.0, 0.9, np.nan) == "plane_tol"
    assert ok(8.0, 0.9, 0.02, reserved=1) == "reserved"


def test_the_librarys_defaults_obey_the_rules():
    """needs the built library, not a GPU"""
    from spath_amd import capi
    d = capi.Reproject.defaults()
    assert M.check_params(d.max_history, d.normal_min, d.plane_tol, d.reserved) == "ok"
    assert d.max_history > 0 and float(d.max_history) == 2.0 ** round(np.log2(d.max_history))     # a power of two
