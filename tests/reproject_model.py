"""Temporal reprojection (include/spath_hip.h "temporal reprojection") stated in numpy operation by operation:
the reprojection of a previous view's (mean, history count) into the current view (reproject: f32, every operation rounded on its
own, the statement the kernel k_reproject is held to bit for bit; with T = np.float64 the same steps in double, for which
viewport64 gives a view's rays in double), the blend of a history
with new samples (blend), the pair an accumulation hands on (history_pair), the rules of the parameters (check_params), and a CPU
G-buffer from the oracle's closest hits (gbuffer) for the tests that have no GPU.

Every pixel gets a reason code (PIXEL_*) and every tap one of TAP_*; NOT_VISITED marks the taps of a pixel that ended before step 5.

Not a test module: tests/test_reproject_model.py holds it to closed forms, tests/test_hip_reproject.py holds the kernels to it."""
import math

import numpy as np

from model_primitives import F, _dot
from oracle import oracle as O

TAKEN, MISS, BEHIND, NONFINITE, REJECTED = range(5)              # REJECTED: step 5 was reached and no tap counted
PIXEL_CODES = ("taken", "miss", "behind", "nonfinite", "rejected")
COUNTED, OUTSIDE, WEIGHT, NOHIST, MAT, NORMAL, PLANE, NOT_VISITED = range(8)
TAP_CODES = ("counted", "outside", "weight", "nohist", "mat", "normal", "plane", "not_visited")

GBUF = np.dtype([("n", "<f4", 3), ("dist", "<f4"), ("a", "<f4", 3), ("mat", "<i4")])

# the rules of sphip_reproject, one per field: (field, lowest, highest) with both ends allowed; every value finite; reserved 0
PARAM_RULES = (("max_history", 0.0, np.finfo(np.float32).max), ("normal_min", -1.0, 1.0), ("plane_tol", 0.0, np.finfo(np.float32).max))


def check_params(max_history, normal_min, plane_tol, reserved=0):
    """-> the name of the first field that breaks its rule, or "ok" """
    for name, v, (_, lo, hi) in zip(("max_history", "normal_min", "plane_tol"), (max_history, normal_min, plane_tol), PARAM_RULES):
        v = float(np.float32(v))
        if not (np.isfinite(v) and lo <= v <= hi):
            return name
    return "ok" if int(reserved) == 0 else "reserved"


def view_consts(cam, T=F):
    """the host constants of a view.Camera -> dict (xo = x_max - h_x, yo likewise).  T = F: f32, as sphip_viewport_device forms them.
    T = np.float64: the same quantities in double, the trigonometric values from the camera's angles in double (viewport64's)"""
    W, H = cam.res_x, cam.res_y
    if T is np.float64:
        x_step, y_step = (W / H) / W, 1.0 / H
        ay, ax = float(cam.angle[1]), float(cam.angle[0])
        return {"xo": T((W / H) / 2.0 - x_step / 2.0), "x_step": T(x_step), "yo": T(0.5 - y_step / 2.0), "y_step": T(y_step),
                "focal": T(cam.focal), "pos": np.asarray(cam.pos, T).copy(), "cos_y": T(math.cos(ay)), "sin_y": T(math.sin(ay)),
                "cos_x": T(math.cos(ax)), "sin_x": T(math.sin(ax))}
    x_size = F(np.float64(W) / np.float64(H))
    y_size = F(1.0)
    x_max = F(np.float64(x_size) / 2.0)
    x_step = F(x_size / F(W))
    h_x = F(np.float64(x_step) / 2.0)
    y_max = F(np.float64(y_size) / 2.0)
    y_step = F(y_size / F(H))
    h_y = F(np.float64(y_step) / 2.0)
    return {"xo": F(x_max - h_x), "x_step": x_step, "yo": F(y_max - h_y), "y_step": y_step, "focal": F(cam.focal),
            "pos": np.asarray(cam.pos, F).copy(), "cos_y": F(cam.cosY), "sin_y": F(cam.sinY), "cos_x": F(cam.cosX), "sin_x": F(cam.sinX)}


def gbuffer(rays, tris, mats):
    """the G-buffer of sphip_gbuffer_device from the oracle's closest hits -> (structured array of GBUF, hit triangle or -1)"""
    rays, tris, mats = np.asarray(rays, F).reshape(-1, 6), np.asarray(tris, F).reshape(-1, 12), np.asarray(mats, F).reshape(-1, 6)
    idx, dist = O.closest_hits(rays, tris, None)
    idx = np.asarray(idx, np.int64)
    first = {}
    cls = np.empty(mats.shape[0], np.int32)
    for i, row in enumerate(mats):
        cls[i] = first.setdefault(row.tobytes(), i)
    g = np.zeros(rays.shape[0], GBUF)
    g["dist"] = F(1e12)
    g["mat"] = -1
    hit = idx >= 0
    n = tris[idx[hit], 9:12].copy()
    flip = _dot(n, rays[hit, 3:6]) > F(0)
    n[flip] = n[flip] * F(-1)
    g["n"][hit] = n
    g["dist"][hit] = np.asarray(dist, F)[hit]
    g["a"][hit] = mats[idx[hit], :3]
    g["mat"][hit] = cls[idx[hit]]
    return g, np.where(hit, idx, -1)


def _project(P, v, T):
    """steps 3 and 4 in the float type T (F or np.float64) -> (c.z, fx, fy)"""
    pos = v["pos"].astype(T)
    cy, sy, cx, sx_ = T(v["cos_y"]), T(v["sin_y"]), T(v["cos_x"]), T(v["sin_x"])
    focal = T(v["focal"])
    d = P.astype(T) - pos
    ax, ay, az = d[:, 0] * cy + d[:, 2] * -sy, d[:, 1], d[:, 0] * sy + d[:, 2] * cy
    c0, c1, c2 = ax, ay * cx + az * sx_, ay * -sx_ + az * cx
    qz = c2 + focal
    sx, sy2 = (c0 * focal) / qz, (c1 * focal) / qz
    fx, fy = (T(v["xo"]) - sx) / T(v["x_step"]), (T(v["yo"]) - sy2) / T(v["y_step"])
    assert all(x.dtype == T for x in (d, ax, az, c1, c2, qz, sx, sy2, fx, fy))
    return c2, fx, fy


def viewport64(cam):
    """view.Camera.get_viewport in float64, with the trigonometric values of the angles in double -> rays [h*w, 6]"""
    v = view_consts(cam, np.float64)
    i, j = np.meshgrid(np.arange(cam.res_x, dtype=np.float64), np.arange(cam.res_y, dtype=np.float64))
    cur = np.stack([v["xo"] - v["x_step"] * i.ravel(), v["yo"] - v["y_step"] * j.ravel(), np.zeros(i.size)], 1)
    t = cur + np.array([0.0, 0.0, v["focal"]])
    d = t / np.sqrt(_dot(t, t))[:, None]

    def rel_move(a):                                             # rY(rX(.))
        x, y, z = a[:, 0], a[:, 1] * v["cos_x"] + a[:, 2] * -v["sin_x"], a[:, 1] * v["sin_x"] + a[:, 2] * v["cos_x"]
        return np.stack([x * v["cos_y"] + z * v["sin_y"], y, x * -v["sin_y"] + z * v["cos_y"]], 1)
    return np.concatenate([rel_move(cur) + v["pos"], rel_move(d)], 1)


def project(rays_cur, dist, cam_prev, T=F):
    """steps 2-4 in the float type T for rays with a hit at distance dist -> (c.z, fx, fy)"""
    r, t = np.asarray(rays_cur).reshape(-1, 6).astype(T), np.asarray(dist).reshape(-1).astype(T)
    with np.errstate(all="ignore"):
        return _project((r[:, :3] + r[:, 3:6] * t[:, None]).astype(T), view_consts(cam_prev, T), T)


def reproject(params, cam_prev, w, h, rays_cur, gbuf_cur, rays_prev, gbuf_prev, mean_prev, hist_prev, T=F):
    """steps 1-6 -> (mean [n, 3], hist [n], pixel code [n], tap code [n, 4] in visiting order, tap pixel [n, 4] or -1, (fx, fy)).
    params = (max_history, normal_min, plane_tol).  T = F is the statement of the kernel (f32 inputs); T = np.float64 the same steps in double (rays of any float type)"""
    n = w * h
    max_history, normal_min, plane_tol = (T(F(x)) for x in params)
    rays_cur, rays_prev = np.asarray(rays_cur).reshape(n, 6).astype(T), np.asarray(rays_prev).reshape(n, 6).astype(T)
    mean_prev, hist_prev = np.asarray(mean_prev, F).reshape(n, 3).astype(T), np.asarray(hist_prev, F).reshape(n).astype(T)
    np_, distp, matp = gbuf_cur["n"].astype(T), gbuf_cur["dist"].astype(T), gbuf_cur["mat"].astype(np.int64)
    nq_all, distq_all, matq_all = gbuf_prev["n"].astype(T), gbuf_prev["dist"].astype(T), gbuf_prev["mat"].astype(np.int64)
    v = view_consts(cam_prev, T)
    code = np.full(n, REJECTED, np.int64)
    tap = np.full((n, 4), NOT_VISITED, np.int64)
    tapq = np.full((n, 4), -1, np.int64)
    with np.errstate(all="ignore"):
        P = (rays_cur[:, :3] + rays_cur[:, 3:6] * distp[:, None]).astype(T)                        # 2.
        cz, fx, fy = _project(P, v, T)                                                            # 3., 4.
        live = matp >= 0                                                                          # 1.
        code[~live] = MISS
        behind = live & ~(cz > T(0))
        code[behind] = BEHIND
        live &= ~behind
        nonfinite = live & ~(np.isfinite(fx) & np.isfinite(fy))
        code[nonfinite] = NONFINITE
        live &= ~nonfinite
        x0f, y0f = np.floor(fx), np.floor(fy)
        tx, ty = (fx - x0f).astype(T), (fy - y0f).astype(T)
        ux, uy = (T(1) - tx).astype(T), (T(1) - ty).astype(T)
        # a footprint wholly off the frame has four taps outside; what is left converts to an integer exactly
        near = live & (x0f >= -1) & (x0f < w) & (y0f >= -1) & (y0f < h)
        x0 = np.where(near, x0f, -2).astype(np.int64)
        y0 = np.where(near, y0f, -2).astype(np.int64)
        ptd = (plane_tol * distp).astype(T)
        Wt, C, Hs = np.zeros(n, T), np.zeros((n, 3), T), np.zeros(n, T)
        for b in (0, 1):                                                                          # 5.
            for a in (0, 1):
                k = b * 2 + a
                xx, yy = x0 + a, y0 + b
                ok = live.copy()
                inside = (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
                tap[ok & ~inside, k] = OUTSIDE
                ok &= inside
                q = np.where(ok, yy * w + xx, 0)
                tapq[ok, k] = q[ok]
                wb = ((tx if a else ux) * (ty if b else uy)).astype(T)
                tap[ok & ~(wb > 0), k] = WEIGHT
                ok &= wb > 0
                hq = hist_prev[q]
                tap[ok & ~(hq > 0), k] = NOHIST
                ok &= hq > 0
                tap[ok & (matq_all[q] != matp), k] = MAT
                ok &= matq_all[q] == matp
                dn = _dot(np_, nq_all[q])
                tap[ok & ~(dn >= normal_min), k] = NORMAL
                ok &= dn >= normal_min
                Pq = (rays_prev[q, :3] + rays_prev[q, 3:6] * distq_all[q][:, None]).astype(T)
                pd = _dot((Pq - P).astype(T), np_)
                tap[ok & ~(np.abs(pd) <= ptd), k] = PLANE
                ok &= np.abs(pd) <= ptd
                tap[ok, k] = COUNTED
                assert all(x.dtype == T for x in (wb, hq, dn, Pq, pd, ptd, P))
                Wt = np.where(ok, Wt + wb, Wt).astype(T)                                           # 6.
                C = np.where(ok[:, None], C + wb[:, None] * mean_prev[q], C).astype(T)
                Hs = np.where(ok, Hs + wb * hq, Hs).astype(T)
        taken = live & (Wt > 0)
        code[taken] = TAKEN
        mean = np.where(taken[:, None], C / Wt[:, None], T(0)).astype(T)
        hist = (Hs / Wt).astype(T)
        hist = np.where(hist > max_history, max_history, hist)
        hist = np.where(taken, hist, T(0)).astype(T)
    assert mean.dtype == T and hist.dtype == T and Wt.dtype == T and C.dtype == T and Hs.dtype == T
    return mean, hist, code, tap, tapq, (fx, fy)


def blend(s, n, hmean=None, hist=None):
    """the blend of a history with the running sum s [k, 3] of n new samples -> mean [k, 3] (f32)"""
    s = np.asarray(s, F).reshape(-1, 3)
    plain = (s * F(1.0 / n)).astype(F)
    if hist is None:
        return plain
    hm, h = np.asarray(hmean, F).reshape(-1, 3), np.asarray(hist, F).reshape(-1)
    with np.errstate(all="ignore"):
        den = (h + F(n)).astype(F)
        mixed = ((h[:, None] * hm + s) / den[:, None]).astype(F)
    assert plain.dtype == F and mixed.dtype == F and den.dtype == F
    return np.where((h == F(0))[:, None], plain, mixed).astype(F)


def history_pair(s, n, hmean=None, hist=None):
    """what an accumulation of n samples (sum s, its own history or none) hands to the next reprojection -> (mean, hist)"""
    k = np.asarray(s, F).reshape(-1, 3).shape[0]
    h = np.zeros(k, F) if hist is None else np.asarray(hist, F).reshape(-1)
    return blend(s, n, hmean, hist), (h + F(n)).astype(F)


def rgba(mean):
    """vec3::clamp and scene::vec3_RGBA of a mean [k, 3] -> uint8 [k, 4] (the oracle's device-math statement, what 5)"""
    m = np.ascontiguousarray(mean, F).reshape(-1, 3)
    return O.device_math(5, m, m.shape[0]).astype(np.uint32).view(np.uint8).reshape(-1, 4)


# ---------------------------------------------------------------------------------------------------------------- the tests' views
BASE_MOVES = ((0.1, -0.2, 0.3), (0.05, 0.1, 0.0))                # hip_checks.MOVES: the view every pair leaves (turned: sin_y, sin_x > 0)
PAIRS = {                                                        # what happens between the previous and the current view
    "identical": (),
    "subpixel_pan": (("mov", (0.004, 0.002, 0.0)),),
    "pan": (("mov", (0.3, -0.1, 0.0)),),
    "turn_off_frame": (("rot", (0.0, 0.6, 0.0)),),
    "dolly": (("mov", (0.0, 0.0, 0.8)),),
    "focal": (("focal", 0.7),),
    "facing_away": (("rot", (0.0, 3.0, 0.0)),),
}


def camera_pair(name, w, h):
    """-> (previous, current) view.Camera of the pair `name`"""
    from spath_amd import view
    cams = []
    for steps in ((), PAIRS[name]):
        cam = view.Camera(w, h)
        cam.set_delta_mov(BASE_MOVES[0])
        cam.set_delta_rot(BASE_MOVES[1])
        for kind, val in steps:
            {"mov": cam.set_delta_mov, "rot": cam.set_delta_rot, "focal": cam.set_delta_focal}[kind](val)
        cams.append(cam)
    return cams[0], cams[1]
