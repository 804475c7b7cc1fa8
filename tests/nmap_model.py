"""Normal mapping (include/spath_hip.h "normal mapping"), restated in numpy: the tangent frame of a hit and the
map's normal in it, in f32 with every operation rounded on its own and in the header's order.  perturb is the device function
nmap_normal (spath_amd/csrc/sp_integrator.h, selftest 13); the UV of the hit and the bilinear sample are texture_model's, unchanged.

samples and render are path_model's with the step in place: for the duration of one call path_model.shade_normal is a function that
runs the original and then perturb, so that path_model stays the one walker of a path.

Not a test module: tests/test_hip_normal_map.py holds the kernels and this model to each other."""
import numpy as np

import path_model
import texture_model as tm
from model_primitives import F, _cross, _dot

# why a hit kept its normal: the first guard of the header's list that failed (0: it was perturbed)
PERTURBED, UNTEXTURED, DET, LT, FLAT_TEXEL, MZ, LP, BELOW, GRAZING = range(9)
GUARDS = ("perturbed", "untextured", "det", "lt", "flat_texel", "mz", "lp", "below", "grazing")


def perturb(nmap, o, d, tv, uvr, nrm, ns, sm):
    """the step for rays (o, d) on triangles with vertices tv [k, 9] and UV rows uvr [k, 6]; nrm: the stored normals turned against d;
    ns, sm: what shade_normal left -> (s, t, ns, sm, why); why[k] is PERTURBED or the first guard that kept ns[k], sm[k] as they were"""
    nmap = np.asarray(nmap, F)
    o, d, tv, uvr, nrm, ns = (np.asarray(x, F) for x in (o, d, tv, uvr, nrm, ns))
    sm = np.asarray(sm, bool)
    k = o.shape[0]
    s, t = tm.hit_uv(o, d, tv, uvr)
    tx = tm.textured(uvr, s, t)
    m = np.ones((k, 3), F)
    q = np.flatnonzero(tx)
    if q.size:
        m[q] = tm.sample(nmap, s[q], t[q])
    with np.errstate(all="ignore"):
        v0 = tv[:, 0:3]
        e1, e2 = tv[:, 3:6] - v0, tv[:, 6:9] - v0
        ds1, ds2 = uvr[:, 2] - uvr[:, 0], uvr[:, 4] - uvr[:, 0]
        dt1, dt2 = uvr[:, 3] - uvr[:, 1], uvr[:, 5] - uvr[:, 1]
        det = ds1 * dt2 - ds2 * dt1
        sg = np.where(det < F(0), F(-1), F(1)).astype(F)
        T = (e1 * dt2[:, None] - e2 * dt1[:, None]) * sg[:, None]
        B = (e2 * ds1[:, None] - e1 * ds2[:, None]) * sg[:, None]
        Tp = T - ns * _dot(ns, T)[:, None]
        lt = _dot(Tp, Tp)
        Tn = Tp / np.sqrt(lt)[:, None]
        C = _cross(ns, Tn)
        h = np.where(_dot(C, B) < F(0), F(-1), F(1)).astype(F)
        Bn = C * h[:, None]
        p = (Tn * m[:, 0:1] + Bn * m[:, 1:2]) + ns * m[:, 2:3]
        lp = _dot(p, p)
        npn = (p / np.sqrt(lp)[:, None]).astype(F)
        ok = [tx, (det > F(0)) | (det < F(0)), (lt > F(0)) & np.isfinite(lt), ~((m[:, 0] == F(0)) & (m[:, 1] == F(0))), m[:, 2] > F(0),
              (lp > F(0)) & np.isfinite(lp), _dot(npn, nrm) > F(0), _dot(d, npn) < F(0)]
    assert all(x.dtype == F for x in (det, T, B, Tp, lt, Tn, C, Bn, p, lp, npn))
    why = np.zeros(k, np.int64)
    for code in range(len(ok), 0, -1):                # the first failing guard wins
        why[~ok[code - 1]] = code
    hit = why == PERTURBED
    return s, t, np.where(hit[:, None], npn, ns).astype(F), sm | hit, why


def samples(rays, tris, mats, seed, s0, n, est, nmap, uv, spec=None, vn=None, glass=None, env=None, rough=None, first_ns=None, collect=(),
            counts=None, _walk=path_model.samples):
    """path_model.samples under SPHIP_FLAG_NORMAL_MAP with the map nmap [nh, nw, 3] and the UV table uv [N, 6].  vn None: the zeros a
    normal-mapped kernel shades with.  counts: a dict that receives the hits per entry of GUARDS"""
    tris = np.ascontiguousarray(tris, F).reshape(-1, 12)
    uv = np.ascontiguousarray(uv, F).reshape(-1, 6)
    rows = {tris[i, :9].tobytes(): i for i in range(tris.shape[0])}
    assert len(rows) == tris.shape[0], "the scene's triangles must be distinct: a hit is found by its nine vertex floats"
    if vn is None:
        vn = np.zeros((tris.shape[0], 9), F)
    original = path_model.shade_normal

    def mapped(o, d, tv, vnr, nrm):
        u, v, ns, sm = original(o, d, tv, vnr, nrm)
        idx = np.fromiter((rows[np.ascontiguousarray(r).tobytes()] for r in tv), np.int64, tv.shape[0])
        _, _, ns, sm, why = perturb(nmap, o, d, tv, uv[idx], nrm, ns, sm)
        if counts is not None:
            for code, name in enumerate(GUARDS):
                counts[name] = counts.get(name, 0) + int((why == code).sum())
        return u, v, ns, sm

    path_model.shade_normal = mapped
    try:
        return _walk(rays, tris, mats, seed, s0, n, est, spec, vn, glass, env, rough, first_ns, collect)
    finally:
        path_model.shade_normal = original


def render(rays, tris, mats, n, seed, est, nmap, uv, spec=None, vn=None, glass=None, env=None, rough=None, first_ns=None, collect=(),
           counts=None):
    """path_model.render of the same -> (rgba, mean, scans, info)"""
    original = path_model.samples
    path_model.samples = lambda r, t, m, sd, s0, k, e, *a: samples(r, t, m, sd, s0, k, e, nmap, uv, *a, counts=counts)
    try:
        return path_model.render(rays, tris, mats, n, seed, est, spec, vn, glass, env, rough, first_ns, collect)
    finally:
        path_model.samples = original
