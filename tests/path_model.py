"""The device estimator, replayed in numpy: the one statement of what a path computes that the integrator kernels are held to, bit
for bit (include/spath_hip.h states the arithmetic operation by operation; DESIGN.md sections 5.4 to 5.9).

A hit goes through the six steps of DESIGN.md section 5.9, each a function here named after its counterpart in
spath_amd/csrc/sp_integrator.h: the turned normal, shade_normal, spec_lobe, the direct term (mis_emit, nee_light, smooth_light_ok),
the bounce (spec_reflect or the diffuse direction) and, backward, spec_unwind.  Closest hits of path and shadow rays go through the
oracle's strict scan (O.closest_hits; a shadow ray is occluded iff the closest hit that skips its source triangle lies below tmax),
draws and diffuse directions through the oracle's device math, every other step in f32 in the stated order.

A table that is not given (spec, vn) means that its step is not executed, as in a kernel instantiated without SpecArgs or NormArgs;
a table of zeros executes the step.  The tests compare the two.

Not a test module: tests/test_hip_nee.py, test_hip_mis.py, test_hip_specular.py and test_hip_smooth.py hold the kernels to it,
tests/test_path_model.py pins its output on the CPU."""
import numpy as np

from oracle import oracle as O
from spath_amd import scene

F = np.float32
INV_PI = np.array([0x3EA2F983], np.uint32).view(F)[0]
INV_P = np.array([0x40C90FDB], np.uint32).view(F)[0]
MARGIN = F(1.0 - 2.0 ** -10)
TWO_PI = F(2.0 * np.pi)
PI_SQ = F(np.pi * np.pi)
TWO_OVER_PI = F(2.0 / np.pi)
ESTIMATORS = ("plain", "nee", "mis")


# ---------------------------------------------------------------------------------------------------------------- primitives
def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _philox(seed, pix, smp, depth):
    n = pix.size
    q = np.zeros((n, 5), np.uint32)
    q[:, 0], q[:, 1] = seed & 0xFFFFFFFF, seed >> 32
    q[:, 2], q[:, 3], q[:, 4] = pix, smp, depth
    r = O.device_math(2, q, n).reshape(n, 2)
    return r[:, 0], r[:, 1]


def _unit_vec(n, r1, r2):
    q = np.zeros((n.shape[0], 5), np.float64)
    q[:, :3], q[:, 3], q[:, 4] = n, r1, r2
    return O.device_math(3, q, n.shape[0]).reshape(-1, 3)


def _u(sxz, dist2, cos_y, ipdf):
    """mis_u: u = p_l / q, a NaN quotient (0/0, inf/inf) counting as 0"""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        u = ((PI_SQ * sxz) * dist2) / (cos_y * ipdf)
    return np.where(np.isnan(u), F(0), u).astype(F)


def light_table(tris, mats):
    """the host's table in float64: (tri, cdf, ipdf, W)"""
    tris = np.asarray(tris, F).reshape(-1, 12)
    mats = np.asarray(mats, F).reshape(-1, 6)
    idx, cdf, es_l = [], [], []
    W_ = 0.0
    for i in range(tris.shape[0]):
        e = mats[i, 3:6].astype(np.float64)
        es = (e[0] + e[1]) + e[2]
        if not es > 0.0:
            continue
        v = tris[i, :9].astype(np.float64)
        e1, e2 = v[3:6] - v[0:3], v[6:9] - v[0:3]
        cx = e1[1] * e2[2] - e1[2] * e2[1]
        cy = e1[2] * e2[0] - e1[0] * e2[2]
        cz = e1[0] * e2[1] - e1[1] * e2[0]
        w = (0.5 * np.sqrt((cx * cx + cy * cy) + cz * cz)) * es
        if not (w > 0.0 and np.isfinite(w)):
            continue
        W_ = W_ + w
        idx.append(i), cdf.append(W_), es_l.append(es)
    ipdf = np.array([W_ / e for e in es_l], np.float64).astype(F)
    return np.array(idx, np.int64), np.array(cdf, np.float64), ipdf, W_


# ---------------------------------------------------------------------------------------------------------------- the steps of a hit
def turned_normal(tris, idx, d):
    """step 1: the stored normal, negated where it points along the ray"""
    nrm = tris[idx, 9:12].copy()
    flip = _dot(nrm, d) > F(0)
    nrm[flip] = nrm[flip] * F(-1)
    return nrm


def shade_normal(o, d, tv, vn, nrm):
    """step 2, rules bary and interp of the header for rays (o, d) on triangles with vertices tv [k, 9], vertex normals vn [k, 9] and
    stored normals nrm (turned against d) -> (u, v, ns, sm)"""
    with np.errstate(all="ignore"):
        v0 = tv[:, 0:3]
        e1, e2 = tv[:, 3:6] - v0, tv[:, 6:9] - v0
        h = _cross(d, e2)
        a = _dot(e1, h)
        f = F(1) / a
        s = o - v0
        u = f * _dot(s, h)
        q = _cross(s, e1)
        v = f * _dot(d, q)
        w = (F(1) - u) - v
        m = (vn[:, 0:3] * w[:, None] + vn[:, 3:6] * u[:, None]) + vn[:, 6:9] * v[:, None]
        l2 = _dot(m, m)
        sm = (l2 > F(0)) & np.isfinite(l2)
        ns = nrm.copy()
        k = np.flatnonzero(sm)
        if k.size:
            nk = (m[k] / np.sqrt(l2[k])[:, None]).astype(F)
            fl = _dot(nk, nrm[k]) < F(0)
            nk[fl] = nk[fl] * F(-1)
            ns[k] = nk
    return u, v, ns, sm


def spec_lobe(seed, pix, smp, depth, p):
    """step 3: specular iff r7 < (double)p"""
    r7, _ = _philox(seed, pix, smp, 32 + depth)
    return r7 < p.astype(np.float64)


def mis_emit(tris, mats, tip, idx, d, dist, weighted):
    """step 4, the BSDF direction's emission: e_d / (1 + u_b) at the hits `weighted` whose triangle is in the light table, else e_d"""
    De = mats[idx, 3:6].copy()
    w = np.flatnonzero(weighted & (tip[idx] > F(0)))
    if w.size:
        db = d[w]
        cyb = np.abs(_dot(db, tris[idx[w], 9:12]))
        sxzb = np.sqrt(db[:, 0] * db[:, 0] + db[:, 2] * db[:, 2])
        opu = F(1) + _u(sxzb, dist[w] * dist[w], cyb, tip[idx[w]])
        De[w] = De[w] / opu[:, None]
    return De


def smooth_light_ok(sm, wd, nrm):
    """a smooth hit takes no light from below its stored normal"""
    return ~sm | (_dot(wd, nrm) > F(0))


def nee_light(tris, mats, light, seed, pix, smp, depth, x, n, idx, mis):
    """step 4, one light sample per hit at x with the normal n on triangle idx -> (ok: a shadow ray is to be traced, wd, tmax, L: what it
    carries when nothing occludes it).  MIS: L carries the balance heuristic's weight and sxz = 0 is no early-out"""
    lt, cdf, ipdf, Wt = light[:4]
    r3, r4 = _philox(seed, pix, smp, 8 + depth)
    r5, _ = _philox(seed, pix, smp, 16 + depth)
    e = np.minimum(np.searchsorted(cdf, r5 * Wt, side="right"), lt.size - 1)
    li = lt[e]
    v0 = tris[li, 0:3]
    e1, e2 = tris[li, 3:6] - v0, tris[li, 6:9] - v0
    ua, ub = np.sqrt(r3).astype(F), r4.astype(F)
    y = (v0 + e1 * (ua * (F(1) - ub))[:, None]) + e2 * (ua * ub)[:, None]
    w = y - x
    dist2 = _dot(w, w)
    ok = (li != idx) & (dist2 > F(0))
    with np.errstate(divide="ignore", invalid="ignore"):
        dd = np.sqrt(dist2)
        wd = w / dd[:, None]
        cx = _dot(wd, n)
        cy = np.abs(_dot(wd, tris[li, 9:12]))                   # the emitter keeps its stored normal
        sxz = np.sqrt(wd[:, 0] * wd[:, 0] + wd[:, 2] * wd[:, 2])
        ok &= (cx > F(0)) & (cy > F(0))
        if mis:
            g = (TWO_PI * cx) / (F(1) + _u(sxz, dist2, cy, ipdf[e]))
        else:
            ok &= sxz > F(0)
            g = (((cx * cy) / dist2) * ipdf[e]) * (TWO_OVER_PI / sxz)
        L = (mats[idx, 0:3] * INV_PI) * (mats[li, 3:6] * g[:, None])
    return ok, wd, dd * MARGIN, L


def spec_reflect(d, n):
    """step 5, the mirror direction dir - n * (c + c), not renormalised -> (nd, c)"""
    c = _dot(d, n)
    t = c + c
    return (d - n * t[:, None]).astype(F), c


def spec_unwind(q, sl, e, brdf, rec, ct):
    """step 6 with a specular table q: E + (ks * rec) * (1 / p) after a mirror lobe, else the reference's expression scaled by
    1 / (1 - p)"""
    p = q[:, 3]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        wS = (F(1) / p)[:, None]
        wD = (F(1) / (F(1) - p))[:, None]
        dif = e + (((brdf * rec) * ct[:, None]) * INV_P) * wD
        spe = e + (q[:, 0:3] * rec) * wS
    return np.where(sl[:, None], spe, dif).astype(F)


# ---------------------------------------------------------------------------------------------------------------- the estimator
def samples(rays, tris, mats, seed, s0, n, est, spec=None, vn=None, first_ns=None, collect=()):
    """-> (rec, scans, info): the radiance [npix, n, 3] of global samples s0 .. s0 + n - 1 under the estimator est ("plain", "nee":
    light samples at the first four hits, emission at the camera's hit only, "mis": NEE|MIS), the scans (path + shadow) they take, and
    what the samples met.  spec [N, 4], vn [N, 9]: the specular table and the vertex normals; None: the flag is not set.
    info: "samples"; "hits" and, of those, "sm" with a shading normal; "spec_then_hit" samples with a specular bounce whose ray hit
    something, "emitter_after_spec" samples that reached an emitter directly after one; paths "ended_diffuse" and "ended_mirror" by
    the rules of smooth shading; "lights" drawn and, of those, "lights_cut" by the geometric guard.  collect: "accepts" adds the list
    of (o, d, triangle) of every hit the float test accepted, path and shadow rays alike, "inexact" the set of triangles with a
    smooth hit whose ns is not n bitwise.
    first_ns: a list that receives (pixel, ns) of every sample's first hit (the G-buffer's normal)"""
    if est not in ESTIMATORS:
        raise ValueError(f"unknown estimator {est!r}")
    if est == "nee" and (spec is not None or vn is not None):
        raise ValueError("plain NEE takes no specular table and no vertex normals (the library refuses the flags together)")
    tris = np.ascontiguousarray(tris, F).reshape(-1, 12)
    mats = np.ascontiguousarray(mats, F).reshape(-1, 6)
    rays = np.ascontiguousarray(rays, F).reshape(-1, 6)
    spec = None if spec is None else np.ascontiguousarray(spec, F).reshape(-1, 4)
    vn = None if vn is None else np.ascontiguousarray(vn, F).reshape(-1, 9)
    mis = est == "mis"
    light = None if est == "plain" else (scene.light_table if mis else light_table)(tris, mats)      # NEE keeps the float64 table above
    tip = light[4] if mis else None
    nhits = 4 if est == "nee" else 5
    npix = rays.shape[0]
    P = npix * n
    pix = np.repeat(np.arange(npix, dtype=np.uint32), n)
    smp = np.tile(np.arange(s0, s0 + n, dtype=np.uint32), npix)
    o, d = rays[pix, :3].copy(), rays[pix, 3:].copy()
    src = np.full(P, -1, np.int32)
    alive = np.ones(P, bool)
    hidx = np.full((nhits, P), -1, np.int64)
    hct = np.zeros((nhits, P), F)
    hspec = np.zeros((nhits, P), bool)
    E = np.zeros((nhits, P, 3), F)
    prev_spec = np.zeros(P, bool)
    spec_then_hit = np.zeros(P, bool)
    emit_after_spec = np.zeros(P, bool)
    info = {"samples": P, "hits": 0, "sm": 0, "ended_diffuse": 0, "ended_mirror": 0, "lights": 0, "lights_cut": 0}
    if "accepts" in collect:
        info["accepts"] = []
    if "inexact" in collect:
        info["inexact"] = set()
    scans = 0
    for depth in range(nhits):
        a = np.flatnonzero(alive)
        if a.size == 0:
            break
        scans += a.size
        idx, dist = O.closest_hits(np.concatenate([o[a], d[a]], 1), tris, src[a])
        hit = idx >= 0
        alive[a[~hit]] = False
        a, idx, dist = a[hit], idx[hit].astype(np.int64), dist[hit]
        info["hits"] += a.size
        if "accepts" in collect:
            info["accepts"].append((o[a].copy(), d[a].copy(), idx.copy()))
        ps = prev_spec[a]
        spec_then_hit[a[ps]] = True
        emit_after_spec[a[ps & (mats[idx, 3:6].astype(np.float64).sum(1) > 0)]] = True
        # 1, 2: the turned normal and the shading normal
        nrm = turned_normal(tris, idx, d[a])
        x = o[a] + d[a] * dist[:, None]
        ns, sm = nrm, None
        if vn is not None:
            _, _, ns, sm = shade_normal(o[a], d[a], tris[idx, 0:9], vn[idx], nrm)
            info["sm"] += int(sm.sum())
            if "inexact" in collect:
                info["inexact"] |= set(idx[sm & (_bits(ns) != _bits(nrm)).any(1)].tolist())
        if depth == 0 and first_ns is not None:
            first_ns.append((pix[a], ns.copy()))
        # 3: the lobe
        sl = None if spec is None else spec_lobe(seed, pix[a], smp[a], depth, spec[idx, 3])
        # 4: the direct term.  MIS: the emission in full at the camera's hit and after a mirror bounce, else weighted; plain NEE: the
        # camera's hit alone emits
        if mis:
            De = mis_emit(tris, mats, tip, idx, d[a], dist, ~ps if depth > 0 else np.zeros(a.size, bool))
        else:
            De = mats[idx, 3:6] if est == "plain" or depth == 0 else np.zeros((a.size, 3), F)
        if light is not None and depth < 4:
            L = np.zeros((a.size, 3), F)
            if light[0].size:
                ok, wd, tmax, Lc = nee_light(tris, mats, light, seed, pix[a], smp[a], depth, x, ns, idx, mis)
                if sl is not None:
                    ok &= ~sl                                               # a specular hit draws no light sample
                    with np.errstate(divide="ignore", invalid="ignore"):
                        Lc = Lc * (F(1) / (F(1) - spec[idx, 3]))[:, None]   # L_d wD
                if sm is not None:
                    with np.errstate(invalid="ignore"):
                        cut = ok & ~smooth_light_ok(sm, wd, nrm)
                    ok &= ~cut
                    info["lights_cut"] += int(cut.sum())
                    info["lights"] += int(cut.sum())
                k = np.flatnonzero(ok)
                info["lights"] += k.size
                scans += k.size
                if k.size:
                    sidx, sd = O.closest_hits(np.concatenate([x[k], wd[k]], 1), tris, idx[k].astype(np.int32))
                    vis = ~((sidx >= 0) & (sd < tmax[k]))
                    if "accepts" in collect:
                        info["accepts"].append((x[k][sidx >= 0], wd[k][sidx >= 0], sidx[sidx >= 0].astype(np.int64)))
                    L[k[vis]] = Lc[k[vis]]
            De = De + L
        E[depth, a] = De
        # 5: the bounce; under smooth shading one that leaves the upper side of the stored normal ends the path
        nd = np.zeros((a.size, 3), F)
        ct = np.zeros(a.size, F)
        ended = np.zeros(a.size, bool)
        df = np.arange(a.size)
        if sl is not None:
            mr, df = np.flatnonzero(sl), np.flatnonzero(~sl)
            nd[mr], c = spec_reflect(d[a[mr]], ns[mr])
            if sm is not None:
                ended[mr] = sm[mr] & (~(c < F(0)) | (_dot(nd[mr], nrm[mr]) < F(0)))
                info["ended_mirror"] += int(ended[mr].sum())
        if df.size:
            r1, r2 = _philox(seed, pix[a[df]], smp[a[df]], depth)
            nd[df] = _unit_vec(ns[df], r1, r2)
            ct[df] = _dot(nd[df], ns[df])
            if sm is not None:
                ended[df] = sm[df] & (_dot(nd[df], nrm[df]) < F(0))
                info["ended_diffuse"] += int(ended[df].sum())
        hct[depth, a] = ct
        hidx[depth, a] = idx
        if sl is not None:
            hspec[depth, a] = sl
            prev_spec[a] = sl
        o[a], d[a], src[a] = x, nd, idx.astype(np.int32)
        alive[a[ended]] = False                                             # the hit keeps E_d; rec_{d+1} = 0; nothing more is scanned
    # 6: the unwind, one step per hit, backward
    rec = np.zeros((P, 3), F)
    for depth in range(nhits - 1, -1, -1):
        h = np.flatnonzero(hidx[depth] >= 0)
        i = hidx[depth, h]
        brdf = mats[i, 0:3] * INV_PI
        if spec is None:
            rec[h] = E[depth, h] + ((brdf * rec[h]) * hct[depth, h][:, None]) * INV_P
        else:
            rec[h] = spec_unwind(spec[i], hspec[depth, h], E[depth, h], brdf, rec[h], hct[depth, h])
    info["spec_then_hit"], info["emitter_after_spec"] = int(spec_then_hit.sum()), int(emit_after_spec.sum())
    return rec.reshape(npix, n, 3), scans, info


def render(rays, tris, mats, n, seed, est, spec=None, vn=None, first_ns=None, collect=()):
    """-> (rgba [npix, 4] u8, mean [npix, 3] f32, scans, info) of a one-shot render of n samples under `samples`' estimator"""
    rec, scans, info = samples(rays, tris, mats, seed, 0, n, est, spec, vn, first_ns, collect)
    acc = np.zeros((rec.shape[0], 3), F)
    for s in range(n):
        acc = acc + rec[:, s]
    mean = acc * F(1.0 / n)
    c = np.clip(mean, F(0), F(1)) * F(255) + F(0.5)
    q = np.where(c < 0, 0, np.where(c > 255, 255, c.astype(np.uint32) & 0xFF)).astype(np.uint8)
    rgba = np.zeros((rec.shape[0], 4), np.uint8)
    rgba[:, :3] = q
    return rgba, mean, scans, info
