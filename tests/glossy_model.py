"""Glossy reflection in the numpy model (include/spath_hip.h, "glossy reflection"), operation by operation: the
GGX visible-normal draw and its Smith weight in f32 (gloss_bounce), and tests/env_model.py's loop restated with the glossy step: a hit
that took the mirror lobe of a triangle of roughness alpha > 0 (not an interface) reflects about the drawn microfacet normal, and the
unwind scales the mirror's term once more by the weight g.

rough = None means that the step is not executed and the loop is env_model.samples' (tests/test_hip_glossy.py holds them together,
bits and scans); with a table the specular, the dielectric and the environment step are executed as in the kernels, against the
tables given, tables of zeros or a black map (which is no map: the miss term is 0 and the light table is the unflagged one).

Not a test module: tests/test_hip_glossy.py holds the device function and the path kernels to it at tolerance 0."""
import numpy as np

from oracle import oracle as O
from dielectric_model import dielectric
from env_model import env_light, env_miss, flagged_light_table, lookup, scene_part, tables
from path_model import (ESTIMATORS, F, INV_P, INV_PI, _cross, _dot, _philox, _unit_vec, mis_emit, nee_light, shade_normal,
                        smooth_light_ok, spec_lobe, spec_reflect, spec_unwind, turned_normal)
from spath_amd import scene

ONE, HALF, ZERO = F(1), F(0.5), F(0)
GLOSS_STREAM = 48


def _sincos(phi):
    sc = O.device_math(0, np.ascontiguousarray(phi, F), phi.size).reshape(-1, 2)
    return sc[:, 0], sc[:, 1]


def gloss_bounce(d, ns, al, u1, u2, parts=None):
    """gloss_bounce for rays d [k, 3], shading normals ns [k, 3] (turned against d), roughness al [k] and uniforms u1, u2 [k] (float64)
    -> (m, nd, g, ok).  parts: a dict that receives the intermediate vh, T1, T2, nh"""
    d, ns, al = np.ascontiguousarray(d, F), np.ascontiguousarray(ns, F), np.ascontiguousarray(al, F)
    u1, u2 = np.asarray(u1, np.float64), np.asarray(u2, np.float64)
    with np.errstate(all="ignore"):
        c = _dot(d, ns)
        nx, ny, nz = ns[:, 0], ns[:, 1], ns[:, 2]
        sg = np.where(nz < ZERO, F(-1), ONE)
        a = F(-1) / (sg + nz)
        b = (nx * ny) * a
        t = np.stack([ONE + (sg * (nx * nx)) * a, sg * b, (-sg) * nx], 1)
        bt = np.stack([b, sg + (ny * ny) * a, -ny], 1)
        v = np.stack([-_dot(d, t), -_dot(d, bt), -c], 1)
        h = np.stack([al * v[:, 0], al * v[:, 1], v[:, 2]], 1)
        vh = h / np.sqrt(_dot(h, h))[:, None]
        l2 = vh[:, 0] * vh[:, 0] + vh[:, 1] * vh[:, 1]
        ln = np.sqrt(l2)
        pos = l2 > ZERO
        T1 = np.stack([np.where(pos, -vh[:, 1] / ln, ONE), np.where(pos, vh[:, 0] / ln, ZERO), np.zeros_like(l2)], 1).astype(F)
        T2 = _cross(vh, T1)
        r = np.sqrt(u1).astype(F)
        phi = ((u2 * np.pi) * 2.0).astype(F)
        sn, cs = _sincos(phi)
        p1 = r * cs
        p2 = r * sn
        s = HALF * (ONE + vh[:, 2])
        q = ONE - p1 * p1
        q = np.where(q > ZERO, q, ZERO)
        p2 = (ONE - s) * np.sqrt(q) + s * p2
        z2 = (ONE - p1 * p1) - p2 * p2
        z = np.sqrt(np.where(z2 > ZERO, z2, ZERO))
        nh = (T1 * p1[:, None] + T2 * p2[:, None]) + vh * z[:, None]
        ne = np.stack([al * nh[:, 0], al * nh[:, 1], np.where(nh[:, 2] > ZERO, nh[:, 2], ZERO)], 1)
        ml = ne / np.sqrt(_dot(ne, ne))[:, None]
        m = (t * ml[:, 0:1] + bt * ml[:, 1:2]) + ns * ml[:, 2:3]
        nd, _ = spec_reflect(d, m)
        cl = _dot(nd, ns)
        ok = cl > ZERO
        g = (cl + cl) / (cl + np.sqrt(al * al + (ONE - al * al) * (cl * cl)))
        g = np.where(g > ONE, ONE, g)
    for x in (vh, T1, T2, nh, m, nd, g):
        assert x.dtype == F, x.dtype
    if parts is not None:
        parts.update(vh=vh, T1=T1, T2=T2, nh=nh, t=t, bt=bt)
    return m.astype(F), nd, g, ok


def gloss_bounce64(d, ns, al, u1, u2):
    """the same formulas in float64 (sin and cos numpy's), from the same f32 inputs -> (m, nd, g, cl)"""
    d, ns, al = np.asarray(d, F).astype(np.float64), np.asarray(ns, F).astype(np.float64), np.asarray(al, F).astype(np.float64)
    u1, u2 = np.asarray(u1, np.float64), np.asarray(u2, np.float64)
    dot = lambda p, q: (p * q).sum(1)
    with np.errstate(all="ignore"):
        c = dot(d, ns)
        nx, ny, nz = ns[:, 0], ns[:, 1], ns[:, 2]
        sg = np.where(nz < 0, -1.0, 1.0)
        a = -1.0 / (sg + nz)
        b = nx * ny * a
        t = np.stack([1.0 + sg * nx * nx * a, sg * b, -sg * nx], 1)
        bt = np.stack([b, sg + ny * ny * a, -ny], 1)
        v = np.stack([-dot(d, t), -dot(d, bt), -c], 1)
        h = np.stack([al * v[:, 0], al * v[:, 1], v[:, 2]], 1)
        vh = h / np.sqrt(dot(h, h))[:, None]
        l2 = vh[:, 0] ** 2 + vh[:, 1] ** 2
        ln = np.sqrt(l2)
        pos = l2 > 0
        T1 = np.stack([np.where(pos, -vh[:, 1] / ln, 1.0), np.where(pos, vh[:, 0] / ln, 0.0), np.zeros_like(l2)], 1)
        T2 = np.cross(vh, T1)
        r = np.sqrt(u1)
        phi = u2 * np.pi * 2.0
        p1, p2 = r * np.cos(phi), r * np.sin(phi)
        s = 0.5 * (1.0 + vh[:, 2])
        p2 = (1.0 - s) * np.sqrt(np.maximum(1.0 - p1 * p1, 0.0)) + s * p2
        z = np.sqrt(np.maximum(1.0 - p1 * p1 - p2 * p2, 0.0))
        nh = T1 * p1[:, None] + T2 * p2[:, None] + vh * z[:, None]
        ne = np.stack([al * nh[:, 0], al * nh[:, 1], np.maximum(nh[:, 2], 0.0)], 1)
        ml = ne / np.sqrt(dot(ne, ne))[:, None]
        m = t * ml[:, 0:1] + bt * ml[:, 1:2] + ns * ml[:, 2:3]
        cm = dot(d, m)
        nd = d - m * (cm + cm)[:, None]
        cl = dot(nd, ns)
        g = np.minimum((cl + cl) / (cl + np.sqrt(al * al + (1.0 - al * al) * cl * cl)), 1.0)
    return m, nd, g, cl


def gloss_unwind(q, e, rec, g):
    """the unwind's step at a glossy hit: E + (((ks * rec) * wS) * g)"""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        wS = (F(1) / q[:, 3])[:, None]
        return (e + ((q[:, 0:3] * rec) * wS) * g[:, None]).astype(F)


def samples(rays, tris, mats, seed, s0, n, est, spec=None, vn=None, glass=None, env=None, rough=None):
    """env_model.samples with a roughness table rough [n_tris] (None: the flag is not set) -> (rec, scans, info).
    info: env_model's counters and "glossy" hits that took the glossy step, "alpha0" hits that took the mirror lobe on a row alpha = 0
    (not an interface), "ended" paths ended by !ok, "two_glossy" paths with two glossy hits or more, "emit_after_glossy" hits on an
    emitter and "miss_after_glossy" misses straight after a glossy hit, "ended_above" / "ended_below": smooth glossy hits ended by the
    rule !(c < 0) / dot3(nd, n) < 0"""
    if est not in ESTIMATORS:
        raise ValueError(f"unknown estimator {est!r}")
    if est == "nee" and (spec is not None or vn is not None or glass is not None or env is not None or rough is not None):
        raise ValueError("plain NEE takes no table and no environment map (the library refuses the flags together)")
    if rough is not None and spec is None:
        raise ValueError("a roughness table needs a specular table (the library refuses the flag without SPHIP_FLAG_SPECULAR)")
    tris = np.ascontiguousarray(tris, F).reshape(-1, 12)
    mats = np.ascontiguousarray(mats, F).reshape(-1, 6)
    rays = np.ascontiguousarray(rays, F).reshape(-1, 6)
    spec = None if spec is None else np.ascontiguousarray(spec, F).reshape(-1, 4)
    vn = None if vn is None else np.ascontiguousarray(vn, F).reshape(-1, 9)
    glass = None if glass is None else np.ascontiguousarray(glass, F).reshape(-1, 4)
    env = None if env is None else np.ascontiguousarray(env, F)
    rough = None if rough is None else np.ascontiguousarray(rough, F).reshape(-1)
    if (env is not None or rough is not None) and glass is None:
        glass = np.zeros((tris.shape[0], 4), F)                   # the context's table of zeros: ior = 0, no interface
    if glass is not None and spec is None:
        spec = np.zeros((tris.shape[0], 4), F)                    # the context's table of zeros: p = 0, wD = 1.0f
    mis = est == "mis"
    tab = tpdf = None
    if est == "plain":
        light = None
    elif env is not None:
        tab = tables(env)
        part = scene_part(tab, tris, mats)
        tpdf = part["tpdf"]
        light = flagged_light_table(tris, mats, part)
    else:
        from path_model import light_table
        light = (scene.light_table if mis else light_table)(tris, mats)
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
    hct = np.zeros((nhits, P), F)                                 # the cosine of a diffuse hit, g of a glossy one, 0 of any other
    hspec = np.zeros((nhits, P), bool)
    htrans = np.zeros((nhits, P), bool)
    E = np.zeros((nhits, P, 3), F)
    rec = np.zeros((P, 3), F)                                     # the unwind starts from the miss term, 0 for a path that did not leave
    prev_spec = np.zeros(P, bool)
    prev_gloss = np.zeros(P, bool)
    n_gloss = np.zeros(P, np.int64)
    info = {"samples": P, "hits": 0, "miss": [0] * 5, "miss_after_spec": 0, "miss_weighted": 0, "env_lights": 0, "env_unoccluded": 0,
            "env_occluded": 0, "tri_lights": 0, "glass": 0, "spec": 0, "glossy": 0, "alpha0": 0, "ended": 0, "two_glossy": 0,
            "emit_after_glossy": 0, "miss_after_glossy": 0, "ended_above": 0, "ended_below": 0}
    scans = 0
    for depth in range(nhits):
        a = np.flatnonzero(alive)
        if a.size == 0:
            break
        scans += a.size
        idx, dist = O.closest_hits(np.concatenate([o[a], d[a]], 1), tris, src[a])
        hit = idx >= 0
        alive[a[~hit]] = False
        info["miss_after_glossy"] += int(prev_gloss[a[~hit]].sum()) if depth > 0 else 0
        if env is not None:                                       # the miss term
            m = a[~hit]
            full = prev_spec[m] if depth > 0 else np.ones(m.size, bool)
            rec[m] = env_miss(env, tpdf, d[m], full, mis)
            info["miss"][depth] += m.size
            info["miss_after_spec"] += int(prev_spec[m].sum()) if depth > 0 else 0
            if mis:
                li_, lj_, _, ok_ = lookup(d[m], env.shape[0])
                info["miss_weighted"] += int((ok_ & ~full & (tpdf[lj_, li_] > F(0))).sum())
        a, idx, dist = a[hit], idx[hit].astype(np.int64), dist[hit]
        info["hits"] += a.size
        if depth > 0:
            es = (mats[idx, 3].astype(np.float64) + mats[idx, 4]) + mats[idx, 5]
            info["emit_after_glossy"] += int((prev_gloss[a] & (es > 0)).sum())
        ps = prev_spec[a]
        # 1, 2: the turned normal and the shading normal
        nrm = turned_normal(tris, idx, d[a])
        x = o[a] + d[a] * dist[:, None]
        ns, sm = nrm, None
        if vn is not None:
            _, _, ns, sm = shade_normal(o[a], d[a], tris[idx, 0:9], vn[idx], nrm)
        # 3: the lobe; an interface is a specular hit
        isg = np.zeros(a.size, bool) if glass is None else glass[idx, 3] > F(0)
        sl = None if spec is None else spec_lobe(seed, pix[a], smp[a], depth, spec[idx, 3])
        if glass is not None:
            sl = sl | isg
        # 4: the direct term
        if mis:
            De = mis_emit(tris, mats, tip, idx, d[a], dist, ~ps if depth > 0 else np.zeros(a.size, bool))
        else:
            De = mats[idx, 3:6] if est == "plain" or depth == 0 else np.zeros((a.size, 3), F)
        if light is not None and depth < 4:
            L = np.zeros((a.size, 3), F)
            if light[0].size:
                with np.errstate(all="ignore"):
                    ok, wd, tmax, Lc = nee_light(tris, mats, light, seed, pix[a], smp[a], depth, x, ns, idx, mis)
                is_env = np.zeros(a.size, bool)
                if env is not None and light[0][-1] < 0:          # the rows whose draw picked the map's entry
                    r5, _ = _philox(seed, pix[a], smp[a], 16 + depth)
                    e = np.minimum(np.searchsorted(light[1], r5 * light[3], side="right"), light[0].size - 1)
                    is_env = light[0][e] < 0
                    q = np.flatnonzero(is_env)
                    if q.size:
                        ok[q], wd[q], tmax[q], Lc[q], _, _ = env_light(env, tab, tpdf, mats, seed, pix[a[q]], smp[a[q]], depth, ns[q], idx[q])
                if sl is not None:
                    ok &= ~sl                                               # a specular hit draws no light sample
                    with np.errstate(divide="ignore", invalid="ignore"):
                        Lc = Lc * (F(1) / (F(1) - spec[idx, 3]))[:, None]   # L_d wD
                if sm is not None:
                    with np.errstate(invalid="ignore"):
                        ok &= smooth_light_ok(sm, wd, nrm)
                k = np.flatnonzero(ok)
                scans += k.size
                info["env_lights"] += int(is_env[k].sum())
                info["tri_lights"] += int((~is_env[k]).sum())
                if k.size:
                    sidx, sd = O.closest_hits(np.concatenate([x[k], wd[k]], 1), tris, idx[k].astype(np.int32))
                    vis = ~((sidx >= 0) & (sd < tmax[k]))
                    info["env_unoccluded"] += int((vis & is_env[k]).sum())
                    info["env_occluded"] += int((~vis & is_env[k]).sum())
                    L[k[vis]] = Lc[k[vis]]
            De = De + L
        E[depth, a] = De
        # 5: the bounce
        nd = np.zeros((a.size, 3), F)
        ct = np.zeros(a.size, F)
        ended = np.zeros(a.size, bool)
        tr = np.zeros(a.size, bool)
        isgl = np.zeros(a.size, bool)
        df = np.arange(a.size)
        if sl is not None:
            gl, mr, df = np.flatnonzero(isg), np.flatnonzero(sl & ~isg), np.flatnonzero(~sl)
            info["spec"] += mr.size
            nd[mr], c = spec_reflect(d[a[mr]], ns[mr])
            if sm is not None:
                ended[mr] = sm[mr] & (~(c < F(0)) | (_dot(nd[mr], nrm[mr]) < F(0)))
            if rough is not None:                                 # the glossy step replaces the mirror's where alpha > 0
                al = rough[idx[mr]]
                info["alpha0"] += int((~(al > F(0))).sum())
                gs = mr[al > F(0)]
                if gs.size:
                    u1, u2 = _philox(seed, pix[a[gs]], smp[a[gs]], GLOSS_STREAM + depth)
                    _, ndg, g, ok = gloss_bounce(d[a[gs]], ns[gs], rough[idx[gs]], u1, u2)
                    nd[gs] = ndg
                    ct[gs] = np.where(ok, g, F(0))
                    e_ = ~ok
                    info["ended"] += int(e_.sum())
                    if sm is not None:
                        cg = _dot(d[a[gs]], ns[gs])
                        above, below = sm[gs] & ~(cg < F(0)), sm[gs] & (_dot(ndg, nrm[gs]) < F(0))
                        info["ended_above"] += int(above.sum())
                        info["ended_below"] += int(below.sum())
                        e_ = e_ | above | below
                    ended[gs] = e_
                    isgl[gs] = True
                    info["glossy"] += gs.size
            if gl.size:
                dg, nsg = d[a[gl]], ns[gl]
                entering = ~(_dot(tris[idx[gl], 9:12], dg) > F(0))
                Fr, tir, nt, c = dielectric(dg, nsg, glass[idx[gl], 3], entering)
                r7, _ = _philox(seed, pix[a[gl]], smp[a[gl]], 32 + depth)
                with np.errstate(invalid="ignore"):
                    t = ~tir & (Fr.astype(np.float64) <= r7)                # a NaN Fr reflects
                nd[gl] = np.where(t[:, None], nt, spec_reflect(dg, nsg)[0])
                tr[gl] = t
                info["glass"] += gl.size
                if sm is not None:
                    below = _dot(nd[gl], nrm[gl]) < F(0)
                    ended[gl] = sm[gl] & (~(c < F(0)) | (~t & below) | (t & ~below))
        if df.size:
            r1, r2 = _philox(seed, pix[a[df]], smp[a[df]], depth)
            nd[df] = _unit_vec(ns[df], r1, r2)
            ct[df] = _dot(nd[df], ns[df])
            if sm is not None:
                ended[df] = sm[df] & (_dot(nd[df], nrm[df]) < F(0))
        hct[depth, a] = ct
        hidx[depth, a] = idx
        if sl is not None:
            hspec[depth, a] = sl
            htrans[depth, a] = tr
            prev_spec[a] = sl
        prev_gloss[:] = False
        prev_gloss[a[isgl & ~ended]] = True
        n_gloss[a[isgl]] += 1
        o[a], d[a], src[a] = x, nd, idx.astype(np.int32)
        alive[a[ended]] = False
    info["two_glossy"] = int((n_gloss >= 2).sum())
    # 6: the unwind, one step per hit, backward, from the miss term
    for depth in range(nhits - 1, -1, -1):
        h = np.flatnonzero(hidx[depth] >= 0)
        i = hidx[depth, h]
        brdf = mats[i, 0:3] * INV_PI
        if spec is None:
            rec[h] = E[depth, h] + ((brdf * rec[h]) * hct[depth, h][:, None]) * INV_P
        else:
            r = spec_unwind(spec[i], hspec[depth, h], E[depth, h], brdf, rec[h], hct[depth, h])
            if glass is not None:
                g = glass[i]
                with np.errstate(invalid="ignore", over="ignore"):
                    through = E[depth, h] + np.where(htrans[depth, h][:, None], g[:, 0:3] * rec[h], rec[h])
                r = np.where((g[:, 3] > F(0))[:, None], through, r).astype(F)
            if rough is not None:                                 # a specular hit whose slot holds g > 0
                gm = hspec[depth, h] & (hct[depth, h] > F(0))
                r = np.where(gm[:, None], gloss_unwind(spec[i], E[depth, h], rec[h], hct[depth, h]), r).astype(F)
            rec[h] = r
    return rec.reshape(npix, n, 3), scans, info


def render(rays, tris, mats, n, seed, est, spec=None, vn=None, glass=None, env=None, rough=None):
    """-> (rgba [npix, 4] u8, mean [npix, 3] f32, scans, info) of a one-shot render of n samples under `samples`' estimator"""
    rec, scans, info = samples(rays, tris, mats, seed, 0, n, est, spec, vn, glass, env, rough)
    acc = np.zeros((rec.shape[0], 3), F)
    for s in range(n):
        acc = acc + rec[:, s]
    mean = acc * F(1.0 / n)
    c = np.clip(mean, F(0), F(1)) * F(255) + F(0.5)
    q = np.where(c < 0, 0, np.where(c > 255, 255, c.astype(np.uint32) & 0xFF)).astype(np.uint8)
    rgba = np.zeros((rec.shape[0], 4), np.uint8)
    rgba[:, :3] = q
    return rgba, mean, scans, info


def covered(info, smooth=False):
    """a replay case proves something only where its rules fire"""
    for k in ("glossy", "ended", "two_glossy"):
        assert info[k] > 0, (k, info)
    assert info["ended"] < info["glossy"], info
    assert info["emit_after_glossy"] + info["miss_after_glossy"] > 0, info
    if smooth:
        assert info["ended_above"] > 0 and info["ended_below"] > 0, info
