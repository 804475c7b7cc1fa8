"""Transparency in the numpy model (include/spath_hip.h "transparency"): tests/path_model.py's loop restated with
the dielectric steps, on top of its step functions and the oracle.  A hit on a triangle whose row of the dielectric table has ior > 0
is a specular hit whose lobe is drawn against the Fresnel reflectance: it reflects by spec_reflect or transmits by Snell's law, and
the unwind adds E_d + rec_{d+1} or E_d + kt * rec_{d+1}.  Every other hit is path_model's.

glass = None means that the step is not executed and the loop is path_model.samples' (tests/test_hip_dielectric.py holds the two
together, bits and scans); with a table the specular step is executed as in the kernels, against spec or, without one, a table of
zeros.

Not a test module: tests/test_hip_dielectric.py holds the kernels to it."""
import numpy as np

from oracle import oracle as O
from path_model import (ESTIMATORS, F, INV_P, INV_PI, _bits, _dot, _philox, _unit_vec, light_table, mis_emit, nee_light,  # noqa: F401
                        shade_normal, smooth_light_ok, spec_lobe, spec_reflect, spec_unwind, turned_normal)
from spath_amd import scene


def dielectric(d, ns, ior, entering):
    """the header's statement for rays d on shading normals ns (turned against d) at interfaces of index ior, entering from the vacuum
    side or not -> (Fr, tir, nt, c); f32, every operation rounded on its own"""
    d, ns, ior = np.asarray(d, F), np.asarray(ns, F), np.asarray(ior, F)
    with np.errstate(all="ignore"):
        eta = np.where(entering, F(1) / ior, ior).astype(F)
        c = _dot(d, ns)
        ci = -c
        k = F(1) - (eta * eta) * (F(1) - ci * ci)
        tir = ~(k > F(0))
        ct = np.sqrt(k)
        a, b = eta * ci, eta * ct
        rs, rp = (a - ct) / (a + ct), (ci - b) / (ci + b)
        Fr = F(0.5) * (rs * rs + rp * rp)
        nt = d * eta[:, None] + ns * (a - ct)[:, None]
    return Fr.astype(F), tir, nt.astype(F), c.astype(F)


def dielectric64(d, ns, ior, entering):
    """Snell and Fresnel in float64 on the same f32 inputs, from the textbook forms (sines and cosines of the two angles) -> (Fr, tir, nt)"""
    d, ns, ior = np.asarray(d, F).astype(np.float64), np.asarray(ns, F).astype(np.float64), np.asarray(ior, F).astype(np.float64)
    with np.errstate(all="ignore"):
        eta = np.where(entering, 1.0 / ior, ior)                  # n_incident / n_transmitted
        ci = -(d * ns).sum(1)
        s2t = eta * eta * (1.0 - ci * ci)                          # sin^2 of the refracted angle
        tir = ~(s2t < 1.0)
        ct = np.sqrt(1.0 - s2t)
        rs = (eta * ci - ct) / (eta * ci + ct)
        rp = (ci - eta * ct) / (ci + eta * ct)
        Fr = 0.5 * (rs * rs + rp * rp)
        nt = eta[:, None] * d + (eta * ci - ct)[:, None] * ns
    return Fr, tir, nt


def samples(rays, tris, mats, seed, s0, n, est, spec=None, vn=None, glass=None, collect=()):
    """path_model.samples with a dielectric table glass [N, 4] (kt.r kt.g kt.b ior; None: the flag is not set) -> (rec, scans, info).
    info adds: "glass" hits on an interface, of those "transmit" transmissions and "tir" total internal reflections;
    "emitter_after_glass" hits on an emitter straight after an interface; "two_transmissions" samples with two or more; paths
    "ended_glass_c" (dir not against ns), "ended_glass_reflect" and "ended_glass_transmit" by the rules of smooth shading"""
    if est not in ESTIMATORS:
        raise ValueError(f"unknown estimator {est!r}")
    if est == "nee" and (spec is not None or vn is not None or glass is not None):
        raise ValueError("plain NEE takes no specular table, no vertex normals and no dielectric table (the library refuses the flags together)")
    tris = np.ascontiguousarray(tris, F).reshape(-1, 12)
    mats = np.ascontiguousarray(mats, F).reshape(-1, 6)
    rays = np.ascontiguousarray(rays, F).reshape(-1, 6)
    spec = None if spec is None else np.ascontiguousarray(spec, F).reshape(-1, 4)
    vn = None if vn is None else np.ascontiguousarray(vn, F).reshape(-1, 9)
    glass = None if glass is None else np.ascontiguousarray(glass, F).reshape(-1, 4)
    if glass is not None and spec is None:
        spec = np.zeros((tris.shape[0], 4), F)                    # the context's table of zeros: p = 0, wD = 1.0f
    mis = est == "mis"
    light = None if est == "plain" else (scene.light_table if mis else light_table)(tris, mats)
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
    htrans = np.zeros((nhits, P), bool)
    E = np.zeros((nhits, P, 3), F)
    prev_spec = np.zeros(P, bool)
    prev_glass = np.zeros(P, bool)
    n_trans = np.zeros(P, np.int64)
    spec_then_hit = np.zeros(P, bool)
    emit_after_spec = np.zeros(P, bool)
    info = {"samples": P, "hits": 0, "sm": 0, "ended_diffuse": 0, "ended_mirror": 0, "lights": 0, "lights_cut": 0, "glass": 0, "transmit": 0,
            "tir": 0, "emitter_after_glass": 0, "ended_glass_c": 0, "ended_glass_reflect": 0, "ended_glass_transmit": 0}
    if "accepts" in collect:
        info["accepts"] = []
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
        emits = mats[idx, 3:6].astype(np.float64).sum(1) > 0
        spec_then_hit[a[ps]] = True
        emit_after_spec[a[ps & emits]] = True
        info["emitter_after_glass"] += int((prev_glass[a] & emits).sum())
        # 1, 2: the turned normal and the shading normal
        nrm = turned_normal(tris, idx, d[a])
        x = o[a] + d[a] * dist[:, None]
        ns, sm = nrm, None
        if vn is not None:
            _, _, ns, sm = shade_normal(o[a], d[a], tris[idx, 0:9], vn[idx], nrm)
            info["sm"] += int(sm.sum())
        # 3: the lobe; an interface is a specular hit (its own draw, from the same stream, comes with the bounce)
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
                    vis = ~((sidx >= 0) & (sd < tmax[k]))                   # glass occludes like everything else
                    if "accepts" in collect:
                        info["accepts"].append((x[k][sidx >= 0], wd[k][sidx >= 0], sidx[sidx >= 0].astype(np.int64)))
                    L[k[vis]] = Lc[k[vis]]
            De = De + L
        E[depth, a] = De
        # 5: the bounce
        nd = np.zeros((a.size, 3), F)
        ct = np.zeros(a.size, F)
        ended = np.zeros(a.size, bool)
        tr = np.zeros(a.size, bool)
        df = np.arange(a.size)
        if sl is not None:
            gl, mr, df = np.flatnonzero(isg), np.flatnonzero(sl & ~isg), np.flatnonzero(~sl)
            nd[mr], c = spec_reflect(d[a[mr]], ns[mr])
            if sm is not None:
                ended[mr] = sm[mr] & (~(c < F(0)) | (_dot(nd[mr], nrm[mr]) < F(0)))
                info["ended_mirror"] += int(ended[mr].sum())
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
                info["transmit"] += int(t.sum())
                info["tir"] += int(tir.sum())
                if sm is not None:
                    below = _dot(nd[gl], nrm[gl]) < F(0)
                    e_c, e_r, e_t = sm[gl] & ~(c < F(0)), sm[gl] & ~t & below, sm[gl] & t & ~below
                    ended[gl] = e_c | e_r | e_t
                    info["ended_glass_c"] += int(e_c.sum())
                    info["ended_glass_reflect"] += int((e_r & ~e_c).sum())
                    info["ended_glass_transmit"] += int((e_t & ~e_c).sum())
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
            htrans[depth, a] = tr
            prev_spec[a] = sl
            prev_glass[a] = isg
            n_trans[a] += tr
        o[a], d[a], src[a] = x, nd, idx.astype(np.int32)
        alive[a[ended]] = False
    # 6: the unwind, one step per hit, backward
    rec = np.zeros((P, 3), F)
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
            rec[h] = r
    info["spec_then_hit"], info["emitter_after_spec"] = int(spec_then_hit.sum()), int(emit_after_spec.sum())
    info["two_transmissions"] = int((n_trans >= 2).sum())
    return rec.reshape(npix, n, 3), scans, info


def render(rays, tris, mats, n, seed, est, spec=None, vn=None, glass=None, collect=()):
    """-> (rgba [npix, 4] u8, mean [npix, 3] f32, scans, info) of a one-shot render of n samples under `samples`' estimator"""
    rec, scans, info = samples(rays, tris, mats, seed, 0, n, est, spec, vn, glass, collect)
    acc = np.zeros((rec.shape[0], 3), F)
    for s in range(n):
        acc = acc + rec[:, s]
    mean = acc * F(1.0 / n)
    c = np.clip(mean, F(0), F(1)) * F(255) + F(0.5)
    q = np.where(c < 0, 0, np.where(c > 255, 255, c.astype(np.uint32) & 0xFF)).astype(np.uint8)
    rgba = np.zeros((rec.shape[0], 4), np.uint8)
    rgba[:, :3] = q
    return rgba, mean, scans, info
