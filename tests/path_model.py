"""The device estimator, replayed in numpy: the one statement of what a path computes that the integrator kernels are held to, bit
for bit (include/spath_hip.h states the arithmetic operation by operation; DESIGN.md sections 5.4 to 5.13).  `samples` is the only
function under tests/ that walks a path.

A hit goes through the six steps of DESIGN.md section 5.9, each a function named after its counterpart in
spath_amd/csrc/sp_integrator.h: the turned normal, shade_normal, spec_lobe, the direct term (mis_emit, nee_light, smooth_light_ok;
env_light for the map's entry of the light table), the bounce (spec_reflect, dielectric at an interface, gloss_bounce on a rough
mirror, or the diffuse direction) and, backward, spec_unwind and gloss_unwind; a ray that leaves the scene takes env_miss.  The steps
of transparency, environment lighting and glossy reflection are in tests/dielectric_model.py, env_model.py and glossy_model.py, the
rest here.  Closest hits of path and shadow rays go through the oracle's strict scan (O.closest_hits; a shadow ray is occluded iff the
closest hit that skips its source triangle lies below tmax), draws and diffuse directions through the oracle's device math, every
other step in f32 in the stated order.

A table that is not given (spec, vn, glass, env, rough) means that its step is not executed, as in a kernel instantiated without
the argument; a table of zeros executes the step.  The tests compare the two.

Not a test module: tests/test_hip_nee.py, test_hip_mis.py, test_hip_specular.py, test_hip_smooth.py, test_hip_dielectric.py,
test_hip_environment.py and test_hip_glossy.py hold the kernels to it, tests/test_path_model.py pins its output on the CPU."""
import numpy as np

from dielectric_model import dielectric
from env_model import env_light, env_miss, flagged_light_table, lookup, scene_part, tables
from glossy_model import GLOSS_STREAM, gloss_bounce, gloss_unwind
from model_primitives import (INV_P, INV_PI, MARGIN, PI_SQ, TWO_OVER_PI, TWO_PI, F, _bits, _cross, _dot, _philox, _u,  # noqa: F401
                              _unit_vec)                          # re-exported: the tests import them from here
from oracle import oracle as O
from spath_amd import scene

ESTIMATORS = ("plain", "nee", "mis")


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
def samples(rays, tris, mats, seed, s0, n, est, spec=None, vn=None, glass=None, env=None, rough=None, first_ns=None, collect=()):
    """-> (rec, scans, info): the radiance [npix, n, 3] of global samples s0 .. s0 + n - 1 under the estimator est ("plain", "nee":
    light samples at the first four hits, emission at the camera's hit only, "mis": NEE|MIS), the scans (path + shadow) they take, and
    what the samples met.  spec [N, 4], vn [N, 9], glass [N, 4] (kt.r kt.g kt.b ior), env [n, n, 3], rough [N]: the specular table, the
    vertex normals, the dielectric table, the environment map and the roughness table; None: the flag is not set.
    info, every counter 0 where its step is not executed: "samples"; "hits" and, of those, "sm" with a shading normal;
    "spec_then_hit" samples with a specular bounce whose ray hit something, "emitter_after_spec" samples that reached an emitter
    directly after one; paths "ended_diffuse" and "ended_mirror" by the rules of smooth shading; "lights" drawn and, of those,
    "lights_cut" by the geometric guard, the rest shadow rays: "tri_lights" towards triangles and "env_lights" towards the map, of those
    "env_unoccluded" and "env_occluded".
    Mirror lobe: "spec" hits that took it (no interface), of those "alpha0" on a row alpha = 0 under a roughness table and "glossy"
    that took the glossy step; "ended" glossy hits ended by !ok, "ended_above" / "ended_below" smooth ones ended by the rule !(c < 0) /
    dot3(nd, n) < 0; "two_glossy" samples with two glossy hits or more, "emit_after_glossy" hits on an emitter and "miss_after_glossy"
    misses straight after a glossy hit.
    Interfaces: "glass" hits on one, of those "transmit" transmissions and "tir" total internal reflections; "emitter_after_glass" hits
    on an emitter straight after one; "two_transmissions" samples with two or more; paths "ended_glass_c" (dir not against ns),
    "ended_glass_reflect" and "ended_glass_transmit" by the rules of smooth shading.
    Under a map: "miss" [5] rays of depth d that left the scene and, of those, "miss_after_spec" straight after a specular or
    transmitted hit and "miss_weighted" those that MIS weighted.
    collect: "accepts" adds the list of (o, d, triangle) of every hit the float test accepted, path and shadow rays alike, "inexact"
    the set of triangles with a smooth hit whose ns is not n bitwise.
    first_ns: a list that receives (pixel, ns) of every sample's first hit (the G-buffer's normal)"""
    if est not in ESTIMATORS:
        raise ValueError(f"unknown estimator {est!r}")
    if est == "nee" and any(x is not None for x in (spec, vn, glass, env, rough)):
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
    # the stand-ins: a kernel with a later flag executes the earlier steps against the context's tables of zeros; with neither table
    # the unwind keeps its plain expression
    if (env is not None or rough is not None) and glass is None:
        glass = np.zeros((tris.shape[0], 4), F)                   # ior = 0, no interface
    if glass is not None and spec is None:
        spec = np.zeros((tris.shape[0], 4), F)                    # p = 0, wD = 1.0f
    mis = est == "mis"
    tab = tpdf = None
    if est == "plain":
        light = None
    elif env is not None:
        tab = tables(env)
        part = scene_part(tab, tris, mats)
        tpdf = part["tpdf"]
        light = flagged_light_table(tris, mats, part)             # a black map adds no entry: scene.light_table itself
    else:
        light = (scene.light_table if mis else light_table)(tris, mats)      # NEE keeps the float64 table above
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
    prev_glass = np.zeros(P, bool)
    prev_gloss = np.zeros(P, bool)
    n_trans = np.zeros(P, np.int64)
    n_gloss = np.zeros(P, np.int64)
    spec_then_hit = np.zeros(P, bool)
    emit_after_spec = np.zeros(P, bool)
    info = dict.fromkeys(("hits", "sm", "ended_diffuse", "ended_mirror", "lights", "lights_cut", "tri_lights", "env_lights", "env_unoccluded",
                          "env_occluded", "spec", "alpha0", "glossy", "ended", "ended_above", "ended_below", "emit_after_glossy",
                          "miss_after_glossy", "glass", "transmit", "tir", "emitter_after_glass", "ended_glass_c", "ended_glass_reflect",
                          "ended_glass_transmit", "miss_after_spec", "miss_weighted"), 0)
    info.update(samples=P, miss=[0] * 5)
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
        # the miss term
        m = a[~hit]
        info["miss_after_glossy"] += int(prev_gloss[m].sum())
        if env is not None:
            full = prev_spec[m] if depth > 0 else np.ones(m.size, bool)
            rec[m] = env_miss(env, tpdf, d[m], full, mis)
            info["miss"][depth] += m.size
            info["miss_after_spec"] += int(prev_spec[m].sum())
            if mis:
                li_, lj_, _, ok_ = lookup(d[m], env.shape[0])
                info["miss_weighted"] += int((ok_ & ~full & (tpdf[lj_, li_] > F(0))).sum())
        a, idx, dist = a[hit], idx[hit].astype(np.int64), dist[hit]
        info["hits"] += a.size
        if "accepts" in collect:
            info["accepts"].append((o[a].copy(), d[a].copy(), idx.copy()))
        ps = prev_spec[a]
        emits = mats[idx, 3:6].astype(np.float64).sum(1) > 0
        spec_then_hit[a[ps]] = True
        emit_after_spec[a[ps & emits]] = True
        info["emitter_after_glass"] += int((prev_glass[a] & emits).sum())
        info["emit_after_glossy"] += int((prev_gloss[a] & emits).sum())
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
        # 3: the lobe; an interface is a specular hit (its own draw, from the same stream, comes with the bounce)
        isg = np.zeros(a.size, bool) if glass is None else glass[idx, 3] > F(0)
        sl = None if spec is None else spec_lobe(seed, pix[a], smp[a], depth, spec[idx, 3])
        if glass is not None:
            sl = sl | isg
        # 4: the direct term.  MIS: the emission in full at the camera's hit and after a specular bounce, else weighted; plain NEE: the
        # camera's hit alone emits
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
                        cut = ok & ~smooth_light_ok(sm, wd, nrm)
                    ok &= ~cut
                    info["lights_cut"] += int(cut.sum())
                    info["lights"] += int(cut.sum())
                k = np.flatnonzero(ok)
                info["lights"] += k.size
                info["env_lights"] += int(is_env[k].sum())
                info["tri_lights"] += int((~is_env[k]).sum())
                scans += k.size
                if k.size:
                    sidx, sd = O.closest_hits(np.concatenate([x[k], wd[k]], 1), tris, idx[k].astype(np.int32))
                    vis = ~((sidx >= 0) & (sd < tmax[k]))                   # glass occludes like everything else
                    if "accepts" in collect:
                        info["accepts"].append((x[k][sidx >= 0], wd[k][sidx >= 0], sidx[sidx >= 0].astype(np.int64)))
                    info["env_unoccluded"] += int((vis & is_env[k]).sum())
                    info["env_occluded"] += int((~vis & is_env[k]).sum())
                    L[k[vis]] = Lc[k[vis]]
            De = De + L
        E[depth, a] = De
        # 5: the bounce; under smooth shading one that leaves the side of the stored normal it belongs on ends the path
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
            info["ended_mirror"] += int((ended[mr] & ~isgl[mr]).sum())
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
        prev_gloss[:] = False
        prev_gloss[a[isgl & ~ended]] = True
        n_gloss[a[isgl]] += 1
        o[a], d[a], src[a] = x, nd, idx.astype(np.int32)
        alive[a[ended]] = False                                             # the hit keeps E_d; rec_{d+1} = 0; nothing more is scanned
    # 6: the unwind, one step per hit, backward, from the miss term
    for depth in range(nhits - 1, -1, -1):
        h = np.flatnonzero(hidx[depth] >= 0)
        i = hidx[depth, h]
        brdf = mats[i, 0:3] * INV_PI
        if spec is None:
            rec[h] = E[depth, h] + ((brdf * rec[h]) * hct[depth, h][:, None]) * INV_P
            continue
        r = spec_unwind(spec[i], hspec[depth, h], E[depth, h], brdf, rec[h], hct[depth, h])
        if glass is not None:
            g = glass[i]
            with np.errstate(invalid="ignore", over="ignore"):
                through = E[depth, h] + np.where(htrans[depth, h][:, None], g[:, 0:3] * rec[h], rec[h])
            r = np.where((g[:, 3] > F(0))[:, None], through, r).astype(F)
        if rough is not None:                                     # a specular hit whose slot holds g > 0
            gm = hspec[depth, h] & (hct[depth, h] > F(0))
            r = np.where(gm[:, None], gloss_unwind(spec[i], E[depth, h], rec[h], hct[depth, h]), r).astype(F)
        rec[h] = r
    info["spec_then_hit"], info["emitter_after_spec"] = int(spec_then_hit.sum()), int(emit_after_spec.sum())
    info["two_transmissions"], info["two_glossy"] = int((n_trans >= 2).sum()), int((n_gloss >= 2).sum())
    return rec.reshape(npix, n, 3), scans, info


def render(rays, tris, mats, n, seed, est, spec=None, vn=None, glass=None, env=None, rough=None, first_ns=None, collect=()):
    """-> (rgba [npix, 4] u8, mean [npix, 3] f32, scans, info) of a one-shot render of n samples under `samples`' estimator"""
    rec, scans, info = samples(rays, tris, mats, seed, 0, n, est, spec, vn, glass, env, rough, first_ns, collect)
    acc = np.zeros((rec.shape[0], 3), F)
    for s in range(n):
        acc = acc + rec[:, s]
    mean = acc * F(1.0 / n)
    c = np.clip(mean, F(0), F(1)) * F(255) + F(0.5)
    q = np.where(c < 0, 0, np.where(c > 255, 255, c.astype(np.uint32) & 0xFF)).astype(np.uint8)
    rgba = np.zeros((rec.shape[0], 4), np.uint8)
    rgba[:, :3] = q
    return rgba, mean, scans, info
