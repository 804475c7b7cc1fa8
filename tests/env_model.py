"""Environment lighting in the numpy model (include/spath_hip.h, "environment lighting"), operation by operation:
the octahedral lookup and the sample in f32, the importance tables in float64 with numpy's sequential cumsum, and tests/path_model.py's
loop restated (on top of tests/dielectric_model.py's restatement) with the environment steps: the map's entry of the flagged light
table, its light sample, and the miss term from which the unwind of a path that left the scene starts.

env = None means that the steps are not executed and the loop is dielectric_model.samples', which without a dielectric table is
path_model.samples' (tests/test_env_model.py holds them together, bits and scans); with a map the specular and the dielectric step
are executed as in the kernels, against the tables given or tables of zeros.

Not a test module: tests/test_hip_environment.py holds the device functions, the table kernels and the path kernels to it at
tolerance 0."""
import numpy as np

from oracle import oracle as O
from dielectric_model import dielectric
from path_model import (ESTIMATORS, F, INV_P, INV_PI, PI_SQ, TWO_PI, _dot, _philox, _unit_vec, mis_emit, nee_light, shade_normal,
                        smooth_light_ok, spec_lobe, spec_reflect, spec_unwind, turned_normal)
from spath_amd import scene

MAX_DIST = F(1e12)

ONE, HALF, TWO = F(1), F(0.5), F(2)


def _sgn(t):
    return np.where(t < 0, t.dtype.type(-1), t.dtype.type(1))


def _dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cell(a, n):
    """clamp((int)((a * 0.5f + 0.5f) * (float)n), 0, n - 1): the C conversion truncates towards zero"""
    v = (a * HALF + HALF) * F(n)
    return np.clip(np.trunc(v), 0, n - 1).astype(np.int64)


def lookup(d, n):
    """env_lookup for directions d [m, 3] -> (i, j, r3, valid)"""
    d = np.ascontiguousarray(d, F).reshape(-1, 3)
    ad = np.abs(d)
    s = (ad[:, 0] + ad[:, 1]) + ad[:, 2]
    valid = (s > 0) & np.isfinite(s)
    with np.errstate(all="ignore"):
        p = d / np.where(valid, s, ONE)[:, None]
        low = ~(p[:, 1] >= 0)
        a = np.where(low, (ONE - np.abs(p[:, 2])) * _sgn(p[:, 0]), p[:, 0])
        b = np.where(low, (ONE - np.abs(p[:, 0])) * _sgn(p[:, 2]), p[:, 2])
        l2 = _dot3(p, p)
        r3 = np.sqrt(l2) * l2
        i, j = _cell(np.where(valid, a, F(-1)), n), _cell(np.where(valid, b, F(-1)), n)
    assert r3.dtype == F
    return np.where(valid, i, 0), np.where(valid, j, 0), np.where(valid, r3, F(0)), valid


def place(i, j, r3u, r4u, n):
    """the direction of place (r3u, r4u) in texel (i, j) -> (wd [m, 3], r3): env_sample after the texel is chosen"""
    step = TWO / F(n)
    a = (np.asarray(i).astype(F) + np.asarray(r3u, np.float64).astype(F)) * step - ONE
    b = (np.asarray(j).astype(F) + np.asarray(r4u, np.float64).astype(F)) * step - ONE
    y = (ONE - np.abs(a)) - np.abs(b)
    up = y >= 0
    x = np.where(up, a, (ONE - np.abs(b)) * _sgn(a))
    z = np.where(up, b, (ONE - np.abs(a)) * _sgn(b))
    g = np.stack([x, y, z], axis=-1)
    l2 = _dot3(g, g)
    ln = np.sqrt(l2)
    wd = g / ln[:, None]
    assert wd.dtype == F
    return wd, ln * l2


def tables(texels):
    """the map's own tables -> dict(n, wt [n, n], rc [n, n], marg [n], T, Phi), float64, the 2-d arrays indexed [j, i]"""
    tx = np.ascontiguousarray(texels, F)
    n = tx.shape[0]
    assert tx.shape == (n, n, 3)
    c = -1.0 + (2.0 * np.arange(n) + 1.0) / float(n)
    a, b = np.meshgrid(c, c, indexing="xy")
    y = (1.0 - np.abs(a)) - np.abs(b)
    up = y >= 0
    x = np.where(up, a, (1.0 - np.abs(b)) * _sgn(a))
    z = np.where(up, b, (1.0 - np.abs(a)) * _sgn(b))
    l2 = (x * x + y * y) + z * z
    t64 = tx.astype(np.float64)
    wt = ((t64[..., 0] + t64[..., 1]) + t64[..., 2]) / (np.sqrt(l2) * l2)
    rc = np.cumsum(wt, axis=1)
    marg = np.cumsum(rc[:, n - 1])
    T = float(marg[n - 1])
    return {"n": n, "wt": wt, "rc": rc, "marg": marg, "T": T, "Phi": T * (4.0 / (float(n) * n))}


def scene_part(tab, tris, mats):
    """what follows the scene: w_env, W and tpdf [n, n] f32 for the tables of `tables` under the scene's light table"""
    t = np.asarray(tris, F).reshape(-1, 12)
    v = t[:, :9].reshape(-1, 3)
    ext = v.max(0).astype(np.float64) - v.min(0).astype(np.float64)
    R2 = 0.25 * ((ext[0] * ext[0] + ext[1] * ext[1]) + ext[2] * ext[2])
    W_tri = scene.light_table(t, mats)[3]
    n, T = tab["n"], tab["T"]
    w_env = (0.5 * R2) * tab["Phi"] if T > 0.0 else 0.0
    if not w_env > 0.0:                                           # a black map, or a scene whose bounding box is a point: no entry
        return {"w_env": 0.0, "W": float(W_tri), "tpdf": np.zeros((n, n), F)}
    W = W_tri + w_env
    tpdf = (((w_env / W) * (tab["wt"] / T)) * (float(n) * n / 4.0)).astype(F)
    return {"w_env": float(w_env), "W": float(W), "tpdf": tpdf}


def _first_above(t, x):
    """the first k with t[k] > x, the last index when there is none (t ascending)"""
    return np.minimum(np.searchsorted(t, x, side="right"), len(t) - 1)


def sample(tab, r8, r9, r3u, r4u):
    """env_sample for uniforms [m] each (float64) -> (i, j, wd [m, 3], r3)"""
    n = tab["n"]
    r8, r9 = np.asarray(r8, np.float64), np.asarray(r9, np.float64)
    j = _first_above(tab["marg"], r8 * tab["T"])
    i = np.zeros_like(j)
    for row in np.unique(j):
        k = j == row
        i[k] = _first_above(tab["rc"][row], r9[k] * tab["rc"][row, n - 1])
    wd, r3 = place(i, j, r3u, r4u, n)
    return i, j, wd, r3


def roundtrip_share(n, count, seed):
    """the share of `count` uniform (texel, r3, r4) draws whose direction env_lookup assigns to another texel: draws that land on a
    texel's edge (or, on the folded half, across it) after the f32 roundings of the two mappings"""
    rng = np.random.default_rng(seed)
    i, j = rng.integers(0, n, count), rng.integers(0, n, count)
    wd, _ = place(i, j, rng.random(count), rng.random(count), n)
    li, lj, _, ok = lookup(wd, n)
    return float(np.mean(~ok | (li != i) | (lj != j)))


# ---------------------------------------------------------------------------------------------------------------- the estimator
def u_env(sxz, r3, tp):
    """the balance ratio ((kPiSq * sxz) * r3) * tpdf[t], 0 where that is NaN"""
    with np.errstate(invalid="ignore", over="ignore"):
        u = ((PI_SQ * sxz) * r3) * tp
    return np.where(np.isnan(u), F(0), u).astype(F)


def flagged_light_table(tris, mats, part):
    """the light table of a flagged render -> (tri, cdf, ipdf, W, tipdf): scene.light_table's entries under the total W that includes
    w_env, then the map's entry (triangle -1, ipdf 0); without an entry (a black map) scene.light_table itself"""
    tri, cdf, ipdf, W, tipdf = scene.light_table(tris, mats)
    if not part["w_env"] > 0.0:
        return tri, cdf, ipdf, W, tipdf
    m = np.asarray(mats, F).reshape(-1, 6)
    e = m[tri, 3:6].astype(np.float64)
    es = (e[:, 0] + e[:, 1]) + e[:, 2]
    Wf = part["W"]
    ip = (Wf / es).astype(F)
    tip = np.zeros_like(tipdf)
    tip[tri] = ip
    return (np.concatenate([tri, np.array([-1], np.int64)]), np.concatenate([cdf, np.array([Wf], np.float64)]),
            np.concatenate([ip, np.zeros(1, F)]), Wf, tip)


def env_light(env, tab, tpdf, mats, seed, pix, smp, depth, n, idx):
    """the light sample that picked the map's entry, at hits on triangles idx with shading normals n -> (ok, wd, tmax, L, i, j)"""
    r8, r9 = _philox(seed, pix, smp, 40 + depth)
    r3u, r4u = _philox(seed, pix, smp, 8 + depth)
    i, j, wd, r3 = sample(tab, r8, r9, r3u, r4u)
    cx = _dot(wd, n)
    ok = cx > F(0)
    sxz = np.sqrt(wd[:, 0] * wd[:, 0] + wd[:, 2] * wd[:, 2])
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        g = (TWO_PI * cx) / (F(1) + u_env(sxz, r3, tpdf[j, i]))
        L = (mats[idx, 0:3] * INV_PI) * (env[j, i] * g[:, None])
    return ok, wd, np.full(idx.size, MAX_DIST, F), L.astype(F), i, j


def env_miss(env, tpdf, d, full, mis):
    """what rays of direction d that left the scene carry; full: the camera's ray or the ray after a specular or transmitted bounce"""
    n = env.shape[0]
    i, j, r3, valid = lookup(d, n)
    Le = np.where(valid[:, None], env[j, i], F(0)).astype(F)
    if not mis:
        return Le
    tp = tpdf[j, i]
    w = valid & ~full & (tp > F(0))
    opu = F(1) + u_env(np.sqrt(d[:, 0] * d[:, 0] + d[:, 2] * d[:, 2]), r3, tp)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(w[:, None], Le / opu[:, None], Le).astype(F)


def samples(rays, tris, mats, seed, s0, n, est, spec=None, vn=None, glass=None, env=None):
    """dielectric_model.samples with an environment map env [n, n, 3] (None: the flag is not set) -> (rec, scans, info).
    info: "miss" [5] rays of depth d that left the scene and, of those, "miss_after_spec" straight after a specular or transmitted
    hit and "miss_weighted" those that MIS weighted; "env_lights" light samples that picked the map and had cos_x > 0, of those
    "env_unoccluded" and "env_occluded"; "tri_lights" shadow rays towards triangles; "glass" hits on an interface, "spec" hits that
    took the mirror lobe"""
    if est not in ESTIMATORS:
        raise ValueError(f"unknown estimator {est!r}")
    if est == "nee" and (spec is not None or vn is not None or glass is not None or env is not None):
        raise ValueError("plain NEE takes no table and no environment map (the library refuses the flags together)")
    tris = np.ascontiguousarray(tris, F).reshape(-1, 12)
    mats = np.ascontiguousarray(mats, F).reshape(-1, 6)
    rays = np.ascontiguousarray(rays, F).reshape(-1, 6)
    spec = None if spec is None else np.ascontiguousarray(spec, F).reshape(-1, 4)
    vn = None if vn is None else np.ascontiguousarray(vn, F).reshape(-1, 9)
    glass = None if glass is None else np.ascontiguousarray(glass, F).reshape(-1, 4)
    env = None if env is None else np.ascontiguousarray(env, F)
    if env is not None and glass is None:
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
    hct = np.zeros((nhits, P), F)
    hspec = np.zeros((nhits, P), bool)
    htrans = np.zeros((nhits, P), bool)
    E = np.zeros((nhits, P, 3), F)
    rec = np.zeros((P, 3), F)                                     # the unwind starts from the miss term, 0 for a path that did not leave
    prev_spec = np.zeros(P, bool)
    info = {"samples": P, "hits": 0, "miss": [0] * 5, "miss_after_spec": 0, "miss_weighted": 0, "env_lights": 0, "env_unoccluded": 0,
            "env_occluded": 0, "tri_lights": 0, "glass": 0, "spec": 0}
    scans = 0
    for depth in range(nhits):
        a = np.flatnonzero(alive)
        if a.size == 0:
            break
        scans += a.size
        idx, dist = O.closest_hits(np.concatenate([o[a], d[a]], 1), tris, src[a])
        hit = idx >= 0
        alive[a[~hit]] = False
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
        df = np.arange(a.size)
        if sl is not None:
            gl, mr, df = np.flatnonzero(isg), np.flatnonzero(sl & ~isg), np.flatnonzero(~sl)
            info["spec"] += mr.size
            nd[mr], c = spec_reflect(d[a[mr]], ns[mr])
            if sm is not None:
                ended[mr] = sm[mr] & (~(c < F(0)) | (_dot(nd[mr], nrm[mr]) < F(0)))
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
        o[a], d[a], src[a] = x, nd, idx.astype(np.int32)
        alive[a[ended]] = False
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
            rec[h] = r
    return rec.reshape(npix, n, 3), scans, info


def render(rays, tris, mats, n, seed, est, spec=None, vn=None, glass=None, env=None):
    """-> (rgba [npix, 4] u8, mean [npix, 3] f32, scans, info) of a one-shot render of n samples under `samples`' estimator"""
    rec, scans, info = samples(rays, tris, mats, seed, 0, n, est, spec, vn, glass, env)
    acc = np.zeros((rec.shape[0], 3), F)
    for s in range(n):
        acc = acc + rec[:, s]
    mean = acc * F(1.0 / n)
    c = np.clip(mean, F(0), F(1)) * F(255) + F(0.5)
    q = np.where(c < 0, 0, np.where(c > 255, 255, c.astype(np.uint32) & 0xFF)).astype(np.uint8)
    rgba = np.zeros((rec.shape[0], 4), np.uint8)
    rgba[:, :3] = q
    return rgba, mean, scans, info


# ---------------------------------------------------------------------------------------------------------------- scenes of the tests
def glass_scene():
    """default_scene without its back wall plus icosphere(1) of glass where hip_checks puts its sphere: paths leave through glass and
    past it -> (tris, mats, glass)"""
    t0, m0 = scene.default_scene()
    ts, ms = scene.icosphere(1, (0.0, -0.35, -0.9), 0.5, (0.8, 0.7, 0.6, 0, 0, 0))
    t, m = np.concatenate([t0[:5], ts]), np.concatenate([m0[:5], ms])
    return t, m, scene.dielectric_table(t, 1.5, (0.9, 0.95, 1.0), which=np.arange(5, t.shape[0]))


def _quads(quads):
    v = []
    for a, b, c, d in quads:
        v += [list(a) + list(b) + list(c), list(a) + list(c) + list(d)]
    t = np.zeros((len(v), 12), F)
    t[:, :9] = np.asarray(v, F)
    return scene.flat_normals(t)


def _box(lo, hi):
    (x0, y0, z0), (x1, y1, z1) = lo, hi
    return [((x0, y0, z0), (x1, y0, z0), (x1, y0, z1), (x0, y0, z1)), ((x0, y1, z0), (x1, y1, z0), (x1, y1, z1), (x0, y1, z1)),
            ((x0, y0, z0), (x1, y0, z0), (x1, y1, z0), (x0, y1, z0)), ((x0, y0, z1), (x1, y0, z1), (x1, y1, z1), (x0, y1, z1)),
            ((x0, y0, z0), (x0, y0, z1), (x0, y1, z1), (x0, y1, z0)), ((x1, y0, z0), (x1, y0, z1), (x1, y1, z1), (x1, y1, z0))]


def window_room():
    """a room x in [-3, 3], y in [-1, 2], z in [-4, 2] around the camera, with a window in the wall z = 2 (x in [-1.5, 1.5], y in
    [0, 1.5]: the wall is four quads around it) and one emissive triangle under the ceiling: both kinds of entry of the flagged light
    table are drawn -> (tris, mats)"""
    q = _box((-3, -1, -4), (3, 2, 2))
    del q[3]                                                      # the wall z = 2, rebuilt around the window
    z = 2
    q += [((-3, -1, z), (3, -1, z), (3, 0, z), (-3, 0, z)), ((-3, 1.5, z), (3, 1.5, z), (3, 2, z), (-3, 2, z)),
          ((-3, 0, z), (-1.5, 0, z), (-1.5, 1.5, z), (-3, 1.5, z)), ((1.5, 0, z), (3, 0, z), (3, 1.5, z), (1.5, 1.5, z))]
    t = _quads(q)
    e = np.zeros((1, 12), F)
    e[0, :9] = [-1, 1.9, -2, 1, 1.9, -2, 0, 1.9, 0]
    t = np.concatenate([t, scene.flat_normals(e)])
    m = np.zeros((t.shape[0], 6), F)
    m[:, 0:3] = (0.7, 0.65, 0.6)
    m[-1] = (0.2, 0.2, 0.2, 6.0, 5.0, 4.0)
    return t, m


def replay_maps():
    """the maps of the replay: a sky at n = 64 whose entry dominates the light table, and a dim one at n = 3 (a non-power of two, texels
    that span the fold) that leaves the triangles a share of the draws"""
    return {"sky64": scene.sky_environment(64),
            "n3": scene.sky_environment(3, sun_radiance=(0.3, 0.25, 0.2), sun_halfangle=0.9, sky_radiance=(0.02, 0.03, 0.05), ground_radiance=(0.01, 0.01, 0.01))}


def replay_scene(name, tables, mixed_table):
    """-> (tris, mats, spec, vn, glass): "open": open_clutter(100), "glass": glass_scene; bare, or with mixed_table (hip_checks') over the
    triangles and smooth normals over the clutter or the sphere"""
    if name == "open":
        t, m = scene.open_clutter(100)
        g, first = None, 7
    else:
        t, m, g = glass_scene()
        first = 5
    if not tables:
        return t, m, None, None, g
    s = np.zeros((t.shape[0], 4), F)
    if g is not None:
        s[first:, 3] = 1                                          # ignored on an interface; mixed_table leaves these rows alone
    return t, m, mixed_table(t, m, s), scene.vertex_normals(t, which=np.arange(first, t.shape[0])), g


def covered(info, name, tables, est):
    """a replay case proves something only where its rules fire"""
    assert all(k > 0 for k in info["miss"]), info
    if est == "mis":
        for k in ("env_lights", "env_unoccluded", "env_occluded", "tri_lights", "miss_weighted"):
            assert info[k] > 0, (k, info)
    if name == "glass" or tables:
        assert info["miss_after_spec"] > 0, info
    if name == "glass":
        assert info["glass"] > 0, info
    if tables:
        assert info["spec"] > 0, info


SUN_LE = 1.0e4
SUN_RHO = 0.6


def sun_scene():
    """a ground plane and three diffuse boxes (reflectance SUN_RHO at most) under a map, n = 64, that is black but for a sun of a few
    texels at radiance SUN_LE -> (tris, mats, env)"""
    q = [((-20, -1, -20), (20, -1, -20), (20, -1, 20), (-20, -1, 20))]
    q += _box((-1.2, -1, 0.6), (-0.4, -0.2, 1.4)) + _box((0.3, -1, 0.9), (0.9, 0.1, 1.5)) + _box((-0.3, -1, 2.0), (0.5, -0.5, 2.8))
    t = _quads(q)
    m = np.zeros((t.shape[0], 6), F)
    m[:, 0:3] = (SUN_RHO, 0.5, 0.4)
    env = scene.sky_environment(64, sun_dir=(0.3, 0.8, -0.5), sun_radiance=(SUN_LE,) * 3, sun_halfangle=0.05, sky_radiance=(0, 0, 0),
                                ground_radiance=(0, 0, 0))
    return t, m, env
