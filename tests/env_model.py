"""Environment lighting in the numpy model (include/spath_hip.h, "environment lighting"), operation by operation:
the octahedral lookup and the sample in f32, the importance tables in float64 with numpy's sequential cumsum, and the environment
steps that tests/path_model.py's loop (its `env` map) calls: the map's entry of the flagged light table, its light sample, and the
miss term from which the unwind of a path that left the scene starts.  The scenes and maps of the replay and their coverage check
are here too.

Not a test module: tests/test_hip_environment.py holds the device functions, the table kernels and, through path_model, the path
kernels to it at tolerance 0."""
import numpy as np

from model_primitives import F, INV_PI, PI_SQ, TWO_PI, _dot, _philox
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


# ---------------------------------------------------------------------------------------------------------------- the estimator's steps
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
