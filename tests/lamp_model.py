"""Lamps (point, spot and sun lights as entries of the light table), stated in numpy operation by operation: the
rules of a lamp row (scene.check_lamp_row), the light table with the lamps' entries in float64 (light_table, and under an environment map the
map's tpdf under that table's total), and the light sample in f32 with every operation rounded on its own (lamp_light).  The kernels
do not carry lamps yet: this is the statement a device function will be held to, bit for bit.

samples and render are path_model's with the step in place: for the duration of one call path_model.nee_light hands every draw that
picked a lamp's entry to lamp_light, and the table builders path_model.samples calls (scene.light_table, and under a map
env_model's scene_part and flagged_light_table) give the lamp table, so that path_model stays the one walker of a path.  With a normal
map the walker is nmap_model's, which substitutes shade_normal the same way.

Not a test module: tests/test_lamp_table.py and tests/test_lamp_model.py hold it to closed forms and to path_model."""
import numpy as np

import env_model
import nmap_model
import path_model
from model_primitives import F, INV_PI, MARGIN, TWO_OVER_PI, _dot, _philox
from spath_amd import scene

POINT, SPOT, SUN = 0, 1, 2
MAX_ROWS = scene.LAMP_MAX_ROWS
RULES = scene.LAMP_RULES
# why a draw gave no sample (0: it gave one), in the order of the header's list
SAMPLE, DIST2, COS_X, SXZ, FALLOFF = range(5)
OUTS = ("sample", "dist2", "cos_x", "sxz", "falloff")


# ---------------------------------------------------------------------------------------------------------------- the row rules
check_row = scene.check_lamp_row                                 # the one statement of the rules: (rule, field)


def first_bad_row(rows):
    """-> (row, rule, field) of the first row that breaks a rule, (n, "ok", -1) when none does"""
    rows = np.asarray(rows, F).reshape(-1, 12)
    for k, q in enumerate(rows):
        rule, field = check_row(q)
        if rule != "ok":
            return k, rule, field
    return rows.shape[0], "ok", -1


# ---------------------------------------------------------------------------------------------------------------- the light table
def light_table(tris, mats, lamps, env_tab=None):
    """the light table of a flagged render -> (tri, cdf, ipdf, W, tipdf), and under the tables env_tab of a map (env_model.tables) a
    sixth element, the map's part {"w_env", "W", "tpdf"} under this table's total.  The triangle entries, the lamps of positive
    finite weight in row order (row k as triangle -2 - k), the map's entry (triangle -1) last"""
    if env_tab is None:
        return scene.lamp_light_table(tris, mats, lamps)
    w_env = env_model.scene_part(env_tab, tris, mats)["w_env"]     # the map's weight does not depend on the other entries
    tab = scene.lamp_light_table(tris, mats, lamps, w_env)
    n, T = env_tab["n"], env_tab["T"]
    if not w_env > 0.0:
        return tab + ({"w_env": 0.0, "W": float(tab[3]), "tpdf": np.zeros((n, n), F)},)
    tpdf = (((w_env / tab[3]) * (env_tab["wt"] / T)) * (float(n) * n / 4.0)).astype(F)
    return tab + ({"w_env": float(w_env), "W": float(tab[3]), "tpdf": tpdf},)


# ---------------------------------------------------------------------------------------------------------------- the light sample
def lamp_light(rows, x, n, refl, ipdf):
    """the light sample of lamp rows [k, 12] at hits x [k, 3] of shading normal n and reflectance refl under the entries' ipdf [k]
    -> (ok, wd, tmax, L, why): why[k] is SAMPLE or the first early-out of OUTS; wd, tmax and L are 0 where there is no sample"""
    q = np.asarray(rows, F).reshape(-1, 12)
    x, n, refl = (np.asarray(v, F).reshape(-1, 3) for v in (x, n, refl))
    ipdf = np.asarray(ipdf, F).reshape(-1)
    kind = q[:, 0].astype(np.int64)
    sun, spot = kind == SUN, kind == SPOT
    a, c, ci, co = q[:, 7:10], q[:, 4:7], q[:, 10], q[:, 11]
    with np.errstate(all="ignore"):
        w = q[:, 1:4] - x
        dist2 = _dot(w, w)
        dist = np.sqrt(dist2)
        wd = np.where(sun[:, None], -a, w / dist[:, None]).astype(F)
        cos_x = _dot(wd, n)
        sxz = np.sqrt(wd[:, 0] * wd[:, 0] + wd[:, 2] * wd[:, 2])
        ca = -_dot(wd, a)
        t = (ca - co) / (ci - co)
        t = np.where(t < F(0), F(0), np.where(t > F(1), F(1), t)).astype(F)
        f = np.where(spot, (t * t) * (F(3) - (t + t)), F(1)).astype(F)
        g_near = (((cos_x / dist2) * f) * ipdf) * (TWO_OVER_PI / sxz)
        g_sun = (cos_x * ipdf) * (TWO_OVER_PI / sxz)
        g = np.where(sun, g_sun, g_near).astype(F)
        tmax = np.where(sun, env_model.MAX_DIST, dist * MARGIN).astype(F)
        L = ((refl * INV_PI) * (c * g[:, None])).astype(F)
    assert all(v.dtype == F for v in (dist2, dist, wd, cos_x, sxz, ca, t, f, g_near, g_sun, tmax, L))
    ok = [sun | (dist2 > F(0)), cos_x > F(0), sxz > F(0), sun | (f > F(0))]
    why = np.zeros(q.shape[0], np.int64)
    for code in range(len(ok), 0, -1):                            # the first failing guard wins
        why[~ok[code - 1]] = code
    hit = why == SAMPLE
    z3 = np.zeros_like(wd)
    return hit, np.where(hit[:, None], wd, z3), np.where(hit, tmax, F(0)).astype(F), np.where(hit[:, None], L, z3), why


# ---------------------------------------------------------------------------------------------------------------- the walker
class _Scene:
    """spath_amd.scene with light_table replaced: what path_model.samples sees as `scene` for the duration of a call"""

    def __init__(self, table):
        self.light_table = table

    def __getattr__(self, name):
        return getattr(scene, name)


def samples(rays, tris, mats, seed, s0, n, est, lamps, spec=None, vn=None, glass=None, env=None, rough=None, first_ns=None, collect=(),
            nmap=None, uv=None, counts=None, _walk=path_model.samples):
    """path_model.samples with the lamps of the lamp table lamps [k, 12] in the light table; with nmap and uv, under SPHIP_FLAG_NORMAL_MAP as
    well (nmap_model's walker).  counts: a dict that receives "lamp_draws", the draws that picked a lamp's entry, "lamp_<kind>" of
    those by kind, and the draws per entry of OUTS"""
    if est != "mis":
        raise ValueError("lamps are sampled under NEE|MIS alone (the plain estimator cannot see a light without area)")
    tris = np.ascontiguousarray(tris, F).reshape(-1, 12)
    mats = np.ascontiguousarray(mats, F).reshape(-1, 6)
    lamps = np.ascontiguousarray(lamps, F).reshape(-1, 12)
    keep = (path_model.nee_light, path_model.scene, path_model.scene_part, path_model.flagged_light_table, path_model.env_light)
    nee, env_sample = keep[0], keep[4]
    box = {}

    def table(t, m):
        return light_table(t, m, lamps)

    def part(tab, t, m):                                          # under a map: the table once, its part for the walker's tpdf
        box["light"] = light_table(t, m, lamps, tab)
        return box["light"][5]

    def flagged(t, m, p):
        return box["light"][:5]

    def lit(tr, mt, light, sd, pix, smp, depth, x, nrm, idx, mis):
        tri, cdf, ipdf, Wt = light[:4]
        tame = (np.where(tri < -1, 0, tri), cdf, ipdf, Wt) + tuple(light[4:])   # a lamp's row of the triangle sample is replaced below
        ok, wd, tmax, L = nee(tr, mt, tame, sd, pix, smp, depth, x, nrm, idx, mis)
        r5, _ = _philox(sd, pix, smp, 16 + depth)
        e = np.minimum(np.searchsorted(cdf, r5 * Wt, side="right"), tri.size - 1)
        q = np.flatnonzero(tri[e] < -1)
        if q.size:
            rows = lamps[-2 - tri[e[q]]]
            okq, wdq, tmq, Lq, why = lamp_light(rows, x[q], nrm[q], mt[idx[q], 0:3], ipdf[e[q]])
            ok, wd, tmax, L = ok.copy(), wd.copy(), tmax.copy(), L.copy()
            ok[q], wd[q], tmax[q], L[q] = okq, wdq, tmq, Lq
            # under a map the walker takes every negative entry for the map's and asks env_light for it: what these rows get there
            box["lamp"] = ((pix[q].astype(np.uint64) << np.uint64(32)) | smp[q].astype(np.uint64), okq, wdq, tmq, Lq, depth)
            if counts is not None:
                counts["lamp_draws"] = counts.get("lamp_draws", 0) + q.size
                for kind, name in enumerate(("point", "spot", "sun")):
                    counts["lamp_" + name] = counts.get("lamp_" + name, 0) + int((rows[:, 0] == kind).sum())
                for code, name in enumerate(OUTS):
                    counts[name] = counts.get(name, 0) + int((why == code).sum())
        else:
            box["lamp"] = None
        return ok, wd, tmax, L

    def map_or_lamp(env_, tab, tpdf, mt, sd, pix, smp, depth, nrm, idx):
        ok, wd, tmax, L, i, j = env_sample(env_, tab, tpdf, mt, sd, pix, smp, depth, nrm, idx)
        if box.get("lamp") is not None:                           # the rows of the last nee_light call that picked a lamp keep its sample
            key, okq, wdq, tmq, Lq, at_depth = box["lamp"]
            # what this leans on in the walker: its rows are ordered by pixel, then sample; it asks env_light straight after nee_light,
            # at the same depth, for every row whose entry is negative (so for every lamp row of that call)
            assert at_depth == depth, "env_light follows the nee_light call of its depth"
            assert (np.diff(key.astype(np.int64)) > 0).all(), "the rows of a nee_light call are ordered by (pixel, sample)"
            mine = (pix.astype(np.uint64) << np.uint64(32)) | smp.astype(np.uint64)
            at = np.minimum(np.searchsorted(key, mine), key.size - 1)
            r = np.flatnonzero(key[at] == mine)
            assert r.size == key.size, "every lamp row of the nee_light call is among the rows env_light is asked for"
            ok, wd, tmax, L = ok.copy(), wd.copy(), tmax.copy(), L.copy()
            ok[r], wd[r], tmax[r], L[r] = okq[at[r]], wdq[at[r]], tmq[at[r]], Lq[at[r]]
        return ok, wd, tmax, L, i, j

    path_model.nee_light, path_model.scene = lit, _Scene(table)
    path_model.scene_part, path_model.flagged_light_table, path_model.env_light = part, flagged, map_or_lamp
    try:
        if nmap is not None:
            return nmap_model.samples(rays, tris, mats, seed, s0, n, est, nmap, uv, spec, vn, glass, env, rough, first_ns, collect, _walk=_walk)
        return _walk(rays, tris, mats, seed, s0, n, est, spec, vn, glass, env, rough, first_ns, collect)
    finally:
        path_model.nee_light, path_model.scene, path_model.scene_part, path_model.flagged_light_table, path_model.env_light = keep


def render(rays, tris, mats, n, seed, est, lamps, spec=None, vn=None, glass=None, env=None, rough=None, first_ns=None, collect=(),
           nmap=None, uv=None, counts=None):
    """path_model.render of the same -> (rgba, mean, scans, info)"""
    original = path_model.samples
    path_model.samples = lambda r, t, m, sd, s0, k, e, *a: samples(r, t, m, sd, s0, k, e, lamps, *a, nmap=nmap, uv=uv, counts=counts,
                                                                   _walk=original)
    try:
        return path_model.render(rays, tris, mats, n, seed, est, spec, vn, glass, env, rough, first_ns, collect)
    finally:
        path_model.samples = original
