"""Scene data: triangles, materials, the reference's default scene and synthetic scenes.

Layouts are the reference's tightly packed float structs (reference src/geom.h:185-190,
src/scene.h:47-50):

    triangles : float32 [N, 12]  = v0.xyz v1.xyz v2.xyz n.xyz      (48 B, geom::triangle)
    materials : float32 [N, 6]   = reflectance.rgb emittance.rgb   (24 B, scene::material)

Everything here is IEEE float32 numpy arithmetic with separately rounded operations, so the
arrays are bit-identical on every machine.
"""
from __future__ import annotations

import struct

import numpy as np

F = np.float32
SCENE_MAGIC = 0x43535053  # 'SPSC'
SPEC_MAGIC = 0x50535053   # 'SPSP'
VNORM_MAGIC = 0x4E565053  # 'SPVN'
GLASS_MAGIC = 0x49445053  # 'SPDI'
ENV_MAGIC = 0x4E455053    # 'SPEN'
ROUGH_MAGIC = 0x47525053  # 'SPRG'
LAMP_MAGIC = 0x414C5053   # 'SPLA'


def flat_normals(tris: np.ndarray) -> np.ndarray:
    """n = unit((v1-v0) x (v2-v0)) in float32, same operation order as geom::flat_normal
    (reference src/geom.h:192-195, cross :143-145, unit :130-141)."""
    t = np.ascontiguousarray(tris, dtype=F).reshape(-1, 12).copy()
    a = t[:, 3:6] - t[:, 0:3]
    b = t[:, 6:9] - t[:, 0:3]
    cx = a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1]
    cy = a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2]
    cz = a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]
    l = np.sqrt((cx * cx + cy * cy) + cz * cz)
    t[:, 9] = cx / l
    t[:, 10] = cy / l
    t[:, 11] = cz / l
    return t


def default_scene():
    """The 7-triangle scene the reference hard-codes (values from reference src/main.cpp:185-231;
    SURVEY.md Appendix C): red pyramid face, two floor triangles, a two-triangle area light,
    a two-triangle back wall."""
    p, al, wd = 20.0, 0.75, 1.0
    v = [
        [(0.0, 0.0, 1.0), (0.5, -0.5, 0.0), (-0.5, -0.5, 0.0)],
        [(p, -1.0, p), (-p, -1.0, -p), (-p, -1.0, p)],
        [(p, -1.0, p), (p, -1.0, -p), (-p, -1.0, -p)],
        [(al, 0.75, al), (-al, 0.75, al), (al, 0.75, -al)],
        [(-al, 0.75, al), (-al, 0.75, -al), (al, 0.75, -al)],
        [(1.25, 0.5, wd), (1.25, -1.0, wd), (-1.25, -1.0, wd)],
        [(1.25, 0.5, wd), (-1.25, -1.0, wd), (-1.25, 0.5, wd)],
    ]
    tris = np.zeros((7, 12), dtype=F)
    tris[:, :9] = np.asarray(v, dtype=F).reshape(7, 9)
    tris = flat_normals(tris)
    mats = np.zeros((7, 6), dtype=F)
    mats[0, 0:3] = (1.0, 0.0, 0.0)
    mats[1, 0:3] = (0.0, 1.0, 0.0)
    mats[2, 0:3] = (0.0, 0.0, 1.0)
    mats[3] = (1.0, 1.0, 1.0, 1.0, 1.0, 1.0)
    mats[4] = (1.0, 1.0, 1.0, 1.0, 1.0, 1.0)
    mats[5, 0:3] = (1.0, 1.0, 1.0)
    mats[6, 0:3] = (1.0, 1.0, 1.0)
    return tris, mats


def _hash_u32(idx: np.ndarray, stream: int, seed: int) -> np.ndarray:
    """Counter hash (murmur3 finaliser over idx, stream, seed) -> uint32."""
    x = (idx.astype(np.uint64) * np.uint64(0x9E3779B1) + np.uint64(stream) * np.uint64(0x85EBCA77)
         + np.uint64(seed & 0xFFFFFFFF)) & np.uint64(0xFFFFFFFF)
    for mul in (0x85EBCA6B, 0xC2B2AE35):
        x ^= x >> np.uint64(16)
        x = (x * np.uint64(mul)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x27D4EB2F)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(15)
    return x.astype(np.uint32)


def _uniform(idx, stream, seed, lo, hi):
    """lo + u*(hi-lo) with u = 24-bit hash / 2^24, all float32 (exact conversions)."""
    u = (_hash_u32(idx, stream, seed) >> np.uint32(8)).astype(F) * F(1.0 / 16777216.0)
    return F(lo) + u * F(hi - lo)


def closed_room(n_tris: int, seed: int = 0x5CE11E, clutter_scale: float | None = None):
    """Synthetic closed scene of SURVEY.md section 8(d): a 12-triangle box around the default
    camera, a 2-triangle emissive ceiling panel and n_tris-14 small clutter triangles.  Closed,
    so every path runs all 5 closest-hit scans (nominal rays == executed scans, up to edge leaks).
    """
    if n_tris < 14:
        raise ValueError("closed_room needs at least 14 triangles")
    x0, x1, y0, y1, z0, z1 = -4.0, 4.0, -1.5, 2.5, -4.0, 4.0
    c = lambda x, y, z: (x, y, z)
    A, B, C, D = c(x0, y0, z0), c(x1, y0, z0), c(x1, y0, z1), c(x0, y0, z1)   # floor
    E, Fq, G, H = c(x0, y1, z0), c(x1, y1, z0), c(x1, y1, z1), c(x0, y1, z1)  # ceiling
    box = [
        (A, B, C), (A, C, D),       # floor
        (E, G, Fq), (E, H, G),      # ceiling
        (A, E, Fq), (A, Fq, B),     # z = z0 wall
        (D, C, G), (D, G, H),       # z = z1 wall
        (A, D, H), (A, H, E),       # x = x0 wall
        (B, Fq, G), (B, G, C),      # x = x1 wall
    ]
    ly, lh = 2.45, 1.5
    light = [
        (c(lh, ly, lh), c(-lh, ly, lh), c(lh, ly, -lh)),
        (c(-lh, ly, lh), c(-lh, ly, -lh), c(lh, ly, -lh)),
    ]
    tris = np.zeros((n_tris, 12), dtype=F)
    mats = np.zeros((n_tris, 6), dtype=F)
    tris[:12, :9] = np.asarray(box, dtype=F).reshape(12, 9)
    mats[:12, 0:3] = 0.75
    tris[12:14, :9] = np.asarray(light, dtype=F).reshape(2, 9)
    mats[12:14, :] = 1.0
    m = n_tris - 14
    if m > 0:
        if clutter_scale is None:
            clutter_scale = float(min(1.0, (10000.0 / max(n_tris, 1)) ** 0.5))
        idx = np.arange(m, dtype=np.uint64)
        ctr = np.stack([_uniform(idx, 0, seed, -1.5, 1.5), _uniform(idx, 1, seed, -1.0, 0.7),
                        _uniform(idx, 2, seed, -0.5, 2.0)], axis=1)
        r = F(0.025 * clutter_scale)
        for k in range(3):
            off = np.stack([_uniform(idx, 3 + 3 * k + a, seed, -1.0, 1.0) * r for a in range(3)], axis=1)
            tris[14:, 3 * k:3 * k + 3] = ctr + off
        for a in range(3):
            mats[14:, a] = _uniform(idx, 12 + a, seed, 0.2, 0.9)
    tris = flat_normals(tris)
    return tris, mats


def open_clutter(n_tris: int, seed: int = 7):
    """Small open test scene: the default scene's floor/light plus random triangles; paths may
    escape, exercising the miss path."""
    if n_tris < 7:
        raise ValueError("open_clutter needs at least the 7 default triangles")
    base_t, base_m = default_scene()
    m = n_tris - 7
    tris = np.zeros((7 + m, 12), dtype=F)
    mats = np.zeros((7 + m, 6), dtype=F)
    tris[:7], mats[:7] = base_t, base_m
    if m:
        idx = np.arange(m, dtype=np.uint64)
        ctr = np.stack([_uniform(idx, 0, seed, -1.2, 1.2), _uniform(idx, 1, seed, -0.9, 0.6),
                        _uniform(idx, 2, seed, -1.0, 0.9)], axis=1)
        for k in range(3):
            off = np.stack([_uniform(idx, 3 + 3 * k + a, seed, -0.2, 0.2) for a in range(3)], axis=1)
            tris[7:, 3 * k:3 * k + 3] = ctr + off
        for a in range(3):
            mats[7:, a] = _uniform(idx, 12 + a, seed, 0.1, 1.0)
        tris = flat_normals(tris)
    return tris, mats


def light_table(tris: np.ndarray, mats: np.ndarray):
    """The light table of next-event estimation and MIS as the library builds it once per scene (include/spath_hip.h), in numpy:
    -> (tri, cdf, ipdf, W, tipdf).  The emitters are the triangles with Esum = ((double)Er + Eg) + Eb > 0 and a positive, finite
    weight A * Esum (A in double from the f32 vertices), in ascending index; cdf is the running double sum of the weights, W its
    last entry, ipdf = float32(W / Esum).  tipdf is MIS's pdf by triangle: float32 [N], the ipdf of the triangle's entry and 0 for
    a triangle not in the table (no emittance, zero area).  The emittances must be finite and >= 0 (the library's contract)."""
    t = np.asarray(tris, F).reshape(-1, 12)
    m = np.asarray(mats, F).reshape(-1, 6)
    tri, cdf, es_l = [], [], []
    W = 0.0
    for i in range(t.shape[0]):
        e = m[i, 3:6].astype(np.float64)
        es = (e[0] + e[1]) + e[2]
        if not es > 0.0:
            continue
        v = t[i, :9].astype(np.float64)
        e1, e2 = v[3:6] - v[0:3], v[6:9] - v[0:3]
        cx = e1[1] * e2[2] - e1[2] * e2[1]
        cy = e1[2] * e2[0] - e1[0] * e2[2]
        cz = e1[0] * e2[1] - e1[1] * e2[0]
        w = (0.5 * np.sqrt((cx * cx + cy * cy) + cz * cz)) * es
        if not (w > 0.0 and np.isfinite(w)):
            continue
        W = W + w
        tri.append(i), cdf.append(W), es_l.append(es)
    ipdf = np.array([W / e for e in es_l], np.float64).astype(F)
    tri = np.array(tri, np.int64)
    tipdf = np.zeros(t.shape[0], F)
    tipdf[tri] = ipdf
    return tri, np.array(cdf, np.float64), ipdf, W, tipdf


LAMP_POINT, LAMP_SPOT, LAMP_SUN = 0, 1, 2
LAMP_MAX_ROWS = 65536


def _unit(v, what):
    v = np.asarray(v, np.float64).reshape(3)
    ln = float(np.sqrt((v * v).sum()))
    if not (np.isfinite(v).all() and ln > 0.0):
        raise ValueError(f"{what}: a finite direction of positive length")
    return (v / ln).astype(F)


def point_lamp(position, intensity) -> np.ndarray:
    """A point light for lamp_table: float32 [12], kind 0 at `position` with the radiant intensity
    (per steradian) `intensity`, a scalar or an rgb triple."""
    row = np.zeros(12, F)
    row[0] = LAMP_POINT
    row[1:4] = np.asarray(position, F).reshape(3)
    row[4:7] = np.broadcast_to(np.asarray(intensity, F), (3,))
    return row


def spot_lamp(position, direction, intensity, inner_deg: float = 20.0, outer_deg: float = 30.0) -> np.ndarray:
    """A spot light for lamp_table: float32 [12], kind 1 at `position`, its cone around `direction` (normalised here, in float64,
    rounded once), radiant intensity `intensity` on the axis, full inside the half-angle inner_deg and none outside outer_deg
    (degrees, 0 <= inner < outer <= 180); the row holds their cosines, float32(cos(radians))."""
    if not 0.0 <= float(inner_deg) < float(outer_deg) <= 180.0:
        raise ValueError("spot lamp: 0 <= inner_deg < outer_deg <= 180")
    row = np.zeros(12, F)
    row[0] = LAMP_SPOT
    row[1:4] = np.asarray(position, F).reshape(3)
    row[4:7] = np.broadcast_to(np.asarray(intensity, F), (3,))
    row[7:10] = _unit(direction, "spot lamp")
    row[10] = F(max(-1.0, min(1.0, np.cos(np.radians(float(inner_deg))))))
    row[11] = F(max(-1.0, min(1.0, np.cos(np.radians(float(outer_deg))))))
    if not row[11] < row[10]:
        raise ValueError("spot lamp: the two cosines coincide in float32")
    return row


def sun_lamp(direction, irradiance) -> np.ndarray:
    """A sun for lamp_table: float32 [12], kind 2, its light travelling along `direction` (normalised here; not the vertical: x and z
    must not both be 0) with `irradiance` on a plane facing it, a scalar or an rgb triple."""
    row = np.zeros(12, F)
    row[0] = LAMP_SUN
    row[4:7] = np.broadcast_to(np.asarray(irradiance, F), (3,))
    row[7:10] = _unit(direction, "sun lamp")
    if row[7] == 0 and row[9] == 0:
        raise ValueError("sun lamp: a vertical sun (a.x == 0 and a.z == 0) lights nothing finitely")
    return row


LAMP_FIELDS = ("kind", "p.x", "p.y", "p.z", "c.r", "c.g", "c.b", "a.x", "a.y", "a.z", "ci", "co")
LAMP_AXIS_TOL = float(F(1e-3))
# the rules of a lamp row, in the order in which a row that breaks several hears of them
LAMP_RULES = ("ok", "non_finite", "negative", "kind", "axis", "cone", "vertical", "must_be_zero")


def check_lamp_row(q):
    """THE rules of a lamp row -> (rule, field): the first rule of LAMP_RULES that q [12] breaks and the first
    float that breaks it; ("ok", -1) for a valid row.  Every value finite; c >= 0; kind 0, 1 or 2; the axis of a spot or a sun a unit
    vector (its squared length, in double, within 1e-3 of 1); a spot's -1 <= co < ci <= 1; no vertical sun (a.x == 0 and a.z == 0);
    a point's a, ci, co and a sun's p, ci, co zero."""
    q = np.asarray(q, F).reshape(12)
    for k in range(12):
        if not np.isfinite(q[k]):
            return "non_finite", k
    for k in (4, 5, 6):
        if not q[k] >= 0:
            return "negative", k
    if float(q[0]) not in (0.0, 1.0, 2.0):
        return "kind", 0
    kind = int(q[0])
    if kind != LAMP_POINT:
        a = q[7:10].astype(np.float64)
        if not abs(((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]) - 1.0) <= LAMP_AXIS_TOL:
            return "axis", 7
    if kind == LAMP_SPOT and not (q[11] >= -1 and q[11] < q[10] and q[10] <= 1):
        return "cone", 10
    if kind == LAMP_SUN and q[7] == 0 and q[9] == 0:
        return "vertical", 7
    for k in {LAMP_POINT: range(7, 12), LAMP_SPOT: (), LAMP_SUN: (1, 2, 3, 10, 11)}[kind]:
        if q[k] != 0:
            return "must_be_zero", k
    return "ok", -1


def lamp_row_message(q, row: int, rule: str, field: int) -> str:
    """What a setter says of row number `row`, q [12], that breaks `rule` at float `field`: the row, the offending values as %g prints
    them, and the rule."""
    v = [float(x) for x in np.asarray(q, F).reshape(12)]
    if rule == "non_finite":
        return "lamp table: row %d has %s = %g (every value finite)" % (row, LAMP_FIELDS[field], v[field])
    if rule == "negative":
        return "lamp table: row %d has c {%g %g %g} (c >= 0)" % (row, v[4], v[5], v[6])
    if rule == "kind":
        return "lamp table: row %d has kind %g (0 point, 1 spot, 2 sun)" % (row, v[0])
    if rule == "axis":
        return "lamp table: row %d has axis {%g %g %g} (a unit vector: |dot(a, a) - 1| <= 1e-3)" % (row, v[7], v[8], v[9])
    if rule == "cone":
        return "lamp table: row %d has {ci %g, co %g} (-1 <= co < ci <= 1)" % (row, v[10], v[11])
    if rule == "vertical":
        return ("lamp table: row %d is a sun with axis {%g %g %g} (a.x and a.z must not both be 0: a vertical sun lights nothing finitely)"
                % (row, v[7], v[8], v[9]))
    if rule == "must_be_zero":
        return "lamp table: row %d (%s) has %s = %g (must be 0 for this kind)" % (row, "point" if v[0] == 0 else "sun", LAMP_FIELDS[field], v[field])
    raise ValueError(f"no message for rule {rule!r}")


def lamp_table(*rows) -> np.ndarray:
    """The lamp table from rows of point_lamp, spot_lamp and sun_lamp (or [12] arrays, or [k, 12] blocks):
    float32 [n, 12] of at most 65536 rows, every row checked by check_lamp_row; the ValueError of the first row that breaks a rule is
    lamp_row_message's."""
    tab = np.concatenate([np.asarray(r, F).reshape(-1, 12) for r in rows]) if rows else np.zeros((0, 12), F)
    if tab.shape[0] > LAMP_MAX_ROWS:
        raise ValueError("lamp table: %d rows (at most %d)" % (tab.shape[0], LAMP_MAX_ROWS))
    for k, q in enumerate(tab):
        rule, field = check_lamp_row(q)
        if rule != "ok":
            raise ValueError(lamp_row_message(q, k, rule, field))
    return np.ascontiguousarray(tab)


def scene_R2(tris: np.ndarray) -> float:
    """A quarter of the squared diagonal of the bounding box of the scene's vertices, in double from the f32 values: the R2 of the
    environment map's weight and of a sun lamp's."""
    v = np.asarray(tris, F).reshape(-1, 12)[:, :9].reshape(-1, 3)
    ext = v.max(0).astype(np.float64) - v.min(0).astype(np.float64)
    return float(0.25 * ((ext[0] * ext[0] + ext[1] * ext[1]) + ext[2] * ext[2]))


def lamp_weights(tris: np.ndarray, lamps: np.ndarray) -> np.ndarray:
    """The weight of every lamp row in the light table's units, float64 [n]: with Csum = ((double)c.r + c.g) + c.b, a point 4 Csum, a
    spot (2 (1 - (double)co)) Csum, a sun R2 Csum (scene_R2)."""
    q = np.asarray(lamps, F).reshape(-1, 12)
    c = q[:, 4:7].astype(np.float64)
    cs = (c[:, 0] + c[:, 1]) + c[:, 2]
    R2 = scene_R2(tris)
    return np.where(q[:, 0] == LAMP_POINT, 4.0 * cs, np.where(q[:, 0] == LAMP_SPOT, (2.0 * (1.0 - q[:, 11].astype(np.float64))) * cs, R2 * cs))


def lamp_light_table(tris: np.ndarray, mats: np.ndarray, lamps: np.ndarray, w_env: float = 0.0):
    """The light table of a render with lamps, in numpy:
    -> (tri, cdf, ipdf, W, tipdf) like light_table.  The triangle entries of light_table, then every lamp of positive finite weight
    in row order (row k as triangle -2 - k), then, with w_env > 0 (the weight of an environment map's entry), triangle -1 last; W is
    the running double sum over all of them; ipdf = float32(W / Esum) for a triangle, float32(W / w) for a lamp, 0 for the map."""
    t = np.asarray(tris, F).reshape(-1, 12)
    m = np.asarray(mats, F).reshape(-1, 6)
    tri, cdf, _, W, _ = light_table(t, m)
    tri, cdf = list(tri), list(cdf)
    n_tri = len(tri)
    lw = []
    for k, w in enumerate(lamp_weights(t, lamps)):
        if not (w > 0.0 and np.isfinite(w)):
            continue
        W = W + float(w)
        tri.append(-2 - k), cdf.append(W), lw.append(float(w))
    if w_env > 0.0:
        W = W + float(w_env)
        tri.append(-1), cdf.append(W)
    tri = np.array(tri, np.int64)
    e = m[tri[:n_tri], 3:6].astype(np.float64)
    ipdf = np.zeros(tri.size, F)
    ipdf[:n_tri] = (W / ((e[:, 0] + e[:, 1]) + e[:, 2])).astype(F)
    ipdf[n_tri:n_tri + len(lw)] = (W / np.array(lw, np.float64)).astype(F)
    tipdf = np.zeros(t.shape[0], F)
    tipdf[tri[:n_tri]] = ipdf[:n_tri]
    return tri, np.array(cdf, np.float64), ipdf, W, tipdf


def write_lamps(path, lamps: np.ndarray) -> None:
    """Lamp file, in the format of the other table files: 'SPLA', n, n * 12 float32."""
    _write_table(path, LAMP_MAGIC, lamps, 12)


def specular_table(tris: np.ndarray, mats: np.ndarray, ks=0.0, which=None, p=None) -> np.ndarray:
    """A specular table for capi.Context.set_specular (include/spath_hip.h, "specular reflection"): float32 [N, 4] rows ks.r ks.g ks.b p.
    ks: the mirror reflectance, a scalar, an rgb triple or an [N, 3] array (finite, >= 0); which: the triangles that get it (an index
    array or a boolean mask; None = all), every other row is zero (the triangle stays as it is).  p, the probability of the mirror
    lobe, is the given value (a scalar or [N], in [0, 1]) or, when None, the share of the mirror in what the triangle reflects:
        s = ((double)ks.r + ks.g) + ks.b,  r = ((double)rho.r + rho.g) + rho.b  (rho: the material's reflectance),
        p = float32(s / (s + r)) where s > 0, else 0
    so a triangle with no diffuse reflectance becomes a pure mirror (p = 1) and one with ks = 0 stays diffuse (p = 0).  Any p in
    (0, 1) gives the same expectation; this one spends the samples where the energy goes."""
    t = np.asarray(tris, F).reshape(-1, 12)
    m = np.asarray(mats, F).reshape(-1, 6)
    n = t.shape[0]
    if m.shape[0] != n:
        raise ValueError("one material per triangle")
    sel = np.ones(n, bool) if which is None else np.zeros(n, bool)
    if which is not None:
        sel[np.asarray(which)] = True
    spec = np.zeros((n, 4), F)
    spec[:, 0:3] = np.broadcast_to(np.asarray(ks, F), (n, 3)) if np.ndim(ks) else F(ks)
    if p is None:
        k64, r64 = spec[:, 0:3].astype(np.float64), m[:, 0:3].astype(np.float64)
        s = (k64[:, 0] + k64[:, 1]) + k64[:, 2]
        r = (r64[:, 0] + r64[:, 1]) + r64[:, 2]
        with np.errstate(invalid="ignore", divide="ignore"):
            spec[:, 3] = np.where(s > 0.0, s / (s + r), 0.0).astype(F)
    else:
        spec[:, 3] = np.broadcast_to(np.asarray(p, F), (n,))
    spec[~sel] = 0.0
    if not (np.isfinite(spec).all() and (spec >= 0).all() and (spec[:, 3] <= 1).all()):
        raise ValueError("specular table: every value finite, ks >= 0, 0 <= p <= 1")
    return spec


def _write_table(path, magic: int, rows: np.ndarray, width: int) -> None:
    """The 'magic, n, rows' file of a per-triangle table: u32 magic, u32 n, then n x width float32."""
    rows = np.ascontiguousarray(rows, dtype=F).reshape(-1, width)
    with open(path, "wb") as f:
        f.write(struct.pack("<II", magic, rows.shape[0]))
        f.write(rows.tobytes())


def write_specular(path, spec: np.ndarray) -> None:
    """Specular file read by the headless CLI (--spec), beside the scene file: 'SPSP', n, n * 4 float32."""
    _write_table(path, SPEC_MAGIC, spec, 4)


def dielectric_table(tris: np.ndarray, ior=1.5, kt=1.0, which=None) -> np.ndarray:
    """A dielectric table for capi.Context.set_dielectric (include/spath_hip.h, "transparency"): float32 [N, 4] rows kt.r kt.g kt.b ior.
    ior: the index of the dielectric behind the triangle's stored normal, a scalar or [N] (finite, >= 1); kt: the tint of what is
    transmitted, a scalar, an rgb triple or an [N, 3] array (finite, >= 0); which: the triangles that get the row (an index array or
    a boolean mask; None = all), every other row is zero (the triangle stays as it is)."""
    t = np.asarray(tris, F).reshape(-1, 12)
    n = t.shape[0]
    sel = np.ones(n, bool) if which is None else np.zeros(n, bool)
    if which is not None:
        sel[np.asarray(which)] = True
    g = np.zeros((n, 4), F)
    g[:, 0:3] = np.broadcast_to(np.asarray(kt, F), (n, 3)) if np.ndim(kt) else F(kt)
    g[:, 3] = np.broadcast_to(np.asarray(ior, F), (n,))
    if not (np.isfinite(g).all() and (g[:, 0:3] >= 0).all() and (g[:, 3] >= 1).all()):
        raise ValueError("dielectric table: every value finite, kt >= 0, ior >= 1")
    g[~sel] = 0.0
    return g


def write_dielectric(path, glass: np.ndarray) -> None:
    """Dielectric file read by the headless CLI (--glass), beside the scene file: 'SPDI', n, n * 4 float32."""
    _write_table(path, GLASS_MAGIC, glass, 4)


def roughness_table(tris: np.ndarray, alpha=0.2, which=None) -> np.ndarray:
    """A roughness table for capi.Context.set_roughness (include/spath_hip.h, "glossy reflection"): float32 [N], the GGX alpha of each
    triangle's mirror lobe.  alpha: a scalar or [N] (finite, in [0, 1]); which: the triangles that get the value (an index array or a
    boolean mask; None = all), every other row is zero (the lobe stays the perfect mirror)."""
    t = np.asarray(tris, F).reshape(-1, 12)
    n = t.shape[0]
    sel = np.ones(n, bool) if which is None else np.zeros(n, bool)
    if which is not None:
        sel[np.asarray(which)] = True
    a = np.broadcast_to(np.asarray(alpha, F), (n,)).copy()
    if not (np.isfinite(a).all() and (a >= 0).all() and (a <= 1).all()):
        raise ValueError("roughness table: every value finite and in [0, 1]")
    a[~sel] = 0.0
    return a


def write_roughness(path, alpha: np.ndarray) -> None:
    """Roughness file read by the headless CLI (--rough), beside the scene file: 'SPRG', n, n float32."""
    _write_table(path, ROUGH_MAGIC, alpha, 1)


def checker_texture(tw: int = 16, th: int = 16, cell: int = 4, a=(0.9, 0.9, 0.9), b=(0.2, 0.2, 0.2)) -> np.ndarray:
    """A checkerboard atlas for capi.Context.set_texture (include/spath_hip.h, "textures"): float32 [th, tw, 3] indexed [j, i], cells of
    cell x cell texels coloured a where (i // cell + j // cell) is even and b where it is odd."""
    if not (1 <= tw <= 4096 and 1 <= th <= 4096 and cell >= 1):
        raise ValueError("checker texture: 1 <= tw, th <= 4096 and cell >= 1")
    i, j = np.meshgrid(np.arange(tw), np.arange(th))
    odd = ((i // cell + j // cell) & 1).astype(bool)
    tex = np.where(odd[..., None], np.asarray(b, F), np.asarray(a, F)).astype(F)
    if not (np.isfinite(tex).all() and (tex >= 0).all()):
        raise ValueError("checker texture: every value finite and >= 0")
    return np.ascontiguousarray(tex)


def uv_table(tris: np.ndarray, uv=(0.0, 0.0, 1.0, 0.0, 0.0, 1.0), which=None) -> np.ndarray:
    """A UV table for capi.Context.set_uv (include/spath_hip.h, "textures"): float32 [N, 6], s0 t0 s1 t1 s2 t2 for v0 v1 v2.  uv: one
    row for all or [N, 6] (finite); which: the triangles that get their row (an index array or a boolean mask; None = all), every other
    row is zero (the triangle stays untextured)."""
    t = np.asarray(tris, F).reshape(-1, 12)
    n = t.shape[0]
    sel = np.ones(n, bool) if which is None else np.zeros(n, bool)
    if which is not None:
        sel[np.asarray(which)] = True
    rows = np.broadcast_to(np.asarray(uv, F).reshape(-1, 6), (n, 6)).copy()
    if not np.isfinite(rows).all():
        raise ValueError("UV table: every value finite")
    rows[~sel] = 0.0
    return rows


def planar_uv(tris: np.ndarray, origin=(0.0, 0.0, 0.0), s_axis=(1.0, 0.0, 0.0), t_axis=(0.0, 0.0, 1.0), which=None) -> np.ndarray:
    """The UV table of a planar projection: vertex p gets s = (p - origin) . s_axis, t = (p - origin) . t_axis (float64, rounded once),
    so one repeat of the atlas covers 1 / |axis| world units.  which as in uv_table."""
    t = np.asarray(tris, F).reshape(-1, 12)
    p = t[:, :9].reshape(-1, 3, 3).astype(np.float64) - np.asarray(origin, np.float64)
    rows = np.stack([p @ np.asarray(s_axis, np.float64), p @ np.asarray(t_axis, np.float64)], axis=2).reshape(-1, 6)
    return uv_table(t, rows.astype(F), which)


def write_texture(path, texels: np.ndarray) -> None:
    """Atlas file read by the headless CLI (--tex): u32 tw, u32 th, then th x tw x {r g b} float32."""
    texels = np.ascontiguousarray(texels, dtype=F)
    if texels.ndim != 3 or texels.shape[2] != 3:
        raise ValueError("an atlas is (th, tw, 3)")
    with open(path, "wb") as f:
        f.write(struct.pack("<II", texels.shape[1], texels.shape[0]))
        f.write(texels.tobytes())


def normal_map_from_height(height, strength: float = 1.0) -> np.ndarray:
    """A normal map for capi.Context.set_normal_map (include/spath_hip.h, "normal mapping") from a height field [nh, nw] indexed
    [j, i]: central differences with repeat wrap, dx = (h[j, i + 1] - h[j, i - 1]) / 2 and dy likewise along j (per texel), and the
    unit vector of (-strength dx, -strength dy, 1) in float64, rounded once: float32 [nh, nw, 3] with z > 0; a constant height gives
    (0, 0, 1) exactly."""
    h = np.asarray(height, np.float64)
    if h.ndim != 2 or not (1 <= h.shape[0] <= 4096 and 1 <= h.shape[1] <= 4096) or not np.isfinite(h).all():
        raise ValueError("normal map: a finite height field [nh, nw], 1 <= nw, nh <= 4096")
    dx = (np.roll(h, -1, axis=1) - np.roll(h, 1, axis=1)) / 2.0
    dy = (np.roll(h, -1, axis=0) - np.roll(h, 1, axis=0)) / 2.0
    v = np.stack([-float(strength) * dx, -float(strength) * dy, np.ones_like(h)], axis=2)
    return np.ascontiguousarray((v / np.sqrt((v * v).sum(axis=2, keepdims=True))).astype(F))


def decode_normal_map(rgb01) -> np.ndarray:
    """The signed vectors of a normal map stored in the 0..1 encoding of image files: 2 c - 1 per component, float32 [nh, nw, 3]."""
    c = np.asarray(rgb01, F)
    if c.ndim != 3 or c.shape[2] != 3:
        raise ValueError("a normal map is (nh, nw, 3)")
    return np.ascontiguousarray(F(2.0) * c - F(1.0))


def write_normal_map(path, texels: np.ndarray) -> None:
    """Normal map file read by the headless CLI (--nmap): 'SPNM', u32 nw, u32 nh, then nh x nw x {x y z} float32 (the atlas file's layout
    behind a magic of its own)."""
    texels = np.ascontiguousarray(texels, dtype=F)
    if texels.ndim != 3 or texels.shape[2] != 3:
        raise ValueError("a normal map is (nh, nw, 3)")
    with open(path, "wb") as f:
        f.write(b"SPNM" + struct.pack("<II", texels.shape[1], texels.shape[0]))
        f.write(texels.tobytes())


def read_normal_map(path) -> np.ndarray:
    """The float32 [nh, nw, 3] texels of a file written by write_normal_map."""
    with open(path, "rb") as f:
        raw = f.read()
    if raw[:4] != b"SPNM" or len(raw) < 12:
        raise ValueError("not a normal map file")
    nw, nh = struct.unpack("<II", raw[4:12])
    if len(raw) != 12 + nw * nh * 12:
        raise ValueError("normal map file: size and header differ")
    return np.frombuffer(raw, F, offset=12).reshape(nh, nw, 3).copy()


def write_uv(path, uv: np.ndarray) -> None:
    """UV file read by the headless CLI (--uv), beside the scene file: n_tris x 6 float32, no header."""
    with open(path, "wb") as f:
        f.write(np.ascontiguousarray(uv, dtype=F).reshape(-1, 6).tobytes())


def octahedral_directions(n: int) -> np.ndarray:
    """The unit directions of the texel centres of an n x n octahedral environment map (include/spath_hip.h, "environment lighting"):
    float64 [n, n, 3] indexed [j, i], texel (i, j) centred at (a, b) = (-1 + (2 i + 1) / n, -1 + (2 j + 1) / n), +y at the centre of the
    square and -y at its corners."""
    c = -1.0 + (2.0 * np.arange(n) + 1.0) / n
    a, b = np.meshgrid(c, c, indexing="xy")
    y = (1.0 - np.abs(a)) - np.abs(b)
    x = np.where(y >= 0, a, (1.0 - np.abs(b)) * np.where(a < 0, -1.0, 1.0))
    z = np.where(y >= 0, b, (1.0 - np.abs(a)) * np.where(b < 0, -1.0, 1.0))
    g = np.stack([x, y, z], axis=-1)
    return g / np.sqrt((g * g).sum(-1, keepdims=True))


def sky_environment(n: int, sun_dir=(0.3, 0.8, 0.5), sun_radiance=(50.0, 45.0, 35.0), sun_halfangle: float = 0.1,
                    sky_radiance=(0.4, 0.6, 1.0), ground_radiance=(0.15, 0.12, 0.1)) -> np.ndarray:
    """A procedural environment map for capi.Context.set_environment: float32 [n, n, 3] indexed [j, i].  Above the horizon the sky's
    radiance fades linearly with the direction's height from the full value at the zenith to half of it at the horizon; below it the
    ground's radiance is constant; every texel whose centre lies within sun_halfangle (radians) of sun_dir has the sun's radiance added."""
    d = octahedral_directions(n)
    up = d[..., 1:2]
    env = np.where(up >= 0, np.asarray(sky_radiance, np.float64) * (0.5 + 0.5 * up), np.asarray(ground_radiance, np.float64))
    sd = np.asarray(sun_dir, np.float64)
    sd = sd / np.sqrt((sd * sd).sum())
    sun = (d * sd).sum(-1) >= np.cos(sun_halfangle)
    env = env + sun[..., None] * np.asarray(sun_radiance, np.float64)
    env = env.astype(F)
    if not (np.isfinite(env).all() and (env >= 0).all()):
        raise ValueError("environment map: every value finite and >= 0")
    return env


def environment_from_latlong(img: np.ndarray, n: int) -> np.ndarray:
    """Resample a latitude-longitude radiance image [h, w, 3] (y up: row 0 is the zenith, the last row the nadir; column 0 is the
    direction -z, the azimuth atan2(x, -z) grows with the column) to an n x n octahedral map, float32 [n, n, 3] indexed [j, i].
    Every texel takes the bilinear sample of the image at its centre's direction (wrapping in azimuth, clamping at the poles).  A host-side
    convenience in float64, not part of the bit-exact contract; a map much smaller than the image undersamples it (shrink the image first)."""
    img = np.asarray(img, np.float64)
    if img.ndim != 3 or img.shape[2] != 3:
        raise ValueError("a lat-long image is (h, w, 3)")
    h, w = img.shape[:2]
    d = octahedral_directions(n)
    u = (np.arctan2(d[..., 0], -d[..., 2]) / (2.0 * np.pi)) % 1.0 * w - 0.5
    v = np.arccos(np.clip(d[..., 1], -1.0, 1.0)) / np.pi * h - 0.5
    u0, v0 = np.floor(u), np.floor(v)
    fu, fv = (u - u0)[..., None], (v - v0)[..., None]
    x0, x1 = u0.astype(np.int64) % w, (u0.astype(np.int64) + 1) % w
    y0, y1 = np.clip(v0.astype(np.int64), 0, h - 1), np.clip(v0.astype(np.int64) + 1, 0, h - 1)
    env = (img[y0, x0] * (1 - fu) + img[y0, x1] * fu) * (1 - fv) + (img[y1, x0] * (1 - fu) + img[y1, x1] * fu) * fv
    return np.maximum(env, 0.0).astype(F)


def write_environment(path, env: np.ndarray) -> None:
    """Environment file, a file of its own beside the scene file: 'SPEN', n, n * n * 3 float32 (texel (i, j) at [(j * n + i) * 3])."""
    env = np.ascontiguousarray(env, dtype=F)
    if env.ndim != 3 or env.shape[0] != env.shape[1] or env.shape[2] != 3:
        raise ValueError("an environment map is (n, n, 3)")
    with open(path, "wb") as f:
        f.write(struct.pack("<II", ENV_MAGIC, env.shape[0]))
        f.write(env.tobytes())


def vertex_normals(tris: np.ndarray, crease_deg: float = 180.0, which=None) -> np.ndarray:
    """Per-vertex normals for capi.Context.set_vertex_normals (include/spath_hip.h, "smooth shading"): float32 [N, 9] rows n0.xyz n1.xyz
    n2.xyz.  The normal of vertex k of triangle i is the double-precision sum of cross(e1, e2) (the area-weighted face normals, from
    the f32 vertices) over the triangles j that have a vertex at the same position bitwise and whose face normal lies within
    crease_deg of triangle i's (the cosine of the two unit face normals, in double, >= cos(crease_deg); i itself always counts),
    normalised and cast to float32.  crease_deg = 0 therefore returns the face normals, 180 smooths everything that touches.
    which: the triangles that get normals (an index array or a boolean mask; None = all), every other row is zero (the triangle
    stays flat).  Zero-area triangles get zero rows."""
    t = np.asarray(tris, F).reshape(-1, 12)
    n = t.shape[0]
    sel = np.ones(n, bool) if which is None else np.zeros(n, bool)
    if which is not None:
        sel[np.asarray(which)] = True
    v = t[:, :9].astype(np.float64).reshape(n, 3, 3)
    fn = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    ln = np.sqrt((fn * fn).sum(1))
    with np.errstate(invalid="ignore", divide="ignore"):
        un = np.where(ln[:, None] > 0.0, fn / ln[:, None], 0.0)
    share = {}
    for i in range(n):
        for k in range(3):
            share.setdefault(t[i, 3 * k:3 * k + 3].tobytes(), []).append(i)
    cos_c = np.cos(np.deg2rad(min(max(float(crease_deg), 0.0), 180.0)))
    out = np.zeros((n, 9), F)
    for i in np.nonzero(sel & (ln > 0.0))[0]:
        for k in range(3):
            js = np.asarray(share[t[i, 3 * k:3 * k + 3].tobytes()])
            if crease_deg >= 180.0:                               # everything that touches: a dot product of opposite unit normals may round below -1
                keep = np.ones(js.size, bool)
            elif crease_deg <= 0.0:
                keep = js == i
            else:
                keep = (un[js] @ un[i] >= cos_c) | (js == i)
            m = fn[js[keep]].sum(0)
            l = np.sqrt((m * m).sum())
            if l > 0.0:
                out[i, 3 * k:3 * k + 3] = (m / l).astype(F)
    return out


def write_vertex_normals(path, vn: np.ndarray) -> None:
    """Vertex-normal file read by the headless CLI (--normals), beside the scene file: 'SPVN', n, n * 9 float32."""
    _write_table(path, VNORM_MAGIC, vn, 9)


def icosphere(subdiv: int, centre=(0.0, 0.0, 0.0), radius: float = 1.0, material=(0.8, 0.8, 0.8, 0.0, 0.0, 0.0)):
    """A curved test object: an icosahedron subdivided subdiv times (20 * 4^subdiv triangles), every vertex pushed onto the sphere
    of the given centre and radius.  -> (tris [N, 12], mats [N, 6]) float32 with outward flat_normals; a vertex shared by several
    triangles has the same bits in each (one vertex table, computed in double and cast once), which is what vertex_normals joins."""
    g = (1.0 + 5.0 ** 0.5) / 2.0
    vs = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1), (-g, 0, -1), (-g, 0, 1)]
    vs = [tuple(np.asarray(p, np.float64) / np.sqrt(1.0 + g * g)) for p in vs]
    fs = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
          (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(int(subdiv)):
        mid, nf = {}, []

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = (np.asarray(vs[a]) + np.asarray(vs[b])) * 0.5
                vs.append(tuple(p / np.sqrt((p * p).sum())))
                mid[key] = len(vs) - 1
            return mid[key]
        for a, b, c in fs:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        fs = nf
    pos = (np.asarray(centre, np.float64) + float(radius) * np.asarray(vs, np.float64)).astype(F)
    tris = np.zeros((len(fs), 12), F)
    tris[:, :9] = pos[np.asarray(fs)].reshape(-1, 9)
    tris = flat_normals(tris)
    mats = np.tile(np.asarray(material, F).reshape(1, 6), (len(fs), 1))
    return tris, mats


def write_scene(path, tris: np.ndarray, mats: np.ndarray) -> None:
    """Scene file read by oracle/ref_driver.cpp and the headless CLI: 'SPSC', n, tris, mats."""
    tris = np.ascontiguousarray(tris, dtype=F).reshape(-1, 12)
    mats = np.ascontiguousarray(mats, dtype=F).reshape(-1, 6)
    assert tris.shape[0] == mats.shape[0]
    with open(path, "wb") as f:
        f.write(struct.pack("<II", SCENE_MAGIC, tris.shape[0]))
        f.write(tris.tobytes())
        f.write(mats.tobytes())


def read_scene(path):
    with open(path, "rb") as f:
        magic, n = struct.unpack("<II", f.read(8))
        if magic != SCENE_MAGIC:
            raise ValueError(f"{path}: not a spath scene file")
        tris = np.frombuffer(f.read(n * 48), dtype=F).reshape(n, 12).copy()
        mats = np.frombuffer(f.read(n * 24), dtype=F).reshape(n, 6).copy()
    return tris, mats
