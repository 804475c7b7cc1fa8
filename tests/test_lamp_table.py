"""Lamps in numpy: point, spot and sun lights as entries of the light table.  The rules of a lamp row, the light
table with the lamps' entries (scene.lamp_light_table, tests/lamp_model.py) and the light sample lamp_light against closed forms in
float64; the scene.py helpers.  No GPU and no library: the kernels do not carry lamps yet."""
import struct

import numpy as np
import pytest

import env_model as em
import lamp_model as lm
from path_model import F, _bits
from spath_amd import scene

EPS = 2.0 ** -24


# ---------------------------------------------------------------------------------------------------------------- the light table
def _room_lamps():
    return scene.lamp_table(scene.point_lamp((0.5, 1.0, -1.0), (3.0, 2.5, 2.0)), scene.spot_lamp((-1, 1.5, 0), (0.3, -1, 0.2), 8.0, 15, 40),
                            scene.sun_lamp((0.3, -0.8, 0.5), (2.0, 1.9, 1.5)))


@pytest.mark.parametrize("name", ["triangles", "lamps", "both", "both+map", "black"])
def test_light_table_shapes(name):
    """the five shapes of a table: triangles only (scene.light_table itself, bit for bit); lamps only (a room whose emittance is
    zeroed: a non-empty table); both; both plus a map's entry, which stays last; a black lamp between two lit ones, which is skipped
    and leaves the others their row numbers"""
    t, m = scene.closed_room(60)
    lamps, w_env = _room_lamps(), 0.0
    if name == "triangles":
        lamps = np.zeros((0, 12), F)
    elif name == "lamps":
        m = m.copy()
        m[:, 3:6] = 0
    elif name == "both+map":
        w_env = em.scene_part(em.tables(scene.sky_environment(8)), t, m)["w_env"]
        assert w_env > 0
    elif name == "black":
        lamps = lamps.copy()
        lamps[1, 4:7] = 0
    plain = scene.light_table(t, m)
    got = scene.lamp_light_table(t, m, lamps, w_env)
    model = lm.light_table(t, m, lamps)[:5] if w_env == 0 else lm.light_table(t, m, lamps, em.tables(scene.sky_environment(8)))[:5]
    assert all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(got, model))
    n_tri = plain[0].size
    R2 = scene.scene_R2(t)
    if name == "triangles":
        assert all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(got, plain))
        assert np.array_equal(_bits(got[2]), _bits(plain[2]))
    elif name == "lamps":
        assert n_tri == 0 and got[0].tolist() == [-2, -3, -4] and got[3] > 0 and not got[4].any()
    elif name == "both":
        assert got[0][:n_tri].tolist() == plain[0].tolist() and got[0][n_tri:].tolist() == [-2, -3, -4]
    elif name == "both+map":
        assert got[0][n_tri:].tolist() == [-2, -3, -4, -1] and got[2][-1] == 0 and got[1][-1] == got[3]
        part = lm.light_table(t, m, lamps, em.tables(scene.sky_environment(8)))[5]
        assert part["W"] == got[3] and part["tpdf"].dtype == F and (part["tpdf"] <= em.scene_part(em.tables(scene.sky_environment(8)), t, m)["tpdf"]).all()
    else:
        assert got[0][n_tri:].tolist() == [-2, -4]
    w = scene.lamp_weights(t, lamps)
    cs = lamps[:, 4:7].astype(np.float64).sum(1)
    assert np.allclose(w, [4 * cs[k] if lamps[k, 0] == 0 else 2 * (1 - float(lamps[k, 11])) * cs[k] if lamps[k, 0] == 1 else R2 * cs[k]
                           for k in range(lamps.shape[0])], rtol=1e-15)
    if name in ("both", "both+map"):
        assert np.allclose(np.diff(got[1])[n_tri - 1:n_tri + 2], w, rtol=1e-12)
        assert np.array_equal(got[2][n_tri:n_tri + 3], (got[3] / w).astype(F))
        e = m[got[0][:n_tri], 3:6].astype(np.float64)
        assert np.array_equal(got[2][:n_tri], (got[3] / ((e[:, 0] + e[:, 1]) + e[:, 2])).astype(F))


# ---------------------------------------------------------------------------------------------------------------- the row rules
POINT = [0, 1, 2, 3, 1, 1, 1, 0, 0, 0, 0, 0]
SPOT = [1, 1, 2, 3, 1, 1, 1, 0, -1, 0, 0.9, 0.5]
SUN = [2, 0, 0, 0, 1, 1, 1, 0.6, -0.8, 0, 0, 0]


def _with(row, **kv):
    r = list(row)
    for k, v in kv.items():
        r[int(k[1:])] = v
    return r


RULE_CASES = [
    ([POINT, SPOT, SUN], 3, "ok", None),
    ([POINT, _with(SPOT, f2=float("nan"))], 1, "non_finite", "lamp table: row 1 has p.y = nan (every value finite)"),
    ([_with(SUN, f11=float("-inf"))], 0, "non_finite", "lamp table: row 0 has co = -inf (every value finite)"),
    ([POINT, POINT, _with(POINT, f5=-0.5)], 2, "negative", "lamp table: row 2 has c {1 -0.5 1} (c >= 0)"),
    ([_with(POINT, f0=3)], 0, "kind", "lamp table: row 0 has kind 3 (0 point, 1 spot, 2 sun)"),
    ([_with(POINT, f0=0.5)], 0, "kind", "lamp table: row 0 has kind 0.5 (0 point, 1 spot, 2 sun)"),
    ([_with(SPOT, f8=-1.01)], 0, "axis", "lamp table: row 0 has axis {0 -1.01 0} (a unit vector: |dot(a, a) - 1| <= 1e-3)"),
    ([_with(SUN, f7=0, f8=0, f9=0)], 0, "axis", "lamp table: row 0 has axis {0 0 0} (a unit vector: |dot(a, a) - 1| <= 1e-3)"),
    ([_with(SPOT, f10=0.5, f11=0.5)], 0, "cone", "lamp table: row 0 has {ci 0.5, co 0.5} (-1 <= co < ci <= 1)"),
    ([_with(SPOT, f10=1.5)], 0, "cone", "lamp table: row 0 has {ci 1.5, co 0.5} (-1 <= co < ci <= 1)"),
    ([_with(SPOT, f11=-1.5)], 0, "cone", "lamp table: row 0 has {ci 0.9, co -1.5} (-1 <= co < ci <= 1)"),
    ([_with(SUN, f7=0, f8=-1, f9=0)], 0, "vertical",
     "lamp table: row 0 is a sun with axis {0 -1 0} (a.x and a.z must not both be 0: a vertical sun lights nothing finitely)"),
    ([_with(POINT, f8=1)], 0, "must_be_zero", "lamp table: row 0 (point) has a.y = 1 (must be 0 for this kind)"),
    ([_with(POINT, f10=0.5)], 0, "must_be_zero", "lamp table: row 0 (point) has ci = 0.5 (must be 0 for this kind)"),
    ([_with(SUN, f1=2)], 0, "must_be_zero", "lamp table: row 0 (sun) has p.x = 2 (must be 0 for this kind)"),
    ([_with(SUN, f11=0.25)], 0, "must_be_zero", "lamp table: row 0 (sun) has co = 0.25 (must be 0 for this kind)"),
]


@pytest.mark.parametrize("rows,bad,rule,message", RULE_CASES)
def test_row_rules_and_messages(rows, bad, rule, message):
    """every rule of a lamp row, the row it names and its message as literals: scene.check_lamp_row is the one statement of the rules
    (lamp_model reads it), scene.lamp_row_message of the messages, and scene.lamp_table refuses the table with exactly that message"""
    got_bad, got_rule, field = lm.first_bad_row(rows)
    assert (got_bad, got_rule) == (bad, rule)
    if rule == "ok":
        assert message is None and field == -1 and scene.lamp_table(np.asarray(rows, F)).shape == (len(rows), 12)
        return
    assert scene.lamp_row_message(rows[bad], bad, rule, field) == message
    with pytest.raises(ValueError) as e:
        scene.lamp_table(np.asarray(rows, F))
    assert str(e.value) == message


def test_axis_tolerance_and_row_limit():
    """an axis whose squared length is off 1 by 1e-3 or less passes, by more fails; 65536 rows pass, 65537 do not"""
    for scale, rule in ((1.0004, "ok"), (0.9996, "ok"), (1.0006, "axis"), (0.9994, "axis")):
        assert lm.check_row(_with(SUN, f7=0.6 * scale, f8=-0.8 * scale))[0] == rule, scale
    assert scene.lamp_table(np.tile(np.asarray(POINT, F), (65536, 1))).shape[0] == lm.MAX_ROWS
    with pytest.raises(ValueError) as e:
        scene.lamp_table(np.tile(np.asarray(POINT, F), (65537, 1)))
    assert str(e.value) == "lamp table: 65537 rows (at most 65536)"


# ---------------------------------------------------------------------------------------------------------------- the light sample
def _hits(n, seed):
    """random hits -> (x, unit normals, reflectances, ipdf)"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-2, 2, (n, 3)).astype(F)
    nn = rng.normal(size=(n, 3))
    nn = (nn / np.linalg.norm(nn, axis=1)[:, None]).astype(F)
    return x, nn, rng.uniform(0.1, 0.9, (n, 3)).astype(F), rng.uniform(0.5, 50, n).astype(F)


def _closed_form(rows, x, n, refl, ipdf, f):
    """L in float64 from the f32 inputs: (refl / pi) c (cos / d^2) f ipdf (2 / pi) / sxz, without 1 / d^2 for a sun -> (L, M): M the same
    with 1 for the cosine and for f, the magnitude no cancellation reaches"""
    q = rows.astype(np.float64)
    x, n, refl, ipdf = (v.astype(np.float64) for v in (x, n, refl, ipdf))
    sun = q[:, 0] == 2
    w = q[:, 1:4] - x
    d2 = (w * w).sum(1)
    wd = np.where(sun[:, None], -q[:, 7:10], w / np.sqrt(d2)[:, None])
    sxz = np.hypot(wd[:, 0], wd[:, 2])
    M = (refl / np.pi) * q[:, 4:7] * (np.where(sun, 1.0, 1.0 / d2) * ipdf * (2 / np.pi) / sxz)[:, None]
    return M * ((wd * n).sum(1) * f)[:, None], M, wd


@pytest.mark.parametrize("kind", ["point", "spot", "sun"])
def test_lamp_light_against_closed_forms(kind):
    """lamp_light on 400 random hits per kind against the closed form in float64 of the same f32 inputs: inverse square, the cosine at
    the hit, the spot's smoothstep in float64.

    The bound.  eps = 2^-24.  Every f32 operation adds at most eps relative to its result.  Up to the cosine everything is a sum of
    squares, a square root, a quotient or a product of positive terms: w (1), dist2 (3: products and sums of positives), dist (0.5 x 4 +
    1), wd (1 + 3), sxz (0.5 x (2 x 5 + 3) + 1), then the four products and two quotients of g (6) and the three of L (3): under 32 eps
    in all, relative to the product M of the closed form's factors without the cosine.  The cosine is a dot product of unit vectors and
    may cancel: its error is at most (5 + 3) eps ABSOLUTE, which is relative to M again.  So |L - L64| <= 40 eps M for a point and a sun.
    The smoothstep adds an absolute error in f: t = (ca - co) / (ci - co) carries the cosine's 8 eps and 2 more over ci - co, and
    |f'| <= 1.5, f's own four operations 4 eps: 15 eps / (ci - co) + 4 eps, so a spot's bound is (44 + 15 / (ci - co)) eps M."""
    x, n, refl, ipdf = _hits(400, {"point": 1, "spot": 2, "sun": 3}[kind])
    rng = np.random.default_rng(7)
    if kind == "point":
        rows = np.stack([scene.point_lamp(rng.uniform(-3, 3, 3), rng.uniform(0.5, 9, 3)) for _ in range(400)])
    elif kind == "spot":
        rows = np.stack([scene.spot_lamp(rng.uniform(-3, 3, 3), rng.normal(size=3), rng.uniform(0.5, 9, 3), 50, 120) for _ in range(400)])
    else:
        rows = np.stack([scene.sun_lamp(rng.normal(size=3), rng.uniform(0.5, 9, 3)) for _ in range(400)])
    ok, wd, tmax, L, why = lm.lamp_light(rows, x, n, refl, ipdf)
    q = rows.astype(np.float64)
    wd64 = _closed_form(rows, x, n, refl, ipdf, np.ones(400))[2]
    f = np.ones(400)
    K = np.full(400, 40.0)
    if kind == "spot":
        t = np.clip((-(wd64 * q[:, 7:10]).sum(1) - q[:, 11]) / (q[:, 10] - q[:, 11]), 0, 1)
        f = t * t * (3 - 2 * t)
        K = 44 + 15 / (q[:, 10] - q[:, 11])
    L64, M, _ = _closed_form(rows, x, n, refl, ipdf, f)
    assert 100 < ok.sum() < 400 and (why[~ok] != lm.SAMPLE).all()
    assert (np.abs(L[ok].astype(np.float64) - L64[ok]) <= (K[:, None] * EPS * M)[ok]).all()
    assert (np.abs(wd[ok].astype(np.float64) - wd64[ok]) <= 4 * EPS).all()
    d = np.sqrt(((q[:, 1:4] - x) ** 2).sum(1))
    want_tmax = np.full(400, 1e12) if kind == "sun" else d * (1 - 2.0 ** -10)
    assert np.allclose(tmax[ok], want_tmax[ok], rtol=8 * EPS)
    # no sample is a row of zeros, and the cosine decides it where nothing else does
    assert not wd[~ok].any() and not L[~ok].any() and not tmax[~ok].any()
    cos64 = (wd64 * n).sum(1)
    assert (ok[(cos64 > 1e-6) & (f > 1e-9)]).all() and not ok[cos64 < -1e-6].any()


def test_spot_smoothstep_at_the_cone_edges():
    """hits placed at cos = co, cos = ci and halfway between (t = 0, 1, 1/2): the spot's sample over the point lamp's at the same place
    is f = 0, 1 and 1/2; inside the inner cone it is the point lamp's sample bit for bit, outside the outer cone there is none"""
    p, a = np.array([0.2, 1.5, -0.3]), np.array([0.0, -1.0, 0.0])
    spot = scene.spot_lamp(p, a, (4, 3, 2), 20, 45)
    point = scene.point_lamp(p, (4, 3, 2))
    ci, co = float(spot[10]), float(spot[11])
    out = {}
    for name, c in (("outside", co - 0.1), ("co", co), ("half", (ci + co) / 2), ("ci", ci), ("inside", ci + 0.02)):
        s = np.sqrt(1 - c * c)
        phi = np.linspace(0.1, 6.0, 16)
        x = (p + 1.7 * (c * a + s * np.stack([np.cos(phi), 0 * phi, np.sin(phi)], 1))).astype(F)
        n = np.tile(np.array([0, 1, 0], F), (16, 1))
        refl, ipdf = np.full((16, 3), 0.5, F), np.full(16, 3.0, F)
        so = lm.lamp_light(np.tile(spot, (16, 1)), x, n, refl, ipdf)
        po = lm.lamp_light(np.tile(point, (16, 1)), x, n, refl, ipdf)
        assert po[0].all()
        out[name] = (so, po)
    so, po = out["outside"]
    assert not so[0].any() and (so[4] == lm.FALLOFF).all()
    so, po = out["inside"]
    assert so[0].all() and all(np.array_equal(_bits(a_), _bits(b_)) for a_, b_ in zip(so[1:4], po[1:4]))
    so, po = out["ci"]
    assert so[0].all() and np.allclose(so[3] / po[3], 1.0, rtol=0, atol=1e-9)
    so, po = out["half"]
    assert so[0].all() and np.allclose(so[3] / po[3], 0.5, rtol=0, atol=1e-5)
    so, po = out["co"]
    assert (so[3] / po[3] <= 1e-9).all()


def test_every_early_out_is_reached():
    """one hit per early-out and kind: the lamp at the hit (dist2 = 0), behind the surface (cos_x <= 0), straight above (sxz = 0), and
    outside a spot's cone (f = 0); a NaN cosine is no sample either"""
    up = np.array([[0, 1, 0]], F)
    one3, ip = np.ones((1, 3), F), np.ones(1, F)
    x = np.array([[0.5, 0.25, -1]], F)
    assert lm.lamp_light(scene.point_lamp(x[0], 1), x, up, one3, ip)[4][0] == lm.DIST2
    assert lm.lamp_light(scene.point_lamp((0.5, -3, 2), 1), x, up, one3, ip)[4][0] == lm.COS_X
    assert lm.lamp_light(scene.point_lamp((0.5, 4, -1), 1), x, up, one3, ip)[4][0] == lm.SXZ
    assert lm.lamp_light(scene.spot_lamp((3, 1, -1), (1, 0, 0), 1), x, up, one3, ip)[4][0] == lm.FALLOFF
    assert lm.lamp_light(scene.sun_lamp((0.3, 1, 0), 1), x, up, one3, ip)[4][0] == lm.COS_X
    sun = scene.sun_lamp((1e-30, -1, 0), 1)                        # a.x survives the rule, its square underflows
    assert lm.check_row(sun)[0] == "ok" and lm.lamp_light(sun, x, up, one3, ip)[4][0] == lm.SXZ
    assert lm.lamp_light(scene.point_lamp((1, 2, 0), 1), x, np.full((1, 3), np.nan, F), one3, ip)[4][0] == lm.COS_X
    ok, wd, tmax, L, why = lm.lamp_light(scene.point_lamp((1, 2, 0), 1), x, up, one3, ip)
    assert ok[0] and why[0] == lm.SAMPLE and tmax[0] > 0 and (L[0] > 0).all()


# ---------------------------------------------------------------------------------------------------------------- helpers
def test_scene_helpers(tmp_path):
    p = scene.point_lamp((1, 2, 3), 2.0)
    assert p.dtype == F and p.tolist() == [0, 1, 2, 3, 2, 2, 2, 0, 0, 0, 0, 0]
    s = scene.spot_lamp((1, 2, 3), (0, -2, 0), (1, 2, 3), 30, 60)
    assert s[:10].tolist() == [1, 1, 2, 3, 1, 2, 3, 0, -1, 0] and s[10] == F(np.cos(np.radians(30.0))) and s[11] == F(np.cos(np.radians(60.0)))
    u = scene.sun_lamp((3, -4, 0), (5, 4, 3))
    assert np.allclose(u, [2, 0, 0, 0, 5, 4, 3, 0.6, -0.8, 0, 0, 0])
    tab = scene.lamp_table(p, s, u)
    assert tab.shape == (3, 12) and tab.dtype == F and lm.first_bad_row(tab) == (3, "ok", -1)
    assert scene.lamp_table().shape == (0, 12) and scene.lamp_table(tab, p).shape == (4, 12)
    for bad in (lambda: scene.spot_lamp((0, 0, 0), (0, 0, 0), 1), lambda: scene.spot_lamp((0, 0, 0), (0, 1, 0), 1, 40, 30),
                lambda: scene.sun_lamp((0, -1, 0), 1), lambda: scene.lamp_table(np.zeros((65537, 12), F)),
                lambda: scene.lamp_table(scene.point_lamp((0, 0, 0), -1.0))):
        with pytest.raises(ValueError):
            bad()
    path = str(tmp_path / "lamps.bin")
    scene.write_lamps(path, tab)
    raw = open(path, "rb").read()
    assert raw[:4] == b"SPLA" and struct.unpack("<I", raw[4:8])[0] == 3 and raw[8:] == tab.tobytes()
    t, m = scene.closed_room(30)
    ext = [float(t[:, k:9:3].max()) - float(t[:, k:9:3].min()) for k in range(3)]
    assert scene.scene_R2(t) == 0.25 * ((ext[0] * ext[0] + ext[1] * ext[1]) + ext[2] * ext[2])
    w = scene.lamp_weights(t, tab)
    assert w[0] == 4.0 * 6.0 and w[1] == (2.0 * (1.0 - float(s[11]))) * 6.0 and w[2] == scene.scene_R2(t) * 12.0
