"""CPU-side check of the RE-TEST of stage 2 of the default scan ("the re-test's cylinder"), independent of the GPU.

Stage 2 re-tests the triangles of a listed group against the cylinder around a SECOND barycentric slab of the triangle (cyl_retest_record:
the second-longest edge's, or the third's where the second's direction has too small a component along the class axis), in the frame
of the triangle's class, with the margin doubled: 2 Dq.  tests/retest_model.py replays the record (double, rounded once), the f32 ray
state and five-term chain and the sign decision; here that replay runs on adversarial pairs -- aimed rays, rays in the planes of
triangles (the reference's noise accepts), millimetre triangles from metres away, slivers and degenerate triangles, scenes scaled by
1e-4 ... 1e20 -- against the oracle's geom::ray_intersect (geom.h:197-222):

  1. no pair the reference accepts is rejected;
  2. every regular record has |w_a| >= 1 / (2 sqrt(3)) (1 - 2^-20): the scale the doubled margin is sized for;
  3. wherever the re-test rejects, that slab's own quantity |gm| - |t| (unit w, double) exceeds the 88u |dir|(|pos|+|v0|+|v1|+|v2|) the
     proof of section 4.1 needs -- the smallest value met is reported, as tests/test_filter_margin_model.py does for stage 1's cylinder.
"""
import numpy as np
import pytest

from spath_amd import scene

import retest_model as M
import test_hip_stage1_audit as A

F = np.float32


def _slivers_and_degenerates(rng, n):
    """Triangles with a third vertex (nearly) on the line of the other two, repeated vertices, points; sizes 1 mm ... 3 m."""
    scale = 10.0 ** rng.uniform(-3, 0.5, (n, 1))
    ctr = rng.uniform(-2, 2, (n, 3))
    v0, v1 = ctr + rng.normal(size=(n, 3)) * scale, ctr + rng.normal(size=(n, 3)) * scale
    s = rng.uniform(-0.5, 1.5, (n, 1))
    off = rng.normal(size=(n, 3)) * scale * 10.0 ** rng.uniform(-7, -2, (n, 1))
    kind = rng.integers(0, 8, n)
    off[kind == 0] = 0.0                                          # exactly collinear (to rounding)
    v2 = v0 + (v1 - v0) * s + off
    v1[kind == 1] = v0[kind == 1]                                 # a repeated vertex
    v2[kind == 2] = v1[kind == 2]
    v1[kind == 3] = v0[kind == 3]; v2[kind == 3] = v0[kind == 3]  # a point
    t = np.zeros((n, 12), dtype=F)
    t[:, 0:3], t[:, 3:6], t[:, 6:9] = v0, v1, v2
    return t


def _cases():
    rng = np.random.default_rng(20261021)
    out = []
    t = scene.closed_room(400)[0]
    out.append(("closed room, aimed", t, A._aimed_rays(rng, t, 768, [3.5, 1.8, 3.5])))
    out.append(("closed room, in-plane", t, A._in_plane_rays(rng, t, 768)))
    t = scene.closed_room(300, clutter_scale=10.0)[0]
    out.append(("large triangles, aimed + in-plane", t, np.concatenate([A._aimed_rays(rng, t, 512, [3.5, 1.8, 3.5]), A._in_plane_rays(rng, t, 256)])))
    t = scene.open_clutter(300)[0]
    out.append(("open clutter, aimed + in-plane", t, np.concatenate([A._aimed_rays(rng, t, 512, [2, 1, 2]), A._in_plane_rays(rng, t, 256)])))
    for it in range(4):
        t = A._small_far_scene(rng, (40, 150, 300, 12)[it])
        out.append((f"small far #{it}", t, A._aimed_rays(rng, t, 1024, [3, 3, 3], unnormalised=0.7)))
    for it in range(3):
        t = _slivers_and_degenerates(rng, 300)
        out.append((f"slivers and degenerates #{it}", t, np.concatenate([A._aimed_rays(rng, t, 768, [3, 3, 3]), A._in_plane_rays(rng, t, 512)])))
    base = scene.closed_room(300)[0]
    for s in (1e-4, 1e-2, 1e3, 1e8, 1e20):
        t = base.copy(); t[:, :9] *= F(s)
        out.append((f"scale {s:g}", t, np.concatenate([A._aimed_rays(rng, t, 384, np.array([3.5, 1.8, 3.5]) * s), A._in_plane_rays(rng, t, 128)])))
    t = base.copy()
    r = A._aimed_rays(rng, t, 384, [3.5, 1.8, 3.5]); r[:, 3:] *= F(1e-12)
    out.append(("directions x 1e-12", t, r))
    return out


def _audit(O, t, rays):
    """Every (ray, triangle) pair of a case: (accepted by the reference [r, n], survives the re-test [r, n], x, slab slack in u [r, n])."""
    n, nr = t.shape[0], rays.shape[0]
    Arec, R = M.records(t)
    ray = M.ray_state(rays, M.scene_bound(t))
    ri, ti = np.repeat(np.arange(nr), n), np.tile(np.arange(n), nr)
    surv, x = M.survives(R, ti, ray, ri, margins=2)
    q = np.concatenate([rays[ri], t[ti, :9]], axis=1)
    with np.errstate(all="ignore"):
        d = O.device_math(4, q, q.shape[0])
    acc = d > 0.0
    # the slab quantity |gm| - |t| of the re-test's slab: unit w, in double
    E = M.Edges(t)
    j = R["edge"]
    with np.errstate(all="ignore"):
        w = E.e[np.arange(n), j]; w = w / np.linalg.norm(w, axis=1, keepdims=True)
        mid, half = np.cross(w, 0.5 * (E.p0(j) + E.p1(j))), np.cross(w, 0.5 * (E.p1(j) - E.p0(j)))
        o, dd = rays[:, :3].astype(np.float64), rays[:, 3:].astype(np.float64)
        P = np.cross(o, dd)
        gm = P @ w.T - dd @ mid.T
        tt = dd @ half.T
        mag = np.linalg.norm(dd, axis=1)[:, None] * (np.linalg.norm(o, axis=1)[:, None] + np.linalg.norm(E.v, axis=2).sum(axis=1)[None, :])
        slack = (np.abs(gm) - np.abs(tt)) / (M.U * mag)
    return acc.reshape(nr, n), surv.reshape(nr, n), R, slack


def test_records_keep_the_scale_the_doubled_margin_is_sized_for():
    """Every regular record has |w_a| >= 1 / (2 sqrt(3)) (1 - 2^-20), read back from the ROUNDED record: 1 / w_a^2 = 1 + beta^2 + gamma^2."""
    rng = np.random.default_rng(5)
    seen = fallback = third = 0
    for tag, t, _ in _cases():
        for tt in (t, t[:, [3, 4, 5, 6, 7, 8, 0, 1, 2, 9, 10, 11]], t[:, [6, 7, 8, 0, 1, 2, 3, 4, 5, 9, 10, 11]]):     # every edge numbering
            Arec, R = M.records(tt)
            reg = R["ok"]
            wa = 1.0 / np.sqrt(1.0 + R["beta"].astype(np.float64) ** 2 + R["gamma"].astype(np.float64) ** 2)
            assert (wa[reg] >= M.WA_MIN * (1.0 - 2.0 ** -20)).all(), (tag, wa[reg].min())
            assert np.isinf(R["H"][~reg]).all() and (R["H"][~reg] > 0).all()
            assert np.isfinite(R["H"][reg]).all() and (R["H"][reg] >= 0).all()
            # a regular triangle (regular longest-edge record) practically always gets a regular re-test record
            seen += int(Arec["ok"].sum()); fallback += int((Arec["ok"] & ~reg).sum())
            E = M.Edges(tt)
            assert (R["edge"] != E.longest()).all()
            ls = np.sort(E.l, axis=1)
            third += int((reg & (E.l[np.arange(E.n), R["edge"]] == ls[:, 0]) & (ls[:, 0] < ls[:, 1])).sum())
    # at the bound itself: an equilateral triangle with one edge along (1, 1, 1) and the other two sharing its x component evenly
    k = np.sqrt(9.0 / 8.0)
    t = np.zeros((3, 12), dtype=F)
    for i in range(3):
        v = np.roll(np.array([[0, 0, 0], [1, 1, 1], [0.5, 0.5 + k, 0.5 - k]]), i, axis=0)
        t[i, :9] = v.reshape(9)
    Arec, R = M.records(t)
    assert R["ok"].all() and (np.abs(R["wa"]) >= 0.28).all()
    print(f"{seen} regular triangles, {fallback} of them with the always-surviving re-test record, {third} re-tested by their shortest edge")
    assert fallback <= seen // 100 and third > 0


def test_retest_never_rejects_a_pair_the_reference_accepts(O):
    tot = tot_acc = tot_rej = inplane_acc = 0
    worst = np.inf
    for tag, t, rays in _cases():
        acc, surv, R, slack = _audit(O, t, rays)
        bad = acc & ~surv
        assert not bad.any(), (tag, "the re-test rejected an accepted pair", np.argwhere(bad)[:4], int(bad.sum()))
        rej = ~surv
        tot += acc.size; tot_acc += int(acc.sum()); tot_rej += int(rej.sum())
        if "in-plane" in tag and "aimed" not in tag:
            inplane_acc += int(acc.sum())
        if rej.any():
            with np.errstate(all="ignore"):
                s = np.nanmin(np.where(rej, slack, np.inf))
            worst = min(worst, s)
            print(f"{tag}: {acc.size} pairs, {int(acc.sum())} accepted, {rej.mean():.3f} rejected, smallest slab slack among the rejections {s:.0f} u")
            assert s > 2 * 44.0, (tag, s)                          # needed by section 4.1 (iii) for any of the three slabs: 88u
    print(f"re-test's cylinder: {tot} pairs, {tot_acc} accepted by geom::ray_intersect, {tot_rej / tot:.3f} rejected; "
          f"smallest slab slack among its rejections {worst:.0f} u (needed 88 u)")
    assert tot >= 2_000_000 and tot_acc >= 5000 and inplane_acc >= 100, (tot, tot_acc, inplane_acc)
    assert tot_rej > tot // 2                                      # and it does reject


def test_model_of_the_longest_edge_record_agrees_with_the_margin_model():
    """retest_model's cyl_record is tests/test_filter_margin_model.py's (the same coefficients, bit for bit)."""
    import test_filter_margin_model as FM
    rng = np.random.default_rng(9)
    t = np.zeros((2000, 12), dtype=F); t[:, :9] = rng.normal(size=(2000, 9))
    E = M.Edges(t)
    jl = E.longest()
    Arec, _ = M.records(t)
    a, b, c, beta, gamma, mc, H = FM.cyl_records(E.e[np.arange(2000), jl], E.p0(jl).astype(F), E.p1(jl).astype(F))
    assert np.array_equal(a, Arec["a"]) and np.array_equal(beta, Arec["beta"]) and np.array_equal(gamma, Arec["gamma"])
    assert np.array_equal(mc, Arec["mc"]) and np.array_equal(H, Arec["H"])
