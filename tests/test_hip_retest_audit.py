"""Per-pair audit of the RE-TEST of stage 2 of the default scan ON THE DEVICE (sphip_selftest_retest).

Stage 2 re-tests the triangles of a listed group against the cylinder of a SECOND edge of the triangle, margin 2 Dq (DESIGN.md
section 4.3); what it lets through goes on to the exact test.  Through the closest hit a wrongly rejected pair shows only when it is
its ray's nearest hit.  Here the re-test alone runs -- the records of the tiles the render kernels read, the same function, the same
margin -- on EVERY (ray, triangle) pair of the stream, under both workgroup shapes (quads and octets), and the oracle's
geom::ray_intersect (reference src/geom.h:197-222) is evaluated on the same pairs: NO PAIR THE REFERENCE ACCEPTS (d > 0) MAY HAVE ITS
BIT CLEAR.  Padding places are the only pairs left out.  Scenes of 65, 257, 513 and 601 triangles: one past a wave, one past a tile,
one past the wide tile, ragged class ends; 2048 rays each from the generators of the stage-1 audit (aimed, in-plane, small-and-far).
The device's verdicts are also compared with the numpy replay of tests/retest_model.py.
"""
import os

import numpy as np
import pytest

from spath_amd import capi, scene

import retest_model as M
import test_hip_stage1_audit as A

pytestmark = pytest.mark.gpu
F = np.float32
_cache = {}


def cases():
    """(tag, triangles, 2048 rays), built once."""
    if "cases" not in _cache:
        rng = np.random.default_rng(20261022)
        out = []
        t = scene.closed_room(65)[0]
        out.append(("closed room 65", t, np.concatenate([A._aimed_rays(rng, t, 1280, [3.5, 1.8, 3.5]), A._in_plane_rays(rng, t, 768)])))
        t = scene.open_clutter(257)[0]
        out.append(("open clutter 257", t, np.concatenate([A._aimed_rays(rng, t, 1280, [2, 1, 2]), A._in_plane_rays(rng, t, 768)])))
        t = scene.closed_room(513)[0]
        out.append(("closed room 513", t, np.concatenate([A._aimed_rays(rng, t, 1280, [3.5, 1.8, 3.5]), A._in_plane_rays(rng, t, 768)])))
        t = A._small_far_scene(rng, 601)
        out.append(("small far 601", t, A._aimed_rays(rng, t, 2048, [3, 3, 3], unnormalised=0.7)))
        _cache["cases"] = out
    return _cache["cases"]


def accepted(O, k):
    """geom::ray_intersect's verdict on every (ray, triangle) pair of case k: bool [ray, triangle], computed once."""
    if ("acc", k) not in _cache:
        _, t, rays = cases()[k]
        n = t.shape[0]
        acc = np.zeros((rays.shape[0], n), dtype=bool)
        for r0 in range(0, rays.shape[0], 256):
            rr = rays[r0:r0 + 256]
            q = np.concatenate([np.repeat(rr, n, axis=0), np.tile(t[:, :9], (rr.shape[0], 1))], axis=1)
            with np.errstate(all="ignore"):
                acc[r0:r0 + 256] = O.device_math(4, q, q.shape[0]).reshape(rr.shape[0], n) > 0.0
        acc.setflags(write=False)
        _cache["acc", k] = acc
    return _cache["acc", k]


@pytest.fixture(params=[256, 512])
def shaped(request):
    old = os.environ.get("SPATH_HIP_CYLM_SHAPE")
    os.environ["SPATH_HIP_CYLM_SHAPE"] = str(request.param)
    ctx = capi.Context(0)
    yield ctx, request.param
    ctx.close()
    if old is None:
        del os.environ["SPATH_HIP_CYLM_SHAPE"]
    else:
        os.environ["SPATH_HIP_CYLM_SHAPE"] = old


def test_retest_never_rejects_a_pair_the_reference_accepts(shaped, O):
    hip, shape = shaped
    pairs = tot_acc = inplane_acc = rejected = 0
    for k, (tag, t, rays) in enumerate(cases()):
        n = t.shape[0]
        hip.set_scene(t, np.full((n, 6), 0.5, dtype=F))
        surv, order, T = hip.selftest_retest(rays)
        assert T == shape, (tag, T)
        valid = (order >= 0) & (order < n)                         # every place but the padding
        pos_of = np.full(n, -1, dtype=np.int64)
        pos_of[order[valid]] = np.flatnonzero(valid)
        big = pos_of < 0                                           # the big class: no filter, every ray runs the reference's test on it
        assert big.sum() <= 64 and np.array_equal(np.sort(order[valid]), np.flatnonzero(~big)), (tag, "every other triangle exactly once")
        s_t = surv[:, np.maximum(pos_of, 0)]                       # [ray, triangle index]
        s_t[:, big] = True
        acc = accepted(O, k)
        bad = acc & ~s_t
        print(f"{tag} ({shape}): {acc.size} pairs, {int(acc.sum())} accepted by geom::ray_intersect, {1.0 - s_t[:, ~big].mean():.4f} rejected by the re-test")
        assert not bad.any(), (tag, shape, "the re-test rejected an accepted pair", np.argwhere(bad)[:4], int(bad.sum()))
        # the device against the numpy replay of the same records and chain (the double arithmetic of the records may differ in the last
        # place between the two: verdicts within a hair of the margin are left out)
        Arec, R = M.records(t)
        ray = M.ray_state(rays, M.scene_bound(t))
        ri, ti = np.repeat(np.arange(rays.shape[0]), n), np.tile(np.arange(n), rays.shape[0])
        m_s, x = M.survives(R, ti, ray, ri, margins=2)
        with np.errstate(all="ignore"):
            near = np.abs(x - 2 * ray["Dq"][ri]) <= 1e-3 * np.abs(2 * ray["Dq"][ri])
        diff = (m_s.reshape(-1, n) != s_t) & ~near.reshape(-1, n) & ~big[None, :]
        assert diff.mean() < 1e-6, (tag, shape, int(diff.sum()))
        pairs += acc.size; tot_acc += int(acc.sum()); rejected += int((~s_t).sum())
        if k < 3:
            inplane_acc += int(acc[1280:].sum())
    assert pairs >= 2_500_000 and tot_acc >= 1000 and inplane_acc >= 100, (pairs, tot_acc, inplane_acc)
    assert rejected > pairs // 2                                   # and it does reject
