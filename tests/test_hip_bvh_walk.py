"""The walk of the opt-in linear BVH (spath_amd/csrc/sp_bvh.h, scan_bvh) called directly (sphip_selftest_bvh_walk), in its closest
form and in its shadow form (tmax, any_hit), and held to the C oracle ray by ray -- not to a share of the rays.  bvh_checks.check_walk:
(index, distance bits) equal the oracle's, or the walk's answer is itself an accept of the strict float test and EVERY accept the
reference would have preferred is a rounding-noise accept by the float64 rule (bvh_model.noise_accept), the one difference the
contract in sp_bvh.h allows; no walk may be ended by its step bound; and the rays that carry a noise accept at all stay below 0.5 %,
so that the first clause is what is tested.

Ray families: random rays plus a camera viewport; directions with one and two zero components; origins exactly on a leaf-box face and
on a leaf-box vertex; rays grazing a triangle's plane at 1e-4 .. 3e-2 rad, where the float distance of a true hit is off by up to 4e-3
relative, hundreds of times the 1e-5 slack of the walk's cull and of the leaf padding; shadow rays from hit points towards the
emitters with tmax at 0.5, 1 - 2^-20 and 1 times the distance.  Each with no source triangle and with a random one.

And the walk's step and leaf counts equal a numpy model of the walk (bvh_model.walk) over the model's tree, so a walk that visits
more than it has to, or less, is seen even where its answer is right."""
import numpy as np
import pytest

import bvh_checks as bc
import bvh_model
from bvh_model import F

pytestmark = pytest.mark.gpu

_cache = {}


def _family(O, name, family, make):
    """(rays, pair values): oracle only, computed once per scene and family"""
    key = (name, family)
    if key not in _cache:
        rays = np.ascontiguousarray(make(), F)
        P = bc.pair_values(O, rays, bc.scene_tris(name))
        rays.setflags(write=False); P.setflags(write=False)
        _cache[key] = (rays, P)
    return _cache[key]


def _set(hip, name):
    t = bc.scene_tris(name)
    hip.set_scene(t, bc.mats_for(t))
    return t, bvh_model.n_leaves_for(t.shape[0])


def _with_and_without_src(hip, O, name, family, rays, P):
    t, nl = _set(hip, name)
    rng = np.random.default_rng(len(name) + rays.shape[0])
    for src in (None, rng.integers(-1, t.shape[0], rays.shape[0]).astype(np.int32)):
        walked = hip.selftest_bvh_walk(rays, src)
        bc.check_walk(O, t, rays, walked, nl, src=src, P=P, tag=f"{name} {family} src={'none' if src is None else 'random'}")


@pytest.mark.parametrize("name", ["closed_room_14", "closed_room_300", "open_clutter_7", "open_clutter_1500", "dups", "n1", "n5", "identical"])
def test_walk_random_and_camera_rays(hip, O, name):
    rays, P = _family(O, name, "mixed", lambda: bc.mixed_rays(11))
    _with_and_without_src(hip, O, name, "mixed", rays, P)
    if name == "dups":                                     # three copies of every triangle: ties in distance go to the lowest index
        wi = hip.selftest_bvh_walk(rays)[0]
        assert (wi >= 0).mean() > 0.3 and (wi[wi >= 0] < 7).all()


@pytest.mark.parametrize("zeros", [1, 2])
@pytest.mark.parametrize("name", ["closed_room_300", "open_clutter_1500"])
def test_walk_axis_parallel_rays(hip, O, name, zeros):
    rays, P = _family(O, name, f"axis{zeros}", lambda: bc.axis_rays(20 + zeros, 1024, zeros))
    assert ((rays[:, 3:] == 0).sum(axis=1) == zeros).all()
    _with_and_without_src(hip, O, name, f"axis{zeros}", rays, P)


@pytest.mark.parametrize("name", ["closed_room_300", "open_clutter_1500"])
def test_walk_origins_on_box_faces_and_vertices(hip, O, name):
    rays, P = _family(O, name, "onbox", lambda: bc.box_origin_rays(30, bc.scene_tris(name), 1024))
    _with_and_without_src(hip, O, name, "onbox", rays, P)


@pytest.mark.parametrize("name", ["closed_room_300", "open_clutter_1500"])
def test_walk_grazing_rays(hip, O, name):
    rays, P = _family(O, name, "grazing", lambda: bc.grazing_rays(40, bc.scene_tris(name)))
    _with_and_without_src(hip, O, name, "grazing", rays, P)


@pytest.mark.parametrize("name,emitters", [("closed_room_300", (12, 13)), ("open_clutter_1500", (3, 4))])
def test_walk_shadow_form(hip, O, name, emitters):
    t, nl = _set(hip, name)
    key = (name, "shadow")
    if key not in _cache:
        prim = bc.mixed_rays(50)
        oi, od = O.closest_hits(prim, t)
        rays, src, dist = bc.shadow_rays(51, t, emitters, prim, oi, od)
        _cache[key] = (rays, src, dist, bc.pair_values(O, rays, t))
    rays, src, dist, P = _cache[key]
    assert rays.shape[0] > 1000
    blocked = 0
    for factor in (0.5, 1.0 - 2.0 ** -20, 1.0):
        tmax = (dist * factor).astype(F)
        for any_hit in (True, False):
            wi, wd, steps, leaves = walked = hip.selftest_bvh_walk(rays, src, tmax, any_hit)
            bc.check_walk(O, t, rays, walked, nl, src=src, tmax=tmax, any_hit=any_hit, P=P, tag=f"{name} shadow x{factor:.7f} any_hit={any_hit}")
            blocked += int((wi >= 0).sum())
            if any_hit:                                    # the shadow form stops at its first hit: never more work than the bounded closest form
                _, _, s2, l2 = hip.selftest_bvh_walk(rays, src, tmax, False)
                assert (steps <= s2).all() and (leaves <= l2).all()
    assert blocked > 0


@pytest.mark.parametrize("name", ["closed_room_300", "open_clutter_7", "big_257"])
def test_walk_counts_equal_model(hip, O, name):
    """index, distance, steps and leaves of 192 rays equal the numpy walk over the model's tree (the strict test's values from the
    oracle), in the closest form with a source triangle and in the shadow form"""
    t, nl = _set(hip, name)
    b = bvh_model.build(t)
    rays = np.concatenate([bc.mixed_rays(60, 96, 8, 4), bc.grazing_rays(61, t, 64)])
    P = bc.pair_values(O, rays, t)
    rng = np.random.default_rng(62)
    src = rng.integers(-1, t.shape[0], rays.shape[0]).astype(np.int32)
    tmax = rng.uniform(0.3, 6.0, rays.shape[0]).astype(F)
    for s, tm, any_hit in ((src, None, False), (src, tmax, True), (None, tmax, False)):
        got = hip.selftest_bvh_walk(rays, s, tm, any_hit)
        for k in range(rays.shape[0]):
            want = bvh_model.walk(b, lambda j: P[k, b["idx"][j]], rays[k], -1 if s is None else int(s[k]), None if tm is None else tm[k], any_hit)
            have = (int(got[0][k]), got[1][k], int(got[2][k]), int(got[3][k]))
            assert have[0] == want[0] and F(have[1]).view(np.uint32) == F(want[1]).view(np.uint32) and have[2:] == want[2:], (name, k, any_hit, have, want)
