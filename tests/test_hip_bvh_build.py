"""The device build of the opt-in linear BVH (spath_amd/csrc/sp_bvh_build.h), read back for the first time: scene box over ordered
uints, the "big" classification with its threshold ladder, Morton keys, the stable sort, leaf records and padded boxes, the big list,
the level-by-level refit.  The inclusive slab test of the walk hides a leaf box that misses a vertex or a parent that is not the union
of its children behind a handful of wrong rays; here every word is compared.

Without a GPU: the numpy model of the build (tests/bvh_model.py) satisfies, on every scene, the invariants that make a tree a correct
one (tests/bvh_checks.py, check_structure), which are stated without the model's arithmetic.
With one: the dump of the device structure (sphip_selftest_bvh_dump) satisfies them too and equals the model bit for bit.

The scenes are the smallest that reach each branch (bvh_checks.SCENES).  Non-finite vertices: sphip_set_scene accepts them and
test_hip_robustness.py holds every brute-force scan to the oracle on such a scene, so they are built, not refused: their coordinates
stay out of every box (a NaN one also out of its triangle's extent), and a triangle whose extent is not finite goes to the big list."""
import numpy as np
import pytest

import bvh_checks as bc
import bvh_model

NAMES = sorted(bc.SCENES)


@pytest.mark.parametrize("name", NAMES)
def test_model_builds_a_correct_tree(name):
    t = bc.scene_tris(name)
    b = bvh_model.build(t)
    bc.check_structure(t, b, bc.EXPECT_N_BIG.get(name))
    if name == "closed_room_4097":
        assert b["n_leaves"] == 2048
    if name == "big_257":
        assert b["meta"][6] == 257 and b["thr"] == np.float32(0.5) * b["max_ext"]
    if name == "big_none":
        assert b["meta"][7] > 256 and b["thr"] == np.inf
    if name == "point":
        assert b["max_ext"] == 0 and not b["keys"].any()
    if name == "plane":
        assert (bvh_model.scene_box(b["meta"])[1] == 0).sum() == 1
    if name.startswith("moved"):
        assert np.signbit(bvh_model.ord2f(bvh_model.f2ord(t[20, 1]))) and bvh_model.f2ord(np.float32(-0.0)) < bvh_model.f2ord(np.float32(0.0))


def test_ordered_uints_round_trip_and_order():
    f = np.array([-np.inf, -3e38, -1.0, -1e-45, -0.0, 0.0, 1e-45, 1.0, 3e38, np.inf], np.float32)
    o = bvh_model.f2ord(f)
    assert (np.diff(o.astype(np.int64)) > 0).all()
    assert np.array_equal(bvh_model.ord2f(o).view(np.uint32), f.view(np.uint32))


def test_model_mutations_are_caught_by_the_invariants():
    """the invariants are not a restatement of the model: a leaf box without its padding still passes them (it contains its vertices;
    only the bit comparison with the device can tell), a box that misses a vertex, a parent that is not the union, an unstable order
    and a lost triangle do not"""
    t = bc.scene_tris("closed_room_300")
    good = bvh_model.build(t)
    nl = good["n_leaves"]

    def broken(f):
        b = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in good.items()}
        f(b)
        with pytest.raises(AssertionError):
            bc.check_structure(t, b)

    broken(lambda b: b["nodes"].__setitem__((nl + 3, 0), b["nodes"][nl + 3, 0] + np.float32(0.05)))          # a leaf box that misses a vertex
    broken(lambda b: b["nodes"].__setitem__((nl // 2, 3), b["nodes"][nl // 2, 3] - np.float32(1e-3)))        # a parent below its children's union
    broken(lambda b: b["idx"].__setitem__([0, 1], b["idx"][[1, 0]]))                                        # order (and record) swapped
    broken(lambda b: b["idx"].__setitem__(5, b["idx"][6]))                                                  # a triangle twice, one lost
    broken(lambda b: b["rec"].__setitem__((4 * nl - 1, 2), np.float32(1.0)))                                # padding with a record


def _dump_equals_model(hip, t, name):
    d = hip.selftest_bvh_dump()
    b = bvh_model.build(t)
    assert d["n_leaves"] == b["n_leaves"], name
    assert np.array_equal(d["meta"][:11], b["meta"][:11]), (name, d["meta"][:11], b["meta"][:11])
    assert np.array_equal(d["idx"], b["idx"]), name
    assert bvh_model.same_bits(d["rec"], b["rec"]), name
    assert bvh_model.same_bits(d["nodes"][1:], b["nodes"][1:]), name
    bc.check_structure(t, d, bc.EXPECT_N_BIG.get(name))


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_device_build_equals_model(hip, name):
    t = bc.scene_tris(name)
    hip.set_scene(t, bc.mats_for(t))
    _dump_equals_model(hip, t, name)


@pytest.mark.gpu
def test_device_rebuild_after_a_smaller_scene(hip):
    """a large scene, then a small one on the same context: the buffers are reused (grow-only) and the structure is rebuilt"""
    for name in ("closed_room_4097", "n5", "open_clutter_1500", "identical", "closed_room_14"):
        t = bc.scene_tris(name)
        hip.set_scene(t, bc.mats_for(t))
        _dump_equals_model(hip, t, name)
