"""tests/history_model.py on the CPU: its transition rules against literals, the legality of every program, what the committed seeds
cover, and the text form.  No GPU is used; tests/test_hip_history.py runs the programs."""
import numpy as np
import pytest

import history_model as hm
from history_model import E_INVALID, E_STATE, Op
from spath_amd import capi

ALL = {"hand:" + k: v for k, v in hm.HAND.items()}
ALL.update({"seed:%d" % s: hm.program(s, hm.LENGTH) for s in hm.SEEDS})
SCENE = Op("set_scene", name="room200", form="host", stream=0)
BEGIN = Op("accum_begin", w=16, h=16, seed=3, flags=0, src="rays", rule=-1)


def full_state():
    ops = [SCENE] + hm._all_tables() + hm._context_items("bright8") + [Op("set_lens", lens="wide")]
    return hm.run_model(ops)[1]


def test_flag_values_are_the_bindings():
    for name, attr in (("REUSE", "FLAG_PRIMARY_REUSE"), ("ACCEL", "FLAG_ACCEL"), ("NEE", "FLAG_NEE"), ("MIS", "FLAG_MIS"), ("CAMS", "FLAG_CAMERA_SAMPLES"),
                       ("SPEC", "FLAG_SPECULAR"), ("SMOOTH", "FLAG_SMOOTH"), ("GLASS", "FLAG_DIELECTRIC"), ("ENV", "FLAG_ENVIRONMENT"),
                       ("GLOSSY", "FLAG_GLOSSY"), ("TEX", "FLAG_TEXTURE"), ("NMAP", "FLAG_NORMAL_MAP")):
        assert hm.FLAG_NAMES[name] == getattr(capi, attr)
    assert capi.flag_chunks(4) == 4 << hm.CHUNKS_SHIFT
    assert [hm.TABLE_SETTER[t] for t in hm.TABLES] == [t[0] for t in capi.TRI_TABLES]
    assert [hm.TABLE_FLOATS[t] for t in hm.TABLES] == [t[1] for t in capi.TRI_TABLES]


def test_pool_scenes_have_their_sizes_and_the_twin_differs():
    for name, n in hm.SCENE_TRIS.items():
        t, m = hm.scene_data(name)
        assert t.shape == (n, 12) and m.shape == (n, 6), name
    a, b = hm.scene_data("room200"), hm.scene_data("room200b")
    assert not np.array_equal(a[0], b[0]) and not np.array_equal(a[1][:, 3:6], b[1][:, 3:6])
    assert not hm.scene_data("dark200")[1][:, 3:6].any()
    assert sorted(w * h for w, h in hm.FRAMES) == [1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 1040, 1536, 2747]


# ---------------------------------------------------------------------------------------------------------------- transitions
def test_set_scene_clears_the_tables_and_keeps_the_context_items():
    s = full_state()
    assert s.key() == ("room200", ("spec", "vn", "glass", "rough", "uv"), "bright8", True, True, "wide")
    s = hm.apply(s, Op("set_scene", name="clutter100", form="device", stream=1))
    assert s.key() == ("clutter100", (), "bright8", True, True, "wide")


def test_a_refused_setter_leaves_its_table_and_the_accumulation():
    s = hm.apply(full_state(), BEGIN)
    for t in hm.TABLES:
        bad = Op("set_table", table=t, form="host", stream=0, bad=1, expect=E_INVALID)
        assert hm.expected_code(s, bad) == E_INVALID
        s2 = hm.apply(s, bad)
        assert s2.key() == s.key() and not s2.accum.ended
    s2 = hm.apply(s, Op("set_env", map="black8", form="host", stream=0, bad=1, expect=E_INVALID))
    assert s2.env == "bright8" and not s2.accum.ended
    empty = hm.State()
    early = Op("set_table", table="spec", form="host", stream=0, expect=E_STATE)
    assert hm.expected_code(empty, early) == E_STATE and hm.apply(empty, early).key() == empty.key()


@pytest.mark.parametrize("ender", [Op("set_scene", name="room200", form="host", stream=0), Op("set_table", table="rough", form="device", stream=1),
                                   Op("set_env", map="black8", form="host", stream=0), Op("set_atlas", form="host", stream=0),
                                   Op("set_nmap", form="host", stream=0)], ids=lambda op: op.kind)
def test_a_setter_or_a_set_scene_ends_an_open_accumulation(ender):
    s = hm.apply(hm.apply(full_state(), BEGIN), Op("accum_step", n=2))
    assert hm.expected_code(s, Op("accum_step", n=1)) == 0
    s = hm.apply(s, ender)
    assert s.accum.ended
    assert hm.expected_code(s, Op("accum_step", n=1)) == E_STATE
    assert hm.expected_code(s, Op("accum_denoise")) == E_STATE and hm.expected_code(s, Op("accum_gbuffer")) == E_STATE
    assert hm.expected_code(s, Op("accum_counts")) == 0
    assert hm.expected_code(hm.apply(s, BEGIN), Op("accum_step", n=1)) == 0


def test_renders_and_the_lens_do_not_end_an_accumulation():
    s = hm.apply(hm.apply(full_state(), BEGIN), Op("accum_step", n=2))
    for op in (Op("render", w=9, h=7, spp=2, seed=1, mode="pt", flags=hm.WIDEST), Op("render_camera", w=9, h=7, spp=2, seed=1, flags=hm.CAMS),
               Op("closest_hit_device", w=9, h=7, flags=0, skip=1, stream=0), Op("gbuffer_device", w=9, h=7, flags=0, stream=0),
               Op("set_lens", lens="pinhole")):
        s = hm.apply(s, op)
    assert not s.accum.ended and s.accum.steps() == [2] and s.accum.at.lens == "wide" and s.lens == "pinhole"
    assert hm.expected_code(hm.State(), Op("accum_step", n=1)) == E_STATE and hm.expected_code(hm.State(), Op("accum_counts")) == E_STATE


def test_flag_rules_against_literals():
    s, bare = full_state(), hm.run_model([SCENE])[1]
    ok = lambda st, f, **k: hm.check_flags(st, f, **k)
    assert ok(s, hm.WIDEST) == 0 and ok(s, hm.WIDEST | 16) == 0 and ok(s, hm.WIDEST | hm.ACCEL) == 0
    assert ok(s, hm.MIS) == E_INVALID and ok(s, hm.NEE | hm.SPEC) == E_INVALID and ok(s, hm.NEE) == 0
    assert ok(s, hm.SPEC | 15) == 0 and ok(s, hm.SPEC | 2) == 0 and ok(s, hm.SMOOTH | 15) == E_INVALID and ok(s, hm.TEX | 2) == E_INVALID
    assert ok(s, hm.GLOSSY) == E_INVALID and ok(s, hm.SPEC | hm.GLOSSY) == 0
    assert ok(s, hm.SPEC, pt=False) == E_INVALID and ok(s, hm.MIS, pt=False) == 0
    assert ok(s, hm.CAMS) == E_INVALID and ok(s, hm.CAMS, have_cam=True) == 0 and ok(s, hm.CAMS | hm.REUSE, have_cam=True) == E_INVALID
    assert ok(s, 3) == E_INVALID                                    # a retired variant
    for f in (hm.SPEC, hm.SMOOTH, hm.GLASS, hm.SPEC | hm.GLOSSY, hm.TEX, hm.NMAP, hm.ENV):
        assert ok(bare, f) == E_STATE, hex(f)
    assert ok(bare, hm.SMOOTH | 15) == E_INVALID                    # the variant is asked before the table


# ---------------------------------------------------------------------------------------------------------------- programs
@pytest.mark.parametrize("name", sorted(ALL))
def test_programs_are_legal_and_every_refusal_is_marked(name):
    prog = ALL[name]
    states, _ = hm.run_model(prog)
    for i, (s, op) in enumerate(zip(states, prog)):
        assert op.expect == hm.expected_code(s, op), (i, op)
        assert op.expect in (0, E_INVALID, E_STATE)


@pytest.mark.parametrize("name", sorted(ALL))
def test_text_form_round_trips(name):
    prog = ALL[name]
    again = hm.parse(hm.text(prog))
    assert again == prog and hm.text(again) == hm.text(prog)
    assert [op.a for op in again] == [op.a for op in prog]


def test_generated_programs_begin_with_the_warm_up_and_are_reproducible():
    w = hm.warm_up()
    assert w[len(hm.TABLES) + 5].a == {"w": 67, "h": 41, "spp": 16, "seed": 2, "mode": "pt", "flags": hm.WIDEST}
    assert [op.kind for op in w[-5:]] == ["accum_begin", "accum_step", "accum_step", "accum_step", "accum_denoise"]
    for s in hm.SEEDS:
        p = hm.program(s, hm.LENGTH)
        assert p[:len(w)] == w and len(p) == hm.LENGTH and p == hm.program(s, hm.LENGTH)
        assert sum(op.a.get("spp") == 16 for op in p[len(w):]) <= 1


def test_hand_programs_hold_a_model_anchor_and_the_stated_orders():
    for name, prog in hm.HAND.items():
        assert sum(op.model for op in prog) == 1 and all(op.kind == "render" and (op.w, op.h, op.spp) == hm.ANCHOR for op in prog if op.model), name
    p = hm.HAND["order_of_5_17[widest]"]
    kinds = [op.kind for op in p if op.kind.startswith(("accum", "render_camera"))]
    assert kinds == ["accum_begin", "accum_step", "accum_step", "accum_step", "render_camera", "accum_step", "accum_counts", "render_camera",
                     "accum_begin", "accum_step", "accum_step"]
    assert [(op.w, op.h) for op in p if op.kind in ("accum_begin", "render_camera")] == [(48, 32), (40, 26), (40, 26), (40, 26)]
    assert [op.n for op in p if op.kind == "accum_step"][:4] == [4, 4, 8, 4]
    p = hm.HAND["large_small_large[mis]"]
    assert [(op.w * op.h, op.spp) for op in p[9:13]] == [(2747, 16), (1, 1), (63, 3), (2747, 2)]


def test_the_seeds_cover_the_vocabulary():
    progs = [ALL["seed:%d" % s] for s in hm.SEEDS]
    ops = [op for p in progs for op in p]
    assert {op.kind for op in ops} == set(hm.FIELDS)
    flags = [op.flags for op in ops if "flags" in op.a and not op.expect]
    for name, bit in hm.FLAG_NAMES.items():
        assert any(f & bit for f in flags), name
    pt = [op.flags for op in ops if not op.expect and (op.kind in ("render_camera", "render_device_accum", "accum_begin") or op.a.get("mode") == "pt")]
    assert any(f & hm.NEE and not f & hm.MIS for f in pt) and any(f & hm.MIS for f in pt) and any(not f & hm.NEE for f in pt)
    for v in hm.VARIANTS:
        assert any(f & hm.VARIANT_MASK == v for f in pt), v
    assert {(f & hm.CHUNKS_MASK) >> hm.CHUNKS_SHIFT for f in pt} >= {0, 1, 4}
    assert {(op.w, op.h) for op in ops if "w" in op.a} == set(hm.FRAMES)
    assert {op.name for op in ops if op.kind == "set_scene"} == set(hm.SCENE_TRIS)
    assert {op.form for op in ops if op.kind == "set_scene"} == {"host", "device"}
    assert {(op.table, op.form) for op in ops if op.kind == "set_table" and not op.bad} == {(t, f) for t in hm.TABLES for f in ("host", "device")}
    assert {op.map for op in ops if op.kind == "set_env"} == set(hm.ENV_MAPS)
    assert {op.expect for op in ops} == {0, E_INVALID, E_STATE}
    assert {op.mode for op in ops if op.kind in ("render", "render_device")} == {"pt", "flat"}
    assert {op.skip for op in ops if op.kind == "closest_hit_device"} == {0, 1} and {op.src for op in ops if op.kind == "accum_begin"} == {"rays", "cam"}
    assert {op.rule for op in ops if op.kind == "accum_begin"} == {-1, 0, 1}
    assert any(op.kind == "accum_step" and op.expect == E_STATE for op in ops)
    assert any(op.kind == "render_camera" and op.flags & hm.CAMS for op in ops) and any(op.kind == "render_camera" and not op.flags & hm.CAMS for op in ops)


def test_references_outside_the_library_are_met():
    """a fresh context is code under test: the oracle and the numpy model must be asked often, not merely be available"""
    count = {"oracle_render": 0, "oracle_hits": 0, "oracle_total": 0, "model": 0}
    for name, prog in ALL.items():
        states, _ = hm.run_model(prog)
        met = [n for s, op in zip(states, prog) for n in hm.anchored_by(s, op)]
        for n in met:
            count[n] += 1
        if name.startswith("hand:"):
            assert met.count("model") == 1, name
    print("queries held to a reference outside the library:", count)
    assert count["oracle_render"] >= 10 and count["oracle_hits"] >= 10 and count["oracle_total"] >= 3 and count["model"] == len(hm.HAND)


def test_the_seeds_reuse_buffers_and_change_packs_and_scenes():
    total = {"reuses": 0, "pack_changes": 0, "grow": 0, "shrink": 0}
    for s in hm.SEEDS:
        c = hm.coverage(ALL["seed:%d" % s])
        for k in total:
            total[k] += int(c[k])
    print("coverage over the seeds", hm.SEEDS, total)
    for k, v in total.items():
        assert v >= 3, (k, v)


def test_work_need_against_hand_derived_plans():
    s = hm.run_model([SCENE])[1]
    r = lambda w, h, spp, f: hm.work_need(s, Op("render", w=w, h=h, spp=spp, seed=1, mode="pt", flags=f))
    # 1 x 1, 1 spp: one block of 1024 padded paths, one chunk (n_iter = 1); plain slot 52 B, MIS 112 B
    assert r(1, 1, 1, 16) == (1024 * 52, 52) and r(1, 1, 1, 16 | hm.NEE_MIS) == (1024 * 112, 112) and r(1, 1, 1, 16 | hm.NEE) == (1024 * 100, 100)
    # 67 x 41 = 2747 rays -> 3072 lanes; 16 spp: chunks double to min(128, 16) = 16
    assert r(67, 41, 16, 16) == (3072 * 16 * 52, 52) and r(67, 41, 16, 16 | hm.flag_chunks(4)) == (3072 * 4 * 52, 52)
    # variant 15: four samples of a pixel per lane -> 4 x the lanes, n_iter = 16 / 4
    assert r(67, 41, 16, 15) == (3072 * 4 * 4 * 52, 52)
    assert r(67, 41, 16, 1) == (0, 0) and r(67, 41, 16, hm.ACCEL) == (0, 0)
