"""The numpy replay of the estimator (tests/path_model.py) pinned on the CPU: tests/golden/path_model_digests.json holds, for every
replay case of the seven estimator test modules at their own 48 x 32, 4 spp, seed 3, the SHA-256 of the mean and the image and the
scan count, and the same for samples 1..4 of one case per estimator and per feature.  The file was computed by the separate models
the replay was folded from, in two steps (its `parent` names the commits): the entries nee/, mis/, specular/ and smooth/ by the four
models of the first fold, the entries glass/, env/ and glossy/ by dielectric_model.render, env_model.render and glossy_model.render
of the second, which also pin the counters of `info`, what first_ns receives and the "accepts" list.  So an edit to the model that
changes any bit or any counter of any case fails here, without a GPU."""
import hashlib
import json
import os

import numpy as np

import env_model
import hip_checks as hc
import path_model
import test_hip_dielectric
import test_hip_glossy

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "path_model_digests.json")
S0 = ("nee/many_emitters", "mis/many_emitters", "specular/mixed_room/plain", "glass/smooth/mixed/mis", "env/glass/tables/n3/mis", "glossy/sky/mis")
LISTS = {"first_ns/smooth/mirror_sphere/mixed/mis", "accepts/smooth/mirror_sphere/mixed/mis", "accepts/glass/smooth/mixed/mis"}


def _cases():
    """-> {key: (t, m, est, dict of samples' keywords)}"""
    out = {}
    for name, make in hc.NEE_SCENES.items():
        for est in ("nee", "mis"):
            out[f"{est}/{name}"] = make() + (est, {})
    for name, make in hc.SPECULAR_SCENES.items():
        for est in hc.ESTIMATORS:
            out[f"specular/{name}/{est}"] = make()[:2] + (est, dict(spec=make()[2]))
    for name in hc.SMOOTH_SCENES:
        for mixed in (False, True):
            t, m, s, vn = hc.smooth_case(name, mixed)
            for est in hc.ESTIMATORS:
                out[f"smooth/{name}/{'mixed' if mixed else 'own'}/{est}"] = (t, m, est, dict(spec=s, vn=vn))
    for smooth in (False, True):
        for mixed in (False, True):
            t, m, s, vn, g = test_hip_dielectric.sphere_scene(smooth, mixed)
            for est in hc.ESTIMATORS:
                out[f"glass/{'smooth' if smooth else 'flat'}/{'mixed' if mixed else 'bare'}/{est}"] = (t, m, est, dict(spec=s, vn=vn, glass=g))
    for name in ("open", "glass"):
        for tables in (False, True):
            t, m, s, vn, g = env_model.replay_scene(name, tables, hc.mixed_table)
            for mp, env in env_model.replay_maps().items():
                for est in hc.ESTIMATORS:
                    out[f"env/{name}/{'tables' if tables else 'bare'}/{mp}/{est}"] = (t, m, est, dict(spec=s, vn=vn, glass=g, env=env))
    for name in test_hip_glossy.CASES:
        k = test_hip_glossy.case(name)
        for est in hc.ESTIMATORS:
            out[f"glossy/{name}/{est}"] = (k["t"], k["m"], est, dict(spec=k["s"], vn=k["vn"], glass=k["g"], env=k["env"], rough=k["rough"]))
    return out


def _digest(lists):
    h = hashlib.sha256()
    for item in lists:
        for a in item:
            h.update(np.ascontiguousarray(a).tobytes())
    return {"sha256": h.hexdigest(), "count": len(lists)}


def _same_info(info, want, key):
    """the counters the entry pins (the entries of the first fold pin none) have the values its model gave them"""
    assert {k: info[k] for k in want.get("info", {})} == want.get("info", {}), key


def test_digests():
    doc = json.load(open(GOLDEN))
    want = doc["cases"]
    w, h = doc["shape"]
    rays = hc.rays(w, h)
    cases = _cases()
    assert sorted(want) == sorted(list(cases) + ["s0=1/" + k for k in S0] + list(LISTS)) and len(cases) == 24 + 34
    lists = {}
    for key, (t, m, est, kw) in cases.items():
        fn = []
        rgba, mean, scans, info = path_model.render(rays, t, m, doc["spp"], doc["seed"], est, first_ns=fn, collect=("accepts",), **kw)
        assert scans == want[key]["scans"], key
        assert hashlib.sha256(mean.tobytes() + rgba.tobytes()).hexdigest() == want[key]["sha256"], key
        _same_info(info, want[key], key)
        lists["first_ns/" + key], lists["accepts/" + key] = _digest(fn), _digest(info["accepts"])
    for key in LISTS:
        assert lists[key] == want[key], key
    for case in S0:
        t, m, est, kw = cases[case]
        rec, scans, info = path_model.samples(rays, t, m, doc["seed"], 1, doc["spp"], est, **kw)
        assert scans == want["s0=1/" + case]["scans"], case
        assert hashlib.sha256(rec.tobytes()).hexdigest() == want["s0=1/" + case]["sha256"], case
        _same_info(info, want["s0=1/" + case], case)
