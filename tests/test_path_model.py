"""The numpy replay of the estimator (tests/path_model.py) pinned on the CPU: tests/golden/path_model_digests.json holds, for every
replay case of the four estimator test modules at their own 48 x 32, 4 spp, seed 3, the SHA-256 of the mean and the image and the
scan count, and the same for samples 1..4 of one case per estimator.  The file was computed by the four separate models the
replay was folded from (the commit it names), so an edit to the model that changes any bit of any case fails here, without a GPU."""
import hashlib
import json
import os

import hip_checks as hc
import path_model

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "path_model_digests.json")


def _cases():
    """-> {key: (t, m, est, spec, vn)}"""
    out = {}
    for name, make in hc.NEE_SCENES.items():
        for est in ("nee", "mis"):
            out[f"{est}/{name}"] = make() + (est, None, None)
    for name, make in hc.SPECULAR_SCENES.items():
        for est in hc.ESTIMATORS:
            out[f"specular/{name}/{est}"] = make()[:2] + (est, make()[2], None)
    for name in hc.SMOOTH_SCENES:
        for mixed in (False, True):
            t, m, s, vn = hc.smooth_case(name, mixed)
            for est in hc.ESTIMATORS:
                out[f"smooth/{name}/{'mixed' if mixed else 'own'}/{est}"] = (t, m, est, s, vn)
    return out


def test_digests():
    doc = json.load(open(GOLDEN))
    want = doc["cases"]
    w, h = doc["shape"]
    rays = hc.rays(w, h)
    cases = _cases()
    s0 = {"s0=1/nee/many_emitters": "nee/many_emitters", "s0=1/mis/many_emitters": "mis/many_emitters",
          "s0=1/specular/mixed_room/plain": "specular/mixed_room/plain"}
    assert sorted(want) == sorted(list(cases) + list(s0)) and len(cases) == 24
    for key, (t, m, est, spec, vn) in cases.items():
        rgba, mean, scans, _ = path_model.render(rays, t, m, doc["spp"], doc["seed"], est, spec, vn)
        assert scans == want[key]["scans"], key
        assert hashlib.sha256(mean.tobytes() + rgba.tobytes()).hexdigest() == want[key]["sha256"], key
    for key, case in s0.items():
        t, m, est, spec, vn = cases[case]
        rec, scans, _ = path_model.samples(rays, t, m, doc["seed"], 1, doc["spp"], est, spec, vn)
        assert scans == want[key]["scans"], key
        assert hashlib.sha256(rec.tobytes()).hexdigest() == want[key]["sha256"], key
