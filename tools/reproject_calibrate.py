"""The calibration of sphip_reproject_defaults and the bound of tests/test_hip_reproject.py's quality check, on the CPU with the numpy
statements (tests/reproject_model.py, tests/path_model.py: the kernels are held to them bit for bit).  No GPU is needed.

table:   scene.closed_room(300) and scene.open_clutter(100) at 64x48 over the camera pairs of the tests (reproject_model.PAIRS), every
         previous pixel with a history: for each (normal_min, plane_tol) the share of camera-hit pixels that keep a history and the share
         of counted taps whose hit triangle differs from the pixel's.  The defaults are the loosest pair at which the latter share is no
         larger than at the strictest pair tried.
ratios:  the quality check's frame (closed_room(300), NEE|MIS, 32x32, the pair "pan", 16 spp of history, 4 new samples, seeds 1..8
         with the new view drawn under seed + 1000, against REF_SPP samples of seed 987654321): per seed, the mean squared error of the
         blend over that of the 4 new samples alone, over the pixels with history; and the same for other caps of the history.
python tools/reproject_calibrate.py [table] [ratios] [REF_SPP]     (both parts when neither is named)"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import path_model as PM
import reproject_model as M
from spath_amd import scene

F = np.float32
args = sys.argv[1:]
ref_spp = next((int(a) for a in args if a.isdigit()), 4096)
parts = [a for a in args if a in ("table", "ratios")] or ["table", "ratios"]
NORMALS = (0.999, 0.99, 0.95, 0.9, 0.7, 0.5, 0.0)               # strictest first
PLANES = (0.001, 0.005, 0.01, 0.02, 0.05, 0.1)

if "table" in parts:
    w, h = 64, 48
    views = []
    for make in (lambda: scene.closed_room(300), lambda: scene.open_clutter(100)):
        t, m = make()
        for name in M.PAIRS:
            prev, cur = M.camera_pair(name, w, h)
            rp, rc = (np.ascontiguousarray(c.get_viewport(), F) for c in (prev, cur))
            (gp, ip), (gc, ic) = M.gbuffer(rp, t, m), M.gbuffer(rc, t, m)
            views.append((prev, rp, gp, ip, rc, gc, ic))
    ones, zeros = np.ones(w * h, F), np.zeros((w * h, 3), F)
    rows = {}
    for nm in NORMALS:
        for pt in PLANES:
            hits = kept = taps = other = 0
            for prev, rp, gp, ip, rc, gc, ic in views:
                _, _, code, tap, tapq, _ = M.reproject((1e9, nm, pt), prev, w, h, rc, gc, rp, gp, zeros, ones)
                hits += int((gc["mat"] >= 0).sum())
                kept += int((code == M.TAKEN).sum())
                cnt = tap == M.COUNTED
                taps += int(cnt.sum())
                other += int((ip[np.where(cnt, tapq, 0)] != ic[:, None])[cnt].sum())
            rows[nm, pt] = (kept / hits, other / taps)
    print(f"closed_room(300) + open_clutter(100), {w}x{h}, pairs {', '.join(M.PAIRS)}")
    print("share of camera-hit pixels that keep a history / share of counted taps on another triangle than the pixel's")
    print("normal_min \\ plane_tol " + " ".join(f"{pt:>15g}" for pt in PLANES))
    for nm in NORMALS:
        print(f"{nm:>22g} " + " ".join(f"{rows[nm, pt][0]:7.4f}/{rows[nm, pt][1]:7.4f}" for pt in PLANES))
    strict = rows[NORMALS[0], PLANES[0]][1]
    fit = [(nm, pt) for nm in NORMALS for pt in PLANES if rows[nm, pt][1] <= strict]
    print(f"strictest pair: other-triangle share {strict:.4f}; pairs no worse: {fit}")

if "ratios" in parts:
    w = h = 32
    t, m = scene.closed_room(300)
    prev, cur = M.camera_pair("pan", w, h)
    rp, rc = (np.ascontiguousarray(c.get_viewport(), F) for c in (prev, cur))
    gp, gc = M.gbuffer(rp, t, m)[0], M.gbuffer(rc, t, m)[0]

    def total(rays, n, seed):
        rec = PM.samples(rays, t, m, seed, 0, n, "mis")[0]
        acc = np.zeros((rec.shape[0], 3), F)
        for s in range(n):
            acc = acc + rec[:, s]
        return acc
    ref = np.zeros((w * h, 3), np.float64)
    for k in range(0, ref_spp, 256):                             # in blocks: the model keeps every sample of a call
        ref += PM.samples(rc, t, m, 987654321, k, min(256, ref_spp - k), "mis")[0].astype(np.float64).sum(1)
    ref /= ref_spp
    lib_defaults = tuple(float(x) for x in (os.environ.get("REPROJECT_PARAMS") or "32,0.5,0.1").split(","))
    print(f"closed_room(300) NEE|MIS {w}x{h}, pair pan, 16 + 4 spp, reference {ref_spp} spp; parameters {lib_defaults}")
    for cap in (lib_defaults[0], 4.0, 8.0, 16.0):
        out = []
        for seed in range(1, 9):
            mean16 = (total(rp, 16, seed) * F(1.0 / 16)).astype(F)
            hm, hh, code, *_ = M.reproject((cap,) + lib_defaults[1:], prev, w, h, rc, gc, rp, gp, mean16, np.full(w * h, 16, F))
            s4 = total(rc, 4, seed + 1000)
            has = hh > 0
            mse = lambda a: float(((a[has].astype(np.float64) - ref[has]) ** 2).mean())
            out.append(mse(M.blend(s4, 4, hm, hh)) / mse(M.blend(s4, 4)))
        print(f"cap {cap:g}: pixels with history {int(has.sum())} of {w * h}; ratios " + " ".join(f"{r:.4f}" for r in out)
              + f"; worst {max(out):.4f}, bound sqrt(worst) {np.sqrt(max(out)):.4f}")
