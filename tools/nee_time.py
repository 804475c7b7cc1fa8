"""What next-event estimation (SPHIP_FLAG_NEE) costs and gains on the configs[2] frame (closed_room(10000), 1920x1080): kernel time
per sample with and without the flag (alternated, default variant), the scans of each (path scans; with NEE plus one per shadow
ray), hence what a shadow ray costs against a path scan, and the RMS error of each estimator's mean against a long plain render
with another seed, at 16 spp and at equal kernel time.
python tools/nee_time.py [spp [ref_spp]]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from spath_amd import capi, scene, view
spp = int(sys.argv[1]) if len(sys.argv) > 1 else 16
ref_spp = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
nt, w, h = 10000, 1920, 1080
ctx = capi.Context(0)
t, m = scene.closed_room(nt)
ctx.set_scene(t, m)
rays = np.ascontiguousarray(view.Camera(w, h).get_viewport(), dtype=np.float32)
ctx.render(rays, w, h, 1)                                    # first use: record streams built, kernels loaded
ctx.render(rays, w, h, 1, flags=capi.FLAG_NEE)               # ... and the light table
print(f"library {capi.build_source_hash()}, {ctx.description}; closed_room({nt}) {w}x{h}", flush=True)
_, ref = ctx.render(rays, w, h, ref_spp, seed=987654321, want_accum=True)
ref = ref.astype(np.float64)
print(f"reference: plain {ref_spp} spp, seed 987654321, kernel {ctx.stats()['kernel_ms']:.1f} ms", flush=True)


def run(flags, n, seed=1, detail=False):
    _, mean = ctx.render(rays, w, h, n, seed=seed, flags=flags, want_accum=True)
    st = ctx.stats()
    e2 = ((mean.astype(np.float64) - ref) ** 2).sum(1)
    if detail:
        # where the error sits: share of the squared error in the worst 0.1 % of pixels and their rows; RMS of the clamped image
        k = max(1, e2.size // 1000)
        worst = np.argsort(e2)[-k:]
        rows = worst // w
        clamped = np.sqrt(np.mean((np.clip(mean, 0, 1).astype(np.float64) - np.clip(ref, 0, 1)) ** 2))
        print(f"      worst 0.1 % of pixels hold {e2[worst].sum() / e2.sum() * 100:.1f} % of the squared error (rows {np.percentile(rows, 5):.0f}-"
              f"{np.percentile(rows, 95):.0f} of {h}); RMS without them {np.sqrt(np.delete(e2, worst).sum() / (e2.size - k) / 3):.5f}; "
              f"RMS of the [0,1]-clamped images {clamped:.5f}", flush=True)
    return st["kernel_ms"], st["scans_executed"], float(np.sqrt(e2.mean() / 3))


res = {}
for rep in range(3):
    for name, f in (("plain", 0), ("nee", capi.FLAG_NEE)):
        ms, sc, rms = run(f, spp, detail=rep == 0)
        res.setdefault(name, []).append((ms, sc, rms))
        print(f"[{rep}] {name:5s} {spp} spp: kernel {ms:9.2f} ms ({ms / spp:7.3f} ms/sample), scans {sc}, RMS {rms:.5f}", flush=True)
pm = np.median([r[0] for r in res["plain"]]); nm = np.median([r[0] for r in res["nee"]])
ps, ns = res["plain"][0][1], res["nee"][0][1]
print(f"median kernel per sample: plain {pm / spp:.3f} ms, NEE {nm / spp:.3f} ms ({(nm / pm - 1) * 100:+.1f} %)")
print(f"scans: plain {ps}, NEE {ns} (path + shadow); time per plain scan {pm / ps * 1e6:.3f} ns, per NEE scan {nm / ns * 1e6:.3f} ns")
# equal kernel time: NEE with the number of samples its per-sample cost affords in the plain run's time (at least 1)
n_eq = max(1, int(round(spp * pm / nm)))
ms, sc, rms = run(capi.FLAG_NEE, n_eq, detail=True)
print(f"equal time: plain {spp} spp {pm:.1f} ms RMS {res['plain'][0][2]:.5f}  vs  NEE {n_eq} spp {ms:.1f} ms RMS {rms:.5f} "
      f"(ratio {rms / res['plain'][0][2]:.3f})", flush=True)
ctx.close()
