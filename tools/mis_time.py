"""What multiple importance sampling (SPHIP_FLAG_NEE | SPHIP_FLAG_MIS) costs and gains on the configs[2] frame (closed_room(10000),
1920x1080), against the plain estimator and NEE alone: kernel time per sample (alternated, default variant), the scans of each
(path scans, plus one per shadow ray), and the RMS error of each estimator's mean against a long plain render with another seed,
full-range and on [0,1]-clamped images, at 16 spp and at equal kernel time.
python tools/mis_time.py [spp [ref_spp]]"""
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
EST = (("plain", 0), ("nee", capi.FLAG_NEE), ("mis", capi.FLAG_NEE | capi.FLAG_MIS))
for _, f in EST:
    ctx.render(rays, w, h, 1, flags=f)                        # first use: record streams built, kernels loaded, light table
print(f"library {capi.build_source_hash()}, {ctx.description}; closed_room({nt}) {w}x{h}", flush=True)
_, ref = ctx.render(rays, w, h, ref_spp, seed=987654321, want_accum=True)
ref = ref.astype(np.float64)
print(f"reference: plain {ref_spp} spp, seed 987654321, kernel {ctx.stats()['kernel_ms']:.1f} ms", flush=True)


def run(flags, n, seed=1):
    _, mean = ctx.render(rays, w, h, n, seed=seed, flags=flags, want_accum=True)
    st = ctx.stats()
    full = float(np.sqrt(np.mean((mean.astype(np.float64) - ref) ** 2)))
    clamped = float(np.sqrt(np.mean((np.clip(mean, 0, 1).astype(np.float64) - np.clip(ref, 0, 1)) ** 2)))
    return st["kernel_ms"], st["scans_executed"], full, clamped


res = {}
for rep in range(3):
    for name, f in EST:
        ms, sc, full, cl = run(f, spp)
        res.setdefault(name, []).append((ms, sc, full, cl))
        print(f"[{rep}] {name:5s} {spp} spp: kernel {ms:9.2f} ms ({ms / spp:7.3f} ms/sample), scans {sc}, RMS {full:.5f}, clamped {cl:.5f}",
              flush=True)
med = {k: float(np.median([r[0] for r in v])) for k, v in res.items()}
npx = w * h * spp
for name, _ in EST:
    sc = res[name][0][1]
    print(f"{name:5s}: median kernel {med[name] / spp:.3f} ms/sample ({(med[name] / med['plain'] - 1) * 100:+.1f} % vs plain), "
          f"scans {sc} ({sc / npx:.2f} per path), {med[name] / sc * 1e6:.3f} ns per scan; RMS {res[name][0][2]:.5f}, clamped {res[name][0][3]:.5f}")
# equal kernel time: each estimator with the number of samples its per-sample cost affords in the plain run's time (at least 1)
for name, f in EST[1:]:
    n_eq = max(1, int(round(spp * med["plain"] / med[name])))
    ms, sc, full, cl = run(f, n_eq)
    print(f"equal time: plain {spp} spp {med['plain']:.1f} ms RMS {res['plain'][0][2]:.5f} clamped {res['plain'][0][3]:.5f}  vs  "
          f"{name} {n_eq} spp {ms:.1f} ms RMS {full:.5f} clamped {cl:.5f}", flush=True)
ctx.close()
