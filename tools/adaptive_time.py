"""What adaptive sampling (sphip_accum_begin_adaptive) saves on the configs[2] frame (closed_room(10000), 1920x1080): uniform
progressive steps against adaptive runs at several thresholds, each as 64 steps of 4 spp -- the sum of the steps' kernel_ms, the
scans executed, the active fraction after selected steps, the mean samples per pixel, and the RMS error of the final mean against
a long uniform render with another seed.  Then the cost of an adaptive step while nothing can stop yet (min_samples above the
total) against a plain step, alternated.
python tools/adaptive_time.py [steps [ref_spp]]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from spath_amd import capi, scene, view
n_steps = int(sys.argv[1]) if len(sys.argv) > 1 else 64
ref_spp = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
per, nt, w, h = 4, 10000, 1920, 1080
RULES = [(0.2, 0.05, 16), (0.05, 0.05, 16), (0.05, 0.05, 64)]
ctx = capi.Context(0)
t, m = scene.closed_room(nt)
ctx.set_scene(t, m)
rays = np.ascontiguousarray(view.Camera(w, h).get_viewport(), dtype=np.float32)
ctx.render(rays, w, h, 1)                                    # first use: record streams built, kernels loaded
print(f"library {capi.build_source_hash()}, {ctx.description}; closed_room({nt}) {w}x{h}, {n_steps} steps of {per} spp", flush=True)
_, ref = ctx.render(rays, w, h, ref_spp, seed=987654321, want_accum=True)
print(f"reference: uniform {ref_spp} spp, seed 987654321, kernel {ctx.stats()['kernel_ms']:.1f} ms", flush=True)
marks = {1, 2, 4, 8, 16, 32, 48, n_steps}


def run(rule):
    ctx.accum_begin(rays=rays, w=w, h=h, seed=1, adaptive=rule)
    kms, scans, frac = 0.0, 0, []
    for s in range(1, n_steps + 1):
        img, mean, total = ctx.accum_step(per, want_mean=True)
        st = ctx.stats()
        kms += st["kernel_ms"]; scans += st["scans_executed"]
        if s in marks:
            frac.append((s, ctx.accum_counts()[1] / (w * h)))
    counts, _ = ctx.accum_counts()
    rms = float(np.sqrt(np.mean((mean.astype(np.float64) - ref.astype(np.float64)) ** 2)))
    return kms, scans, frac, float(counts.mean()), rms


base = None
for rule in [None] + RULES:
    kms, scans, frac, spp_mean, rms = run(rule)
    base = base or (kms, scans)
    name = "uniform            " if rule is None else f"adaptive t={rule[0]:<4} f={rule[1]} min={rule[2]}"
    fr = " ".join(f"{s}:{f:.3f}" for s, f in frac)
    print(f"{name}: kernel sum {kms:9.2f} ms ({(kms / base[0] - 1) * 100:+6.1f} %), scans {scans} ({(scans / base[1] - 1) * 100:+6.1f} %), "
          f"mean spp {spp_mean:6.1f}, RMS error of the mean {rms:.5f}; active fraction after step {fr}", flush=True)

# overhead while nothing can stop: min_samples above the total, alternated with plain steps
k = 16
for rep in range(2):
    for rule in (None, (0.05, 0.05, per * k + 1)):
        ctx.accum_begin(rays=rays, w=w, h=h, seed=1, adaptive=rule)
        ms, launches = [], set()
        for _ in range(k):
            ctx.accum_step(per)
            st = ctx.stats()
            ms.append(st["kernel_ms"]); launches.add(st["n_launches"])
        print(f"[{rep}] {'plain   ' if rule is None else 'adaptive'} step of {per} spp, nothing stops: kernel {np.mean(ms):.3f} ms per step "
              f"(median {np.median(ms):.3f}), launches/step {sorted(launches)}", flush=True)
ctx.close()
