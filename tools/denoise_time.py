"""What the denoiser (sphip_gbuffer_device, sphip_denoise_device, sphip_accum_denoise) costs and buys on the configs[2] frame
(closed_room(10000), 1920x1080): the G-buffer build against the closest-hit scan alone; the filter per iteration (K = 5 minus
K = 0, over 5) for both kernels (taps staged in LDS, taps read through the caches) and the HBM bandwidth that implies at 64 B per pixel and iteration (16 B in, 32 B G-buffer, 16 B out) against
8 TB/s; then the quality: RMS error of the mean and of the denoised image against a long render with another seed, at
1/4/16/64/256 spp, with the defaults and a small parameter grid (the calibration of sphip_denoise_defaults).
python tools/denoise_time.py [ref_spp]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from spath_amd import capi, scene, view

ref_spp = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
nt, w, h = 10000, 1920, 1080
n = w * h
NEVER = (0.0, 0.0, 0xFFFFFFFF)
ctx = capi.Context(0)
t, m = scene.closed_room(nt)
ctx.set_scene(t, m)
rays = np.ascontiguousarray(view.Camera(w, h).get_viewport(), dtype=np.float32)
print(f"library {capi.build_source_hash()}, {ctx.description}; closed_room({nt}) {w}x{h}", flush=True)

dev = torch.device("cuda:0")
st = torch.cuda.current_stream().cuda_stream
d_rays = torch.from_numpy(rays).to(dev)
d_g = torch.zeros(n * 32, dtype=torch.uint8, device=dev)
d_idx = torch.zeros(n, dtype=torch.int32, device=dev)
d_d = torch.zeros(n, dtype=torch.float32, device=dev)
d_rgba = torch.zeros((n, 4), dtype=torch.uint8, device=dev)
d_rgb = torch.zeros((n, 3), dtype=torch.float32, device=dev)


def timed(fn, reps=7):
    ms = []
    for _ in range(reps):
        fn()
        torch.cuda.synchronize()
        ms.append(ctx.stats()["kernel_ms"])
    return float(np.median(ms[1:])), ctx.stats()


hit_ms, _ = timed(lambda: ctx.closest_hit_device(d_rays.data_ptr(), n, d_idx.data_ptr(), d_d.data_ptr(), stream=st))
gb_ms, s = timed(lambda: ctx.gbuffer_device(d_rays.data_ptr(), n, d_g.data_ptr(), stream=st))
print(f"G-buffer: {gb_ms:.3f} ms (closest-hit scan alone {hit_ms:.3f} ms, entry kernel {gb_ms - hit_ms:.3f} ms), "
      f"scans {s['scans_executed']}, launches {s['n_launches']}", flush=True)

_, mean4 = ctx.render(rays, w, h, 4, seed=1, want_accum=True)
d_mean = torch.from_numpy(mean4).to(dev)
d_var = torch.full((n,), 0.01, dtype=torch.float32, device=dev)
default_kernel = os.environ.get("SPATH_HIP_ATROUS")
outs = {}
for kern in ("lds", "l2"):                                   # SPATH_HIP_ATROUS: taps staged in LDS, or read through the caches
    os.environ["SPATH_HIP_ATROUS"] = kern
    per_k = {}
    for rep in range(2):                                     # alternated with the other kernel's block below
        for K in (0, 1, 5):
            for var in (False, True):
                ms, s = timed(lambda: ctx.denoise_device(w, h, d_mean.data_ptr(), d_g.data_ptr(), d_rgba.data_ptr(),
                                                         d_var=d_var.data_ptr() if var else 0, d_out_rgb=d_rgb.data_ptr(),
                                                         params=dict(iterations=K), stream=st), reps=11)
                per_k.setdefault((K, var), []).append(ms)
    for K in (0, 1, 5):
        for var in (False, True):
            print(f"[{kern}] filter K={K} {'with' if var else 'without'} variance: " + " / ".join(f"{x:.3f}" for x in per_k[(K, var)])
                  + f" ms ({K + 1} launches)", flush=True)
    for var in (False, True):
        it = (min(per_k[(5, var)]) - min(per_k[(0, var)])) / 5
        gbs = 64.0 * n / (it * 1e-3) / 1e9
        print(f"[{kern}] per iteration ({'with' if var else 'without'} variance): {it:.3f} ms -> {gbs:.0f} GB/s at 64 B/pixel "
              f"({gbs / 8000 * 100:.1f} % of 8 TB/s)", flush=True)
    torch.cuda.synchronize()
    outs[kern] = (d_rgba.cpu().numpy().copy(), d_rgb.cpu().numpy().copy())
print(f"lds and l2 outputs identical: {all(np.array_equal(a, b) for a, b in zip(outs['lds'], outs['l2']))}", flush=True)
if default_kernel is None:
    del os.environ["SPATH_HIP_ATROUS"]
else:
    os.environ["SPATH_HIP_ATROUS"] = default_kernel

step4 = ctx.render(rays, w, h, 4, seed=1)
print(f"a 4-spp render of this frame: kernel {ctx.stats()['kernel_ms']:.2f} ms", flush=True)

# ---- quality
_, ref = ctx.render(rays, w, h, ref_spp, seed=987654321, want_accum=True)
ref = ref.astype(np.float64)
print(f"reference: {ref_spp} spp, seed 987654321", flush=True)


def rms(a):
    return float(np.sqrt(np.mean((a.astype(np.float64) - ref) ** 2)))


GRID = [dict(iterations=k, sigma_lum=sl, sigma_depth=sz, normal_log2=nl)
        for k in (3, 4, 5, 6) for sl in (2.0, 4.0, 8.0, 16.0) for sz in (0.05, 0.1, 0.3, 1.0) for nl in (2, 7)]
marks = (1, 4, 16, 64, 256)
for rule, name in ((NEVER, "with variance (never-stopping adaptive rule)"), (None, "plain accumulation (no variance)")):
    ctx.accum_begin(rays=rays, w=w, h=h, seed=1, adaptive=rule)
    total = 0
    print(f"-- {name}", flush=True)
    for mk in marks:
        _, mean, total = ctx.accum_step(mk - total, want_mean=True)
        _, den = ctx.accum_denoise(want_rgb=True)
        dms = ctx.stats()["kernel_ms"]
        r0, r1 = rms(mean), rms(den)
        line = f"{mk:4d} spp: RMS raw {r0:.5f}, denoised (defaults) {r1:.5f}, ratio {r1 / r0:.3f}, denoise kernel {dms:.3f} ms"
        if mk in (4, 16) and rule is not None:
            scores = []
            for p in GRID:
                _, dg = ctx.accum_denoise(p, want_rgb=True)
                scores.append((rms(dg) / r0, p))
            scores.sort(key=lambda x: x[0])
            line += "; grid best " + ", ".join(f"{r:.3f} {p}" for r, p in scores[:3])
        print(line, flush=True)

# ---- the frame of tests/test_hip_denoise.py's quality check: closed_room(200), 96x64, 16 spp, seed 1, against 1024 spp of seed 1000
t2, m2 = scene.closed_room(200)
ctx.set_scene(t2, m2)
w2, h2 = 96, 64
rays2 = np.ascontiguousarray(view.Camera(w2, h2).get_viewport(), dtype=np.float32)
_, ref2 = ctx.render(rays2, w2, h2, 1024, seed=1000, want_accum=True)
ref2 = ref2.astype(np.float64)
ctx.accum_begin(rays=rays2, w=w2, h=h2, seed=1, adaptive=NEVER)
_, mean2, _ = ctx.accum_step(16, want_mean=True)
r0 = float(np.sqrt(np.mean((mean2 - ref2) ** 2)))
scores = []
for p in [None] + GRID:
    _, dg = ctx.accum_denoise(p, want_rgb=True)
    scores.append((float(np.sqrt(np.mean((dg - ref2) ** 2))) / r0, p))
print(f"-- closed_room(200) 96x64, 16 spp: RMS raw {r0:.5f}; denoised/raw with the defaults {scores[0][0]:.3f}; grid best "
      + ", ".join(f"{r:.3f} {p}" for r, p in sorted(scores[1:], key=lambda x: x[0])[:5]), flush=True)
ctx.close()
