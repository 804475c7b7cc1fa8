"""What a progressive step costs (sphip_accum_begin / sphip_accum_step) on the configs[2] frame: 64 steps of 4 spp and 256 steps of
1 spp against one 256-spp render -- the sum of the steps' kernel_ms, wall time per step, and whether the final images (RGBA8 and
mean) are bit-identical.  Alternates the three forms twice.
python tools/progressive_time.py [spp [tris w h]]"""
import hashlib, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from spath_amd import capi, scene, view
spp = int(sys.argv[1]) if len(sys.argv) > 1 else 256
nt, w, h = (int(x) for x in sys.argv[2:5]) if len(sys.argv) > 4 else (10000, 1920, 1080)
ctx = capi.Context(0)
t, m = scene.closed_room(nt)
ctx.set_scene(t, m)
rays = np.ascontiguousarray(view.Camera(w, h).get_viewport(), dtype=np.float32)
ctx.render(rays, w, h, 1)                                    # first use: record streams built, kernels loaded
sha = lambda a: hashlib.sha256(a.tobytes()).hexdigest()[:16]
print(f"library {capi.build_source_hash()}, {ctx.description}; closed_room({nt}) {w}x{h}, {spp} spp", flush=True)
for rep in range(2):
    t0 = time.perf_counter()
    img0, mean0 = ctx.render(rays, w, h, spp, want_accum=True)
    wall0 = time.perf_counter() - t0
    st0 = ctx.stats()
    print(f"[{rep}] one shot  {spp:4d} spp: kernel {st0['kernel_ms']:9.2f} ms, wall {wall0 * 1e3:9.2f} ms (upload {st0['upload_ms']:.2f}, "
          f"download {st0['download_ms']:.2f}), scans {st0['scans_executed']}, rgba {sha(img0)} mean {sha(mean0)}", flush=True)
    for per in (4, 1):
        n_steps = spp // per
        t0 = time.perf_counter()
        ctx.accum_begin(rays=rays, w=w, h=h)
        t_begin = time.perf_counter() - t0
        kms, scans, walls, launches = 0.0, 0, [], set()
        for _ in range(n_steps):
            t1 = time.perf_counter()
            img, mean, total = ctx.accum_step(per, want_mean=True)
            walls.append(time.perf_counter() - t1)
            st = ctx.stats()
            kms += st["kernel_ms"]; scans += st["scans_executed"]; launches.add(st["n_launches"])
        same = np.array_equal(img, img0) and np.array_equal(mean.view(np.uint32), mean0.view(np.uint32))
        print(f"[{rep}] {n_steps:3d} x {per} spp: kernel sum {kms:9.2f} ms ({(kms / st0['kernel_ms'] - 1) * 100:+.2f} % vs one shot), "
              f"wall per step {np.mean(walls) * 1e3:.2f} ms (median {np.median(walls) * 1e3:.2f}, kernel {kms / n_steps:.2f}), begin {t_begin * 1e3:.2f} ms, "
              f"launches/step {sorted(launches)}, scans {scans} ({'equal' if scans == st0['scans_executed'] else 'DIFFERENT'}), "
              f"final image {'bit-identical' if same else 'DIFFERENT'} (rgba {sha(img)} mean {sha(mean)}, total {total})", flush=True)
        if not same:
            sys.exit(1)
