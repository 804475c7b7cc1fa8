"""What per-sample camera rays (SPHIP_FLAG_CAMERA_SAMPLES) cost on the configs[2] frame (closed_room(10000), 1920x1080): kernel time
per sample of sphip_render_camera without the flag, with it (pinhole, box-filtered pixel) and with it and a lens, for the default
variant (16 on this scene: rpl_cylm), the f32 cylinder scan (15) and the BVH (8), alternated; and the scans of each (the flag adds none).
python tools/camera_time.py [spp [reps]]  (writes what it prints to profiles/camera.log)"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from spath_amd import capi, scene, view
spp = int(sys.argv[1]) if len(sys.argv) > 1 else 16
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
nt, w, h = 10000, 1920, 1080
out = open(os.path.join(ROOT, "profiles", "camera.log"), "w")


def say(s):
    print(s, flush=True)
    out.write(s + "\n")
    out.flush()


ctx = capi.Context(0)
t, m = scene.closed_room(nt)
ctx.set_scene(t, m)
cam = view.Camera(w, h)
CASES = (("no flag", 0, None), ("flag, pinhole", capi.FLAG_CAMERA_SAMPLES, (0.0, 0.0)),
         ("flag, lens 0.05 @ 3", capi.FLAG_CAMERA_SAMPLES, (0.05, 3.0)))
VARIANTS = ((16, 16), (15, 15), (8, capi.FLAG_ACCEL))
for _, vf in VARIANTS:
    for _, f, lens in CASES:                                   # first use: record streams built, kernels loaded
        ctx.set_lens(*(lens or (0.0, 0.0)))
        ctx.render_camera(cam, 1, flags=f | vf)
say(f"library {capi.build_source_hash()}, {ctx.description}; closed_room({nt}) {w}x{h}, {spp} spp, sphip_render_camera")
res = {}
for rep in range(reps):
    for vname, vf in VARIANTS:
        for name, f, lens in CASES:
            ctx.set_lens(*(lens or (0.0, 0.0)))
            ctx.render_camera(cam, spp, seed=1, flags=f | vf)
            st = ctx.stats()
            res.setdefault((vname, name), []).append((st["kernel_ms"], st["scans_executed"]))
            say(f"[{rep}] variant {vname:2d} {name:20s}: kernel {st['kernel_ms']:9.2f} ms ({st['kernel_ms'] / spp:7.3f} ms/sample), "
                f"scans {st['scans_executed']}")
for vname, _ in VARIANTS:
    base = float(np.median([r[0] for r in res[(vname, CASES[0][0])]]))
    for name, _, _ in CASES:
        med = float(np.median([r[0] for r in res[(vname, name)]]))
        say(f"variant {vname:2d} {name:20s}: median {med / spp:7.3f} ms/sample ({(med / base - 1) * 100:+.1f} % vs no flag), "
            f"scans {res[(vname, name)][0][1]}")
ctx.close()
out.close()
