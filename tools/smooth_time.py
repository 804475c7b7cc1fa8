"""What smooth shading (SPHIP_FLAG_SMOOTH) costs on the configs[2] frame (closed_room(10000), 1920x1080): kernel time per sample of
the plain estimator and of NEE|MIS, each unflagged, flagged with a table of zeros (every triangle flat: the same image) and flagged
with scene.vertex_normals over the clutter (isolated triangles: their own face normals, so every clutter hit takes the smooth
path), for the default variant (16 on this scene: rpl_cylm) and the BVH (8), alternated; and the scans per path of each.
python tools/smooth_time.py [spp [reps]]  (writes what it prints to profiles/smooth.log)"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from spath_amd import capi, scene, view
spp = int(sys.argv[1]) if len(sys.argv) > 1 else 16
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
nt, w, h = 10000, 1920, 1080
out = open(os.path.join(ROOT, "profiles", "smooth.log"), "w")


def say(s):
    print(s, flush=True)
    out.write(s + "\n")
    out.flush()


ctx = capi.Context(0)
t, m = scene.closed_room(nt)
ctx.set_scene(t, m)
rays = np.ascontiguousarray(view.Camera(w, h).get_viewport(), dtype=np.float32)
zeros = np.zeros((nt, 9), np.float32)
clutter = scene.vertex_normals(t, which=np.arange(14, nt))
CASES = (("no flag", 0, None), ("flag, zero table", capi.FLAG_SMOOTH, zeros), ("flag, clutter normals", capi.FLAG_SMOOTH, clutter))
EST = (("plain", 0), ("mis", capi.FLAG_NEE | capi.FLAG_MIS))
VARIANTS = ((16, 16), (8, capi.FLAG_ACCEL))
ctx.set_vertex_normals(zeros)
for _, vf in VARIANTS:
    for _, ef in EST:
        for _, f, _ in CASES:                                 # first use: record streams built, kernels loaded, light table
            ctx.render(rays, w, h, 1, flags=f | ef | vf)
say(f"library {capi.build_source_hash()}, {ctx.description}; closed_room({nt}) {w}x{h}, {spp} spp; clutter normals: "
    f"{int(clutter.any(1).sum())} of {nt} triangles")
res = {}
npx = w * h * spp
for rep in range(reps):
    for vname, vf in VARIANTS:
        for ename, ef in EST:
            for name, f, tab in CASES:
                if tab is not None:
                    ctx.set_vertex_normals(tab)
                ctx.render(rays, w, h, spp, seed=1, flags=f | ef | vf)
                st = ctx.stats()
                res.setdefault((vname, ename, name), []).append((st["kernel_ms"], st["scans_executed"]))
                say(f"[{rep}] variant {vname:2d} {ename:5s} {name:21s}: kernel {st['kernel_ms']:9.2f} ms ({st['kernel_ms'] / spp:7.3f} ms/sample), "
                    f"scans {st['scans_executed']} ({st['scans_executed'] / npx:.3f} per path)")
for vname, _ in VARIANTS:
    for ename, _ in EST:
        base = float(np.median([r[0] for r in res[(vname, ename, CASES[0][0])]]))
        for name, _, _ in CASES:
            ms = [r[0] for r in res[(vname, ename, name)]]
            med = float(np.median(ms))
            sc = res[(vname, ename, name)][0][1]
            say(f"variant {vname:2d} {ename:5s} {name:21s}: median {med / spp:7.3f} ms/sample (min {min(ms) / spp:.3f}, max {max(ms) / spp:.3f}; "
                f"{(med / base - 1) * 100:+.1f} % vs no flag), {sc / npx:.3f} scans per path, {med / sc * 1e6:.3f} ns per scan")
ctx.close()
out.close()
