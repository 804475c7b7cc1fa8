"""What transparency (SPHIP_FLAG_DIELECTRIC) costs on the configs[2] frame (closed_room(10000), 1920x1080) with a glass icosphere(3)
(1280 triangles, ior 1.5, smooth) two units in front of the camera: kernel time per sample of the plain estimator and of NEE|MIS,
each unflagged, flagged with a table of zeros (the same image) and flagged with the sphere's table, for the default variant (16:
rpl_cylm) and the BVH (8), alternated; and the scans per path of each.
python tools/dielectric_time.py [spp [reps]]  (writes what it prints to profiles/dielectric.log)
Every (variant, estimator) step runs in a process of its own under a time limit of its own; the first step that fails, faults or
runs out of time ends the run."""
import os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from spath_amd import capi, scene, view

VARIANTS = {"16": 16, "8": capi.FLAG_ACCEL}
EST = {"plain": 0, "mis": capi.FLAG_NEE | capi.FLAG_MIS}
NT, W, H = 10000, 1920, 1080
STEP_LIMIT_S = 240


def step(vname, ename, spp, reps):
    """one (variant, estimator): the three cases alternated reps times -> lines on stdout"""
    ctx = capi.Context(0)
    rays = np.ascontiguousarray(view.Camera(W, H).get_viewport(), dtype=np.float32)
    centre = rays[(H // 2) * W + W // 2]
    t0, m0 = scene.closed_room(NT)
    ts, ms = scene.icosphere(3, tuple(centre[0:3] + 2.0 * centre[3:6]), 0.6, (0.1, 0.1, 0.1, 0, 0, 0))
    t, m = np.concatenate([t0, ts]), np.concatenate([m0, ms])
    sphere = np.arange(NT, t.shape[0])
    ctx.set_scene(t, m)
    ctx.set_vertex_normals(scene.vertex_normals(t, which=sphere))
    zeros = np.zeros((t.shape[0], 4), np.float32)
    glass = scene.dielectric_table(t, 1.5, (0.9, 0.95, 1.0), which=sphere)
    G, S = capi.FLAG_DIELECTRIC, capi.FLAG_SMOOTH
    cases = (("no flag", 0, None), ("flag, zero table", G, zeros), ("flag, glass sphere", G, glass))
    f0 = VARIANTS[vname] | EST[ename] | S
    ctx.set_dielectric(zeros)
    for _, f, _ in cases:                                     # first use: record streams built, kernels loaded, light table
        ctx.render(rays, W, H, 1, flags=f | f0)
    print(f"library {capi.build_source_hash()}, {ctx.description}; closed_room({NT}) + glass icosphere(3) {W}x{H}, {spp} spp", flush=True)
    res = {}
    npx = W * H * spp
    for rep in range(reps):
        for name, f, tab in cases:
            if tab is not None:
                ctx.set_dielectric(tab)
            ctx.render(rays, W, H, spp, seed=1, flags=f | f0)
            st = ctx.stats()
            res.setdefault(name, []).append((st["kernel_ms"], st["scans_executed"]))
            print(f"[{rep}] variant {vname:>2s} {ename:5s} {name:18s}: kernel {st['kernel_ms']:9.2f} ms ({st['kernel_ms'] / spp:7.3f} ms/sample), "
                  f"scans {st['scans_executed']} ({st['scans_executed'] / npx:.3f} per path)", flush=True)
    base = float(np.median([r[0] for r in res[cases[0][0]]]))
    for name, _, _ in cases:
        ms_ = [r[0] for r in res[name]]
        med = float(np.median(ms_))
        sc = res[name][0][1]
        print(f"variant {vname:>2s} {ename:5s} {name:18s}: median {med / spp:7.3f} ms/sample (min {min(ms_) / spp:.3f}, max {max(ms_) / spp:.3f}; "
              f"{(med / base - 1) * 100:+.1f} % vs no flag), {sc / npx:.3f} scans per path, {med / sc * 1e6:.3f} ns per scan", flush=True)
    ctx.close()


def main():
    spp = sys.argv[1] if len(sys.argv) > 1 else "16"
    reps = sys.argv[2] if len(sys.argv) > 2 else "3"
    with open(os.path.join(ROOT, "profiles", "dielectric.log"), "w") as out:
        for vname in VARIANTS:
            for ename in EST:
                r = subprocess.run(["timeout", "-k", "10", str(STEP_LIMIT_S), sys.executable, os.path.abspath(__file__), "--step", vname, ename, spp, reps],
                                   capture_output=True, text=True)
                sys.stdout.write(r.stdout)
                sys.stdout.flush()
                out.write(r.stdout)
                out.flush()
                if r.returncode != 0:                          # nothing more is started on the device after a failure
                    msg = f"step variant {vname} {ename} ended with status {r.returncode}; the run stops here\n{r.stderr[-2000:]}"
                    sys.stdout.write(msg + "\n")
                    out.write(msg + "\n")
                    return r.returncode
    return 0


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--step":
        step(sys.argv[2], sys.argv[3], int(sys.argv[4]), int(sys.argv[5]))
    else:
        sys.exit(main())
