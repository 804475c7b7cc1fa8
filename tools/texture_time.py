"""What textures (SPHIP_FLAG_TEXTURE) cost on the configs[2] frame (closed_room(10000), 1920x1080) whose
clutter is mixed diffuse/mirror (p = 0.5): kernel time per sample of the plain estimator and of NEE|MIS, each with the glossy-flagged
kernel (SPHIP_FLAG_SPECULAR | SPHIP_FLAG_GLOSSY, a roughness table of zeros: the GlossArgs twin of the textured kernel), with
SPHIP_FLAG_TEXTURE and a UV table of zeros on top (the same image) and with every triangle textured (three repeats of a 64 x 64
checker), for the default variant (16: rpl_cylm) and the BVH (8); and the scans per path of each.
python tools/texture_time.py [spp [reps]]  (writes what it prints to profiles/texture.log)
Every case runs in a process of its own under a time limit of its own, the three cases of a (variant, estimator) alternated reps
times; the first process that fails, faults or runs out of time ends the run."""
import os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from spath_amd import capi, scene, view

VARIANTS = {"16": 16, "8": capi.FLAG_ACCEL}
EST = {"plain": 0, "mis": capi.FLAG_NEE | capi.FLAG_MIS}
CASES = ("glossy flag", "tex flag, zero UVs", "tex flag, textured")
NT, W, H = 10000, 1920, 1080
STEP_LIMIT_S = 120


def one(vname, ename, case, spp):
    """one render of one case -> 'kernel_ms scans' on stdout"""
    ctx = capi.Context(0)
    rays = np.ascontiguousarray(view.Camera(W, H).get_viewport(), dtype=np.float32)
    t, m = scene.closed_room(NT)
    clutter = np.arange(14, NT)
    ctx.set_scene(t, m)
    ctx.set_specular(scene.specular_table(t, m, 0.8, which=clutter, p=0.5))
    ctx.set_roughness(scene.roughness_table(t, 0.0))
    f = VARIANTS[vname] | EST[ename] | capi.FLAG_SPECULAR | capi.FLAG_GLOSSY
    if case != CASES[0]:
        ctx.set_texture(scene.checker_texture(64, 64, 8, (0.95, 0.9, 0.8), (0.15, 0.25, 0.5)))
        ctx.set_uv(np.zeros((NT, 6), np.float32) if case == CASES[1] else scene.uv_table(t, (0, 0, 3, 0, 0, 3)))
        f |= capi.FLAG_TEXTURE
    ctx.render(rays, W, H, 1, flags=f)                        # first use: record streams built, kernels loaded, light table
    ctx.render(rays, W, H, spp, seed=1, flags=f)
    st = ctx.stats()
    print(f"{st['kernel_ms']!r} {st['scans_executed']} {capi.build_source_hash()} {ctx.description}", flush=True)
    ctx.close()


def main():
    spp = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    npx = W * H * spp
    with open(os.path.join(ROOT, "profiles", "texture.log"), "w") as out:
        def say(s):
            sys.stdout.write(s + "\n")
            sys.stdout.flush()
            out.write(s + "\n")
            out.flush()
        first = True
        for vname in VARIANTS:
            for ename in EST:
                res = {}
                for rep in range(reps):
                    for case in CASES:
                        r = subprocess.run(["timeout", "-k", "10", str(STEP_LIMIT_S), sys.executable, os.path.abspath(__file__), "--one", vname, ename, case, str(spp)],
                                           capture_output=True, text=True)
                        if r.returncode != 0:                  # nothing more is started on the device after a failure
                            say(f"variant {vname} {ename} {case!r} ended with status {r.returncode}; the run stops here\n{r.stderr[-2000:]}")
                            return r.returncode
                        ms_, sc, src, desc = r.stdout.split(None, 3)
                        if first:
                            say(f"library {src}, {desc.strip()}; closed_room({NT}), clutter p = 0.5, {W}x{H}, {spp} spp")
                            first = False
                        res.setdefault(case, []).append((float(ms_), int(sc)))
                        say(f"[{rep}] variant {vname:>2s} {ename:5s} {case:20s}: kernel {float(ms_):9.2f} ms ({float(ms_) / spp:7.3f} ms/sample), "
                            f"scans {sc} ({int(sc) / npx:.3f} per path)")
                base = [r[0] for r in res[CASES[0]]]
                for case in CASES:
                    v = [r[0] for r in res[case]]
                    med, sc = float(np.median(v)), res[case][0][1]
                    inside = min(base) <= med <= max(base)
                    say(f"variant {vname:>2s} {ename:5s} {case:20s}: median {med / spp:7.3f} ms/sample (min {min(v) / spp:.3f}, max {max(v) / spp:.3f}; "
                        f"{(med / float(np.median(base)) - 1) * 100:+.2f} % vs the glossy flag, whose runs spread {(max(base) / min(base) - 1) * 100:.2f} %: "
                        f"{'inside' if inside else 'OUTSIDE'} that spread), {sc / npx:.3f} scans per path, {med / sc * 1e6:.3f} ns per scan")
                if res[CASES[0]][0][1] != res[CASES[1]][0][1]:
                    say("a UV table of zeros changed scans_executed")
                    return 1
    return 0


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--one":
        one(sys.argv[2], sys.argv[3], sys.argv[4], int(sys.argv[5]))
    else:
        sys.exit(main())
