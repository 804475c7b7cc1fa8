"""What normal mapping (SPHIP_FLAG_NORMAL_MAP) costs on the configs[2] frame (closed_room(10000), 1920x1080) whose
clutter is mixed diffuse/mirror (p = 0.5): kernel time per sample of the plain estimator and of NEE|MIS, each with the textured
kernel on a UV table of zeros (SPHIP_FLAG_SPECULAR | SPHIP_FLAG_GLOSSY | SPHIP_FLAG_TEXTURE, a roughness table of zeros: the TexArgs
twin of the normal-mapped kernel), with the same kernel on three repeats per triangle of a 1 x 1 white atlas (the same image again),
and with SPHIP_FLAG_NORMAL_MAP in SPHIP_FLAG_TEXTURE's place over the same UVs under a flat map ((0, 0, 1) everywhere: the same image)
and under a bumpy 64 x 64 map, for the default variant (16: rpl_cylm) and the BVH (8); and the scans per path of each.
The two twins separate two costs.  On zero UVs tex_albedo returns before it samples; a normal-mapped kernel without SPHIP_FLAG_TEXTURE
samples the context's white texel at real UVs.  So "against the twin on zero UVs" includes that sample, which is texturing's cost, and
"against the twin on a white atlas" is nmap_normal's alone (with the NormArgs the pack always carries).
python tools/normal_map_time.py [spp [reps]]  (writes what it prints to profiles/normal_map.log)
Every case runs in a process of its own under a time limit of its own, the four cases of a (variant, estimator) alternated reps
times; the first process that fails, faults or runs out of time ends the run."""
import os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from spath_amd import capi, scene, view

VARIANTS = {"16": 16, "8": capi.FLAG_ACCEL}
EST = {"plain": 0, "mis": capi.FLAG_NEE | capi.FLAG_MIS}
CASES = ("tex flag, zero UVs", "tex flag, white atlas", "nmap flag, flat map", "nmap flag, bumpy map")
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
    if case == CASES[0]:
        ctx.set_texture(scene.checker_texture(64, 64, 8, (0.95, 0.9, 0.8), (0.15, 0.25, 0.5)))
        ctx.set_uv(np.zeros((NT, 6), np.float32))
        f |= capi.FLAG_TEXTURE
    elif case == CASES[1]:
        ctx.set_texture(np.ones((1, 1, 3), np.float32))
        ctx.set_uv(scene.uv_table(t, (0, 0, 3, 0, 0, 3)))
        f |= capi.FLAG_TEXTURE
    else:
        height = np.zeros((64, 64)) if case == CASES[2] else np.random.default_rng(1).random((64, 64))
        ctx.set_normal_map(scene.normal_map_from_height(height, 2.0))
        ctx.set_uv(scene.uv_table(t, (0, 0, 3, 0, 0, 3)))
        f |= capi.FLAG_NORMAL_MAP
    ctx.render(rays, W, H, 1, flags=f)                        # first use: record streams built, kernels loaded, light table
    ctx.render(rays, W, H, spp, seed=1, flags=f)
    st = ctx.stats()
    print(f"{st['kernel_ms']!r} {st['scans_executed']} {capi.build_source_hash()} {ctx.description}", flush=True)
    ctx.close()


def main():
    spp = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    npx = W * H * spp
    with open(os.path.join(ROOT, "profiles", "normal_map.log"), "w") as out:
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
                        say(f"[{rep}] variant {vname:>2s} {ename:5s} {case:21s}: kernel {float(ms_):9.2f} ms ({float(ms_) / spp:7.3f} ms/sample), "
                            f"scans {sc} ({int(sc) / npx:.3f} per path)")
                base = [r[0] for r in res[CASES[0]]]
                white = float(np.median([r[0] for r in res[CASES[1]]]))
                for case in CASES:
                    v = [r[0] for r in res[case]]
                    med, sc = float(np.median(v)), res[case][0][1]
                    inside = min(base) <= med <= max(base)
                    say(f"variant {vname:>2s} {ename:5s} {case:21s}: median {med / spp:7.3f} ms/sample (min {min(v) / spp:.3f}, max {max(v) / spp:.3f}; "
                        f"{(med / float(np.median(base)) - 1) * 100:+.2f} % vs zero UVs, whose runs spread {(max(base) / min(base) - 1) * 100:.2f} %: "
                        f"{'inside' if inside else 'OUTSIDE'} that spread; {(med / white - 1) * 100:+.2f} % vs the white atlas), {sc / npx:.3f} scans per path, {med / sc * 1e6:.3f} ns per scan")
                if len({res[c][0][1] for c in CASES[:3]}) != 1:
                    say("a white atlas or a flat map changed scans_executed")
                    return 1
    return 0


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--one":
        one(sys.argv[2], sys.argv[3], sys.argv[4], int(sys.argv[5]))
    else:
        sys.exit(main())
