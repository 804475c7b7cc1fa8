"""What environment lighting (SPHIP_FLAG_ENVIRONMENT) costs on the configs[2] frame (closed_room(10000),
1920x1080): kernel time per sample of the plain estimator and of NEE|MIS, each unflagged, flagged with an all-zero map (the same image)
and flagged with the sky map (n = 64) in the same room with one wall removed (the wall the camera looks at), for the default variant
(16: rpl_cylm) and the BVH (8), alternated, median of three; and the scans per path of each.  A first step times the setters (the
device-pointer form between two events, the host form by the host clock) at n = 64, 512 and 2048.
python tools/env_time.py [spp [reps]]  (writes what it prints to profiles/environment.log)
Every step runs in a process of its own under a time limit of its own; the first step that fails, faults or runs out of time ends
the run."""
import os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from spath_amd import capi, scene, view

VARIANTS = {"16": 16, "8": capi.FLAG_ACCEL}
EST = {"plain": 0, "mis": capi.FLAG_NEE | capi.FLAG_MIS}
NT, W, H = 10000, 1920, 1080
STEP_LIMIT_S = 240


def open_room(t, m, rays):
    """the room without the wall that the centre ray of the camera hits: the two triangles of the room's box coplanar with that hit"""
    from oracle import oracle as O
    c = rays[(H // 2) * W + W // 2][None, :]
    idx, _ = O.closest_hits(np.ascontiguousarray(c, np.float32), t[:14], np.full(1, -1, np.int32))      # the box is the first triangles
    n, v = t[idx[0], 9:12], t[idx[0], 0:3]
    d = np.abs(((t[:14, 0:9].reshape(-1, 3, 3) - v) * n).sum(-1)).max(1)
    keep = np.ones(t.shape[0], bool)
    keep[:14] = ~((d < 1e-4) & (np.abs((t[:14, 9:12] * n).sum(1)) > 0.999))
    return np.ascontiguousarray(t[keep]), np.ascontiguousarray(m[keep]), int((~keep).sum())


def setters():
    import torch
    torch.cuda.is_available()
    ctx = capi.Context(0)
    print(f"library {capi.build_source_hash()}, {ctx.description}", flush=True)
    st = torch.cuda.current_stream()
    for n in (64, 512, 2048):
        env = scene.sky_environment(n)
        d = torch.from_numpy(env).to("cuda")
        dev_ms, host_ms = [], []
        for rep in range(6):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            ctx.set_environment_device(d.data_ptr(), n, st.cuda_stream)
            e1.record(st)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ctx.set_environment(env)
            t1 = time.perf_counter()
            if rep:                                                # the first round loads the kernels and sizes the buffers
                dev_ms.append(e0.elapsed_time(e1)), host_ms.append((t1 - t0) * 1e3)
        print(f"n {n:4d} ({env.nbytes / 2**20:6.2f} MiB): device setter {np.median(dev_ms):7.3f} ms (min {min(dev_ms):.3f}, max {max(dev_ms):.3f}); "
              f"host setter {np.median(host_ms):8.3f} ms (min {min(host_ms):.3f}, max {max(host_ms):.3f})", flush=True)
        del d
    ctx.close()


def step(vname, ename, spp, reps):
    """one (variant, estimator): the three cases alternated reps times -> lines on stdout"""
    rays = np.ascontiguousarray(view.Camera(W, H).get_viewport(), dtype=np.float32)
    t, m = scene.closed_room(NT)
    to, mo, gone = open_room(t, m, rays)
    zero, sky = np.zeros((4, 4, 3), np.float32), scene.sky_environment(64)
    E = capi.FLAG_ENVIRONMENT
    closed, opened = capi.Context(0), capi.Context(0)
    closed.set_scene(t, m)
    closed.set_environment(zero)
    opened.set_scene(to, mo)
    opened.set_environment(sky)
    cases = (("no flag", closed, 0), ("flag, zero map", closed, E), ("flag, sky, open wall", opened, E))
    f0 = VARIANTS[vname] | EST[ename]
    for _, c, f in cases:                                      # first use: record streams built, kernels loaded, light tables
        c.render(rays, W, H, 1, flags=f | f0)
    print(f"library {capi.build_source_hash()}, {closed.description}; closed_room({NT}) {W}x{H}, {spp} spp; the open room lacks {gone} triangles", flush=True)
    res = {}
    npx = W * H * spp
    for rep in range(reps):
        for name, c, f in cases:
            c.render(rays, W, H, spp, seed=1, flags=f | f0)
            st = c.stats()
            res.setdefault(name, []).append((st["kernel_ms"], st["scans_executed"]))
            print(f"[{rep}] variant {vname:>2s} {ename:5s} {name:20s}: kernel {st['kernel_ms']:9.2f} ms ({st['kernel_ms'] / spp:7.3f} ms/sample), "
                  f"scans {st['scans_executed']} ({st['scans_executed'] / npx:.3f} per path)", flush=True)
    base = [r[0] for r in res[cases[0][0]]]
    for name, _, _ in cases:
        ms_ = [r[0] for r in res[name]]
        med = float(np.median(ms_))
        sc = res[name][0][1]
        print(f"variant {vname:>2s} {ename:5s} {name:20s}: median {med / spp:7.3f} ms/sample (min {min(ms_) / spp:.3f}, max {max(ms_) / spp:.3f}; "
              f"{(med / float(np.median(base)) - 1) * 100:+.2f} % vs no flag, whose runs spread {(max(base) / min(base) - 1) * 100:.2f} %), "
              f"{sc / npx:.3f} scans per path, {med / sc * 1e6:.3f} ns per scan", flush=True)
    assert res[cases[0][0]][0][1] == res[cases[1][0]][0][1], "an all-zero map changed scans_executed"
    closed.close()
    opened.close()


def main():
    spp = sys.argv[1] if len(sys.argv) > 1 else "8"
    reps = sys.argv[2] if len(sys.argv) > 2 else "3"
    steps = [["--setters"]] + [["--step", v, e, spp, reps] for v in VARIANTS for e in EST]
    with open(os.path.join(ROOT, "profiles", "environment.log"), "w") as out:
        for args in steps:
            r = subprocess.run(["timeout", "-k", "10", str(STEP_LIMIT_S), sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True)
            sys.stdout.write(r.stdout)
            sys.stdout.flush()
            out.write(r.stdout)
            out.flush()
            if r.returncode != 0:                              # nothing more is started on the device after a failure
                msg = f"step {' '.join(args)} ended with status {r.returncode}; the run stops here\n{r.stderr[-2000:]}"
                sys.stdout.write(msg + "\n")
                out.write(msg + "\n")
                return r.returncode
    return 0


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--setters":
        setters()
    elif len(sys.argv) > 1 and sys.argv[1] == "--step":
        step(sys.argv[2], sys.argv[3], int(sys.argv[4]), int(sys.argv[5]))
    else:
        sys.exit(main())
