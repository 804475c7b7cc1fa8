"""What a camera move costs with temporal reprojection (sphip_reproject_device + sphip_temporal_resolve_device)
on the configs[2] frame (closed_room(10000), 1920x1080): the two kernels back to back, each on its own, for a pan of a few pixels and
for a turn that sends most of the frame off the old one; beside them what the move costs anyway (the new view's G-buffer), one
progressive step of 1 spp and the denoiser on the same frame.  Times are device events around BATCH back-to-back calls on one stream,
divided by BATCH; the median of REPS such windows after a warm-up, with the spread (min .. max).  Bandwidth: the bytes the operation
needs once (current G-buffer and rays 56 B, the previous view's G-buffer, rays, mean and count 72 B, outputs 16 B per pixel for the
reprojection; sum, history and outputs 12 + 16 + 16 B for the resolve) over the time, against 8 TB/s.
python tools/reproject_time.py"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from spath_amd import capi, scene, view

nt, w, h = 10000, 1920, 1080
n = w * h
BATCH, REPS, WARM = 20, 11, 2
ctx = capi.Context(0)
t, m = scene.closed_room(nt)
ctx.set_scene(t, m)
print(f"library {capi.build_source_hash()}, {ctx.description}; closed_room({nt}) {w}x{h}", flush=True)
dev = torch.device("cuda:0")
st = torch.cuda.current_stream().cuda_stream
params = capi.Reproject.defaults()
print(f"parameters (the defaults): {params.as_dict()}", flush=True)


def buf(nbytes):
    return torch.zeros(nbytes, dtype=torch.uint8, device=dev)


def window(fn):
    """median, min, max over REPS windows of BATCH calls, in ms per call"""
    ms = []
    for rep in range(WARM + REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(BATCH):
            fn()
        e1.record()
        e1.synchronize()
        if rep >= WARM:
            ms.append(e0.elapsed_time(e1) / BATCH)
    return float(np.median(ms)), min(ms), max(ms)


def look(moves):
    cam = view.Camera(w, h)
    for kind, val in moves:
        {"mov": cam.set_delta_mov, "rot": cam.set_delta_rot}[kind](val)
    rays, g = buf(n * 24), buf(n * 32)
    ctx.viewport_device(cam, rays.data_ptr(), st)
    ctx.gbuffer_device(rays.data_ptr(), n, g.data_ptr(), stream=st)
    torch.cuda.synchronize()
    return cam, rays, g, ctx.stats()["kernel_ms"]


prev, rays_p, g_p, _ = look(())
d_sum, d_rgba, d_mean = buf(n * 12), buf(n * 4), buf(n * 12)
ctx.render_device_accum(rays_p.data_ptr(), n, 0, 4, d_sum.data_ptr(), d_rgba.data_ptr(), seed=1, image_width=w, d_out_mean=d_mean.data_ptr(), stream=st)
torch.cuda.synchronize()
hist_p = torch.full((n,), 4.0, dtype=torch.float32, device=dev)
hm, hh, o_rgba, o_mean = buf(n * 12), buf(n * 4), buf(n * 4), buf(n * 12)
for name, moves in (("pan of a few pixels", (("mov", (0.02, 0.01, 0.0)),)), ("turn off the frame", (("rot", (0.0, 0.6, 0.0)),))):
    cur, rays_c, g_c, gb_ms = look(moves)

    def reproject():
        ctx.reproject_device(params, prev, w, h, rays_c.data_ptr(), g_c.data_ptr(), rays_p.data_ptr(), g_p.data_ptr(), d_mean.data_ptr(),
                             hist_p.data_ptr(), hm.data_ptr(), hh.data_ptr(), st)

    def resolve():
        ctx.temporal_resolve_device(n, d_sum.data_ptr(), 4, o_rgba.data_ptr(), o_mean.data_ptr(), d_hist_mean=hm.data_ptr(), d_hist=hh.data_ptr(), stream=st)

    both = window(lambda: (reproject(), resolve()))
    a, b = window(reproject), window(resolve)
    torch.cuda.synchronize()
    kept = float((hh.view(torch.float32) > 0).float().mean())
    print(f"-- {name}: {100 * kept:.1f} % of the pixels keep a history; the new view's G-buffer {gb_ms:.3f} ms", flush=True)
    print(f"reproject + resolve: {both[0]:.4f} ms ({both[1]:.4f} .. {both[2]:.4f})", flush=True)
    for what, r, nbytes in (("reproject", a, 144.0 * n), ("resolve", b, 44.0 * n)):
        gbs = nbytes / (r[0] * 1e-3) / 1e9
        print(f"{what}: {r[0]:.4f} ms ({r[1]:.4f} .. {r[2]:.4f}) -> {gbs:.0f} GB/s of needed bytes ({gbs / 8000 * 100:.1f} % of 8 TB/s)", flush=True)

# beside them: one progressive step and the denoiser on this frame (the library's own kernel clock, median of 5 after a warm-up)
ctx.accum_begin(cam=prev, seed=1)
step = []
for _ in range(6):
    ctx.accum_step(1)
    step.append(ctx.stats()["kernel_ms"])
dn = []
for _ in range(6):
    ctx.accum_denoise()
    dn.append(ctx.stats()["kernel_ms"])
print(f"one progressive step of 1 spp: {np.median(step[1:]):.3f} ms; the denoiser (defaults, G-buffer cached): {np.median(dn[1:]):.3f} ms", flush=True)
ctx.close()
