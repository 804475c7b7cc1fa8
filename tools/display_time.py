"""What the display transform costs at 1920x1080: the luminance histogram (sphip_luminance_histogram_device) on a
rendered mean, on a CONSTANT image (every lane of every wave in one bin: what the aggregation in k_lum_histogram is for) and on a noise
image (log-uniform over 21 octaves: about 170 bins in use); the transform (sphip_display_device) for every curve with the sRGB encoding,
without and with the float output, beside a device-to-device copy of the same number of bytes, which is the yardstick of a kernel bound
by memory (12 B in, 4 B or 16 B out per pixel); and the blocking sphip_accum_display, metered and not, by the wall clock (it reads the
image back).  Times are device events around BATCH back-to-back calls on one stream, divided by BATCH; the median of REPS such windows
after a warm-up, with the spread (min .. max).  Every device-pointer figure is taken twice: "cache" calls the same buffers every time, so
a frame of 25 to 58 MB stays in the 256 MB last-level cache and the rate is the cache's, not HBM's; "hbm" rotates over as many sets of
buffers as make SPAN bytes, several times the cache, so every call finds its frame in HBM -- the case of a transform that follows a
render step.  Rates are the bytes the operation needs once over the time; only the "hbm" ones may be held against the 8 TB/s HBM peak.
Writes what it prints to profiles/display.log (or the file named).
python tools/display_time.py [LOG]"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from spath_amd import capi, scene, view

nt, w, h = 10000, 1920, 1080
n = w * h
BATCH, REPS, WARM = 200, 11, 2
SPAN = 1 << 30                    # bytes the rotating buffer sets cover: four times the last-level cache
log = open(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "display.log"), "w")


def say(s):
    print(s, flush=True)
    log.write(s + "\n")
    log.flush()


ctx = capi.Context(0)
t, m = scene.closed_room(nt)
ctx.set_scene(t, m)
say(f"library {capi.build_source_hash()}, {ctx.description}; closed_room({nt}) {w}x{h}")
dev = torch.device("cuda:0")
st = torch.cuda.current_stream().cuda_stream


def window(fn):
    """median, min, max over REPS windows of BATCH calls, in ms per call"""
    ms = []
    for rep in range(WARM + REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(BATCH):
            fn(i)
        e1.record()
        e1.synchronize()
        if rep >= WARM:
            ms.append(e0.elapsed_time(e1) / BATCH)
    return float(np.median(ms)), min(ms), max(ms)


def rate(nbytes, ms, hbm):
    gbs = nbytes / (ms * 1e-3) / 1e9
    return f"{gbs:.0f} GB/s" + (f" ({gbs / 8000 * 100:.1f} % of the 8 TB/s HBM peak)" if hbm else " (cache-resident)")


def sets(nbytes_per_set, hbm):
    """how many sets of buffers the calls rotate over"""
    return max(2, -(-SPAN // int(nbytes_per_set))) if hbm else 1


cam = view.Camera(w, h)
ctx.accum_begin(cam=cam, seed=1)
_, mean, _ = ctx.accum_step(4, want_mean=True)
rng = np.random.default_rng(1)
images = {"rendered mean (4 spp)": mean,
          "constant image": np.tile(np.float32((0.5, 0.25, 2.0)), (n, 1)),
          "noise image": (2.0 ** rng.uniform(-14, 7, (n, 3))).astype(np.float32)}
d_hist = torch.zeros(capi.LUM_BINS, dtype=torch.int32, device=dev)
hist_ms = {}
for name, img in images.items():
    for hbm in (False, True):
        k = sets(12.0 * n, hbm)
        d_imgs = [torch.from_numpy(np.ascontiguousarray(img)).to(dev) for _ in range(k)]
        r = window(lambda i: ctx.luminance_histogram_device(n, d_imgs[i % k].data_ptr(), d_hist.data_ptr(), st))
        torch.cuda.synchronize()
        hh = d_hist.cpu().numpy().view(np.uint32)
        assert int(hh.sum()) == n
        hist_ms[name, hbm] = r[0]
        say(f"histogram, {name}, {'hbm' if hbm else 'cache'} ({k} image{'s' if k > 1 else ''}): {r[0]:.4f} ms ({r[1]:.4f} .. {r[2]:.4f}); "
            f"{int((hh > 0).sum())} bins in use, the fullest holds {100.0 * hh.max() / n:.1f} % of the pixels; 12 B/pixel read -> {rate(12.0 * n, r[0], hbm)}")
        del d_imgs
for hbm in (False, True):
    say(f"histogram, constant over noise, {'hbm' if hbm else 'cache'}: {hist_ms['constant image', hbm] / hist_ms['noise image', hbm]:.2f}")

for with_rgb, nbytes in ((False, 16.0 * n), (True, 28.0 * n)):
    for hbm in (False, True):
        k = sets(nbytes, hbm)
        where = f"{'hbm' if hbm else 'cache'} ({k} set{'s' if k > 1 else ''} of buffers)"
        # the yardstick: a device-to-device copy that moves as many bytes (half of them read, half written)
        src = [torch.zeros(int(nbytes) // 2, dtype=torch.uint8, device=dev) for _ in range(k)]
        dst = [torch.zeros(int(nbytes) // 2, dtype=torch.uint8, device=dev) for _ in range(k)]
        c = window(lambda i: dst[i % k].copy_(src[i % k]))
        say(f"-- RGBA8{' + float' if with_rgb else ''}, {where}: {nbytes / n:.0f} B/pixel moved; a device-to-device copy of as many bytes: {c[0]:.4f} ms "
            f"({c[1]:.4f} .. {c[2]:.4f}) -> {rate(nbytes, c[0], hbm)}")
        del src, dst
        d_mean = [torch.from_numpy(np.ascontiguousarray(mean)).to(dev) for _ in range(k)]
        d_rgba = [torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(k)]
        d_rgb = [torch.zeros(n * 3 if with_rgb else 1, dtype=torch.float32, device=dev) for _ in range(k)]
        for curve in ("clamp", "reinhard", "filmic"):
            for enc in ("linear", "srgb"):
                p = capi.Display.make({"curve": curve, "encode": enc, "exposure": 0.8})
                r = window(lambda i: ctx.display_device(n, d_mean[i % k].data_ptr(), d_rgba[i % k].data_ptr(),
                                                        d_out_rgb=d_rgb[i % k].data_ptr() if with_rgb else 0, params=p, stream=st))
                say(f"transform {curve:8s} {enc:6s} {'hbm' if hbm else 'cache':5s}: {r[0]:.4f} ms ({r[1]:.4f} .. {r[2]:.4f}) -> {rate(nbytes, r[0], hbm)}; "
                    f"{r[0] / c[0]:.2f} x the copy")
        del d_mean, d_rgba, d_rgb
        torch.cuda.empty_cache()

# the blocking call on the accumulation above: wall clock, the read-back of the image (8.3 MB) included; the library's kernel clock beside it
for name, kw in (("exposure given", {}), ("metered", {"metering": True}), ("metered, denoised (defaults, G-buffer cached)", {"metering": True, "denoise": True})):
    wall, kern = [], []
    for i in range(7):
        t0 = time.perf_counter()
        _, e = ctx.accum_display(**kw)
        wall.append((time.perf_counter() - t0) * 1e3)
        kern.append(ctx.stats()["kernel_ms"])
    say(f"sphip_accum_display, {name}: wall {np.median(wall[1:]):.3f} ms ({min(wall[1:]):.3f} .. {max(wall[1:]):.3f}), kernels {np.median(kern[1:]):.3f} ms; "
        f"exposure {e:.6g}")
ctx.close()
log.close()
