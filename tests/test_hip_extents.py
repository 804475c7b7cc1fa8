"""Device-pointer calls write their stated extents only, and read nothing that reaches a result from outside them.

include/spath_hip.h states every extent: n_rays*6 f32 of rays, n_rays i32 of source triangles, n_rays*4 u8 and n_rays*3 f32 of a
render's outputs, n_rays*3 f32 of a running sum, res_x*res_y*6 f32 of generated rays, 32 B per pixel of a G-buffer, w*h*3 f32, w*h f32
and w*h*4 u8 around the filter.  Each call here runs four times: once on separately allocated tensors, and three times with every input
and output carved out of ONE allocation with at least 4096 bytes of one byte value on each side of each region (0xff: a NaN as f32, -1
as i32; 0x00; 0xa5).  Afterwards every byte outside the regions still holds that value, and every output (and scans_executed, where
the call counts scans) equals the separately allocated run bit for bit: STATED TOLERANCE 0.  A store past an extent shows in a band; a
padding lane that reads past n_rays and lets the value reach an output, a count or the scan counter shows as a difference between
the runs, whose surroundings differ.

Counts: 1, 63, 64, 65, 255, 256, 257, 513, 1025, 1040 rays or pixels; variants 2, 15, 16 and SPHIP_FLAG_ACCEL; flags 0, NEE|MIS and the
widest pack (with the variants it is built for).

LIMITATION: a read past an extent whose value is masked out before it reaches any result is invisible to this test.  Nothing here
tries to provoke one."""
import numpy as np
import pytest

import hip_checks as hc
import history_model as hm
from hip_checks import _torch_first  # noqa: F401  (fixture)
from spath_amd import capi

pytestmark = pytest.mark.gpu

BAND = 4096
FILLS = (0xFF, 0x00, 0xA5)
FRAMES = {1: (1, 1), 63: (9, 7), 64: (8, 8), 65: (13, 5), 255: (15, 17), 256: (16, 16), 257: (257, 1), 513: (19, 27), 1025: (41, 25), 1040: (40, 26)}
SCANS = (2, 15, 16, hm.ACCEL)
PT_FLAGS = tuple(v | p for v in SCANS for p in (0, hm.NEE_MIS)) + (16 | hm.WIDEST, hm.ACCEL | hm.WIDEST)
SCENE = "room200"


@pytest.fixture(scope="module")
def ctx():
    """one context with the scene, every table, the map, the atlas, the normal map and a lens"""
    c = capi.Context(0)
    t, m = hm.scene_data(SCENE)
    c.set_scene(t, m)
    for table in hm.TABLES:
        c._set_table(hm.TABLE_SETTER[table], hm.table_data(table, SCENE))
    c.set_environment(hm.env_data("bright8"))
    c.set_texture(hm.atlas_data())
    c.set_normal_map(hm.nmap_data())
    c.set_lens(*hm.LENSES["wide"])
    yield c
    c.close()


class Separate:
    """every region a tensor of its own"""
    def __init__(self, inputs, outputs):
        import torch
        self.t = {k: torch.from_numpy(np.ascontiguousarray(v).view(np.uint8).ravel().copy()).to("cuda") for k, v in inputs.items()}
        self.t.update({k: torch.zeros(n, dtype=torch.uint8, device="cuda") for k, n in outputs.items()})

    def ptr(self, name):
        return self.t[name].data_ptr()

    def get(self, name):
        return self.t[name].cpu().numpy()

    def intact(self):
        return True


class Carved:
    """every region inside one allocation filled with one byte value; regions start on 256-byte boundaries, as separate allocations do,
    with at least BAND bytes of the fill before, between and behind them"""
    def __init__(self, inputs, outputs, fill):
        import torch
        self.fill, self.off, self.size = fill, {}, {}
        pos = BAND
        for k, n in list((k, np.ascontiguousarray(v).nbytes) for k, v in inputs.items()) + list(outputs.items()):
            self.off[k], self.size[k] = pos, n
            pos = (pos + n + BAND + 255) // 256 * 256
        self.buf = torch.full((pos,), fill, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 256 == 0
        for k, v in inputs.items():
            self.buf[self.off[k]:self.off[k] + self.size[k]] = torch.from_numpy(np.ascontiguousarray(v).view(np.uint8).ravel().copy()).to("cuda")

    def ptr(self, name):
        return self.buf.data_ptr() + self.off[name]

    def get(self, name):
        return self.buf[self.off[name]:self.off[name] + self.size[name]].cpu().numpy()

    def intact(self):
        h = self.buf.cpu().numpy()
        outside = np.ones(h.size, bool)
        for k in self.off:
            outside[self.off[k]:self.off[k] + self.size[k]] = False
        return bool((h[outside] == self.fill).all())


def held(ctx, fn, inputs, outputs, scans=False, what=""):
    """fn(ptr, stream) on separate tensors and on the three carvings: bands intact, outputs (and scans) equal"""
    import torch
    st = torch.cuda.current_stream().cuda_stream
    want = None
    for fill in (None,) + FILLS:
        mem = Separate(inputs, outputs) if fill is None else Carved(inputs, outputs, fill)
        torch.cuda.synchronize()
        try:
            fn(mem.ptr, st)
        except capi.SpathHipError as e:
            if "[-2]" in str(e):                                    # SPHIP_E_DEVICE: nothing more is started on the GPU in this session
                pytest.exit("device error in %s: %s" % (what, e), returncode=3)
            raise
        torch.cuda.synchronize()
        got = {k: mem.get(k) for k in outputs}
        if scans:
            got["scans"] = ctx.stats()["scans_executed"]
        assert mem.intact(), "%s: a byte outside the stated extents changed (fill 0x%02x)" % (what, fill)
        if want is None:
            want = got
            continue
        for k in want:
            assert np.array_equal(got[k], want[k]), "%s: output %s depends on what surrounds the buffers (fill 0x%02x)" % (what, k, fill)


def rays_of(n):
    return hc.cam_rays(*FRAMES[n], hm.MOVES)


@pytest.mark.parametrize("n", sorted(FRAMES))
def test_render_device(ctx, n):
    r = rays_of(n)[1]
    for flags in PT_FLAGS:
        for accum in (False, True):
            outs = {"rgba": n * 4, **({"accum": n * 12} if accum else {})}
            held(ctx, lambda p, st: ctx.render_device(p("rays"), n, 2, p("rgba"), seed=3, mode=capi.MODE_PT, flags=flags, image_width=FRAMES[n][0],
                                                      d_out_accum=p("accum") if accum else 0, stream=st),
                 {"rays": r}, outs, scans=True, what="render_device pt flags 0x%x accum %d" % (flags, accum))
    for flags in SCANS:
        held(ctx, lambda p, st: ctx.render_device(p("rays"), n, 1, p("rgba"), mode=capi.MODE_FLAT, flags=flags, image_width=FRAMES[n][0], stream=st),
             {"rays": r}, {"rgba": n * 4}, scans=True, what="render_device flat flags 0x%x" % flags)


@pytest.mark.parametrize("n", sorted(FRAMES))
def test_render_device_accum(ctx, n):
    r = rays_of(n)[1]

    def two_steps(flags):
        def fn(p, st):
            for base, cnt in ((0, 2), (2, 1)):                       # the first step ignores the sum's contents, the second adds to them
                ctx.render_device_accum(p("rays"), n, base, cnt, p("sum"), p("rgba"), seed=3, flags=flags, image_width=FRAMES[n][0], d_out_mean=p("mean"), stream=st)
        return fn
    for flags in PT_FLAGS:
        held(ctx, two_steps(flags), {"rays": r}, {"sum": n * 12, "rgba": n * 4, "mean": n * 12}, scans=True, what="render_device_accum flags 0x%x" % flags)


@pytest.mark.parametrize("n", sorted(FRAMES))
def test_closest_hit_device(ctx, n):
    r = rays_of(n)[1]
    k = np.arange(n)
    src = np.where(k % 3 == 0, -1, (k * 7) % hm.SCENE_TRIS[SCENE]).astype(np.int32)
    for flags in SCANS:
        held(ctx, lambda p, st: ctx.closest_hit_device(p("rays"), n, p("idx"), p("dist"), flags=flags, stream=st),
             {"rays": r}, {"idx": n * 4, "dist": n * 4}, scans=True, what="closest_hit_device flags 0x%x" % flags)
        held(ctx, lambda p, st: ctx.closest_hit_device(p("rays"), n, p("idx"), p("dist"), d_src_idx=p("src"), flags=flags, stream=st),
             {"rays": r, "src": src}, {"idx": n * 4, "dist": n * 4}, scans=True, what="closest_hit_device with d_src_idx flags 0x%x" % flags)


@pytest.mark.parametrize("n", sorted(FRAMES))
def test_viewport_and_camera_rays_device(ctx, n):
    cam = rays_of(n)[0]
    held(ctx, lambda p, st: ctx.viewport_device(cam, p("rays"), stream=st), {}, {"rays": n * 24}, what="viewport_device")
    for sample in (0, 5):
        held(ctx, lambda p, st: ctx.camera_rays_device(cam, sample, p("rays"), seed=11, stream=st), {}, {"rays": n * 24}, what="camera_rays_device")


@pytest.mark.parametrize("n", sorted(FRAMES))
def test_gbuffer_and_denoise_device(ctx, n):
    import torch
    w, h = FRAMES[n]
    r = rays_of(n)[1]
    for flags in SCANS + (hm.SMOOTH | hm.NMAP | 16, hm.SMOOTH | hm.NMAP | hm.ACCEL):
        held(ctx, lambda p, st: ctx.gbuffer_device(p("rays"), n, p("gbuf"), flags=flags, stream=st), {"rays": r}, {"gbuf": n * 32},
             what="gbuffer_device flags 0x%x" % flags)
    d_rays = torch.from_numpy(r).to("cuda")
    d_g = torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
    ctx.gbuffer_device(d_rays.data_ptr(), n, d_g.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    g = d_g.cpu().numpy()
    rng = np.random.default_rng(n)
    mean, var = rng.random((n, 3)).astype(np.float32), (rng.random(n) * 0.05).astype(np.float32)
    held(ctx, lambda p, st: ctx.denoise_device(w, h, p("mean"), p("gbuf"), p("rgba"), d_var=p("var"), d_out_rgb=p("rgb"), stream=st),
         {"mean": mean, "var": var, "gbuf": g}, {"rgba": n * 4, "rgb": n * 12}, what="denoise_device with variance")
    held(ctx, lambda p, st: ctx.denoise_device(w, h, p("mean"), p("gbuf"), p("rgba"), stream=st),
         {"mean": mean, "gbuf": g}, {"rgba": n * 4}, what="denoise_device without variance or rgb")
