"""Python mirror of the reference's renderer plugin interface for the HIP backend.

`Renderer` has the eight virtuals of scene::renderer (reference src/renderer.h:24-36);
`BasicRenderer` supplies the five camera ones exactly as basic_renderer does for every backend
(reference src/basic_renderer.h:25-54); `HipRenderer` implements get_description / render_flat /
render on top of the C ABI (include/spath_hip.h), i.e. it is the Python twin of the C++ adapter
spath_amd/host/hip_renderer.cpp.  `get(w, h)` mirrors the per-backend factory
`X_renderer::get(w, h)` (reference src/cpu_renderer.h:23-25).

Argument meaning and error behaviour follow the reference: render calls are synchronous, borrow
the caller's arrays only for the duration of the call, size the output bitmap themselves
(cpu_renderer.cpp:120-122) and raise (the reference throws std::runtime_error) on device failure.
"""
from __future__ import annotations

import numpy as np

from . import capi
from .view import Camera


NEVER_STOP = (0.0, 0.0, 0xFFFFFFFF)    # an adaptive rule that never stops a pixel (min_samples = UINT32_MAX)
# What HipRenderer keeps beside the triangles and sends with every scene upload, in upload order: (name, floats per triangle or None for a
# context-level image, the flag of a path-traced frame, the capi.Context setter).  A flag is on while everything that lists it is set.
PARTS = (
    ("spec", 4, capi.FLAG_SPECULAR, "set_specular"),
    ("vnorm", 9, capi.FLAG_SMOOTH, "set_vertex_normals"),
    ("glass", 4, capi.FLAG_DIELECTRIC, "set_dielectric"),
    ("rough", 1, capi.FLAG_GLOSSY, "set_roughness"),
    ("uv", 6, capi.FLAG_TEXTURE | capi.FLAG_NORMAL_MAP, "set_uv"),         # the one UV table addresses the atlas and the normal map
    ("env", None, capi.FLAG_ENVIRONMENT, "set_environment"),
    ("tex", None, capi.FLAG_TEXTURE, "set_texture"),
    ("nmap", None, capi.FLAG_NORMAL_MAP, "set_normal_map"),
)


class Bitmap:
    """scene::bitmap (reference src/scene.h:41-45): res_x, res_y, values[res_x*res_y] RGBA8."""

    def __init__(self):
        self.res_x = 0
        self.res_y = 0
        self.values = np.zeros((0, 4), dtype=np.uint8)

    def image(self) -> np.ndarray:
        return self.values.reshape(self.res_y, self.res_x, 4)


class Viewport:
    """view::viewport (reference src/view.h:28-31): res_x, res_y, rays[res_x*res_y]."""

    def __init__(self, res_x=0, res_y=0, rays=None):
        self.res_x, self.res_y = res_x, res_y
        self.rays = rays if rays is not None else np.zeros((0, 6), dtype=np.float32)


class Renderer:
    """scene::renderer (reference src/renderer.h:24-36)."""

    def get_description(self) -> str: raise NotImplementedError
    def set_viewport_size(self, w: int, h: int): raise NotImplementedError
    def set_delta_mov(self, m): raise NotImplementedError
    def set_delta_rot(self, r): raise NotImplementedError
    def set_delta_focal(self, f: float): raise NotImplementedError
    def get_viewport(self, vp: Viewport): raise NotImplementedError
    def render_flat(self, vp, tris, mats, n_tris, n_samples, out: Bitmap): raise NotImplementedError
    def render(self, vp, tris, mats, n_tris, n_samples, out: Bitmap): raise NotImplementedError


class BasicRenderer(Renderer):
    """basic_renderer (reference src/basic_renderer.h:25-54): owns the camera."""

    def __init__(self, x: int, y: int):
        self.vc = Camera(x, y)

    def set_viewport_size(self, w, h): self.vc.set_viewport_size(w, h)
    def set_delta_mov(self, m): self.vc.set_delta_mov(m)
    def set_delta_rot(self, r): self.vc.set_delta_rot(r)
    def set_delta_focal(self, f): self.vc.set_delta_focal(f)

    def get_viewport(self, vp: Viewport):
        vp.res_x, vp.res_y = self.vc.res_x, self.vc.res_y
        vp.rays = self.vc.get_viewport()


class HipRenderer(BasicRenderer):
    """The MI355X backend behind the reference's plugin interface."""

    def __init__(self, x: int, y: int, device: int = 0, seed: int = 1, flags: int = 0, progressive: bool = False, adaptive=None,
                 denoise=False):
        super().__init__(x, y)
        self.ctx = capi.Context(device)      # raises like cl_r/vk_r constructors do on init failure
        self.seed = seed
        self.flags = flags
        # progressive=True: render() / render_own_viewport() add their n_samples to those of the previous calls while the
        # viewport rays (bit for bit) or the camera, the scene, the seed and the flags stay the same, and return the image of all
        # of them (bit-identical to one render of the sum); any change begins a new accumulation.  render_flat is not accumulated.
        self.progressive = progressive
        # adaptive=(t, floor, min_samples) with progressive=True: converged pixels stop (capi.Context.accum_begin); part of the
        # accumulation's key, so changing it begins anew.  adaptive_counts() gives the per-pixel sample counts.
        if adaptive is not None and not progressive:
            raise ValueError("adaptive sampling needs progressive=True")
        self.adaptive = tuple(adaptive) if adaptive is not None else None
        # denoise=True (the library's defaults) or a dict of capi.Denoise fields, with progressive=True: the bitmap of every
        # progressive step is the accumulation denoised (capi.Context.accum_denoise); the raw image stays in raw_bitmap.  Without
        # an adaptive rule the accumulation is begun with one that never stops a pixel, so that the filter has the variance; its
        # raw image is bit-identical to a plain accumulation's.
        if denoise is not False and denoise is not None and not progressive:
            raise ValueError("denoising needs progressive=True")
        self.denoise = None if denoise is False or denoise is None else capi.Denoise.make(None if denoise is True else denoise)
        self.raw_bitmap = Bitmap()
        self.reproject = None                                  # set_reproject
        self.display = None                                    # set_display: (capi.Display, capi.Metering or None)
        self.display_exposure = 1.0                            # the exposure the last progressive step was shown with
        self._moves = 0
        self._scene_key = None
        self._accum_key = None
        self.last_stats = None
        self._parts = {name: None for name, _, _, _ in PARTS}

    def _set_part(self, name, data):
        """keep a copy of a table ([n_tris, floats]) or an image (as given), or None; the next frame uploads the scene again"""
        floats = next(p[1] for p in PARTS if p[0] == name)
        if data is not None:
            data = np.ascontiguousarray(data, dtype=np.float32)
            data = (data if floats is None else data.reshape(-1, floats)).copy()
        self._parts[name] = data
        self._scene_key = None

    def set_texture(self, texels):
        """The atlas of capi.FLAG_TEXTURE renders ([th, tw, 3] float32, scene.checker_texture; None: no atlas), like
        hip_renderer::set_texture: it goes to the library with the next scene upload and begins a new accumulation, and while an atlas
        and a UV table (set_uv) are both set every path-traced frame carries capi.FLAG_TEXTURE (render_flat never does)."""
        self._set_part("tex", texels)

    def set_normal_map(self, texels):
        """The normal map of capi.FLAG_NORMAL_MAP renders ([nh, nw, 3] float32 of signed tangent-space vectors,
        scene.normal_map_from_height or scene.decode_normal_map; None: no map), like hip_renderer::set_normal_map: it goes to the
        library with the next scene upload and begins a new accumulation, and while a map and a UV table (set_uv) are both set every
        path-traced frame carries capi.FLAG_NORMAL_MAP (render_flat never does)."""
        self._set_part("nmap", texels)

    def set_uv(self, uv):
        """The UV table of capi.FLAG_TEXTURE and capi.FLAG_NORMAL_MAP renders ([n_tris, 6] float32, scene.uv_table or scene.planar_uv; None: no table), like
        hip_renderer::set_uv: see set_texture."""
        self._set_part("uv", uv)

    def set_roughness(self, alpha):
        """The roughness table of capi.FLAG_GLOSSY renders ([n_tris] float32, scene.roughness_table; None: no table), like
        hip_renderer::set_roughness: it goes to the library with the next scene upload and begins a new accumulation, and while one is
        set every path-traced frame carries capi.FLAG_GLOSSY (render_flat never does); the flag needs a specular table beside it."""
        self._set_part("rough", alpha)

    def set_environment(self, env):
        """The environment map of capi.FLAG_ENVIRONMENT renders ([n, n, 3] float32, scene.sky_environment or
        scene.environment_from_latlong; None: no map), like hip_renderer::set_environment: it goes to the library with the next scene
        upload and begins a new accumulation, and while one is set every path-traced frame carries capi.FLAG_ENVIRONMENT (render_flat
        never does)."""
        self._set_part("env", env)

    def set_dielectric(self, glass):
        """The dielectric table of capi.FLAG_DIELECTRIC renders ([n_tris, 4] float32, scene.dielectric_table; None: no table), like
        hip_renderer::set_dielectric: it goes to the library with the next scene upload and begins a new accumulation, and while one
        is set every path-traced frame carries capi.FLAG_DIELECTRIC (render_flat never does)."""
        self._set_part("glass", glass)

    def set_vertex_normals(self, vn):
        """The per-vertex normals of capi.FLAG_SMOOTH renders ([n_tris, 9] float32, scene.vertex_normals; None: none), like
        hip_renderer::set_vertex_normals: they go to the library with the next scene upload and begin a new accumulation, and while
        they are set every path-traced frame carries capi.FLAG_SMOOTH (render_flat never does)."""
        self._set_part("vnorm", vn)

    def set_specular(self, spec):
        """The specular table of capi.FLAG_SPECULAR renders ([n_tris, 4] float32, scene.specular_table; None: no table), like
        hip_renderer::set_specular: it goes to the library with the next scene upload and begins a new accumulation, and while one is
        set every path-traced frame carries capi.FLAG_SPECULAR (render_flat never does).  Without a table the flags are the caller's."""
        self._set_part("spec", spec)

    def set_reproject(self, params=True):
        """Temporal reprojection of the progressive mode, like hip_renderer::set_reproject: with params True (the library's defaults), a
        capi.Reproject, a (max_history, normal_min, plane_tol) tuple or a dict of its fields, a camera move (set_delta_mov /
        set_delta_rot / set_delta_focal) between two render_own_viewport frames no longer begins a new accumulation: the old view's
        accumulation is reprojected into the new view (capi.Context.accum_reproject) and blended with its samples, drawn under seed +
        the number of moves reprojected so far.  Every other cause still begins anew: a scene, table or image change, a resize, the
        seed, the flags, and render() (the caller's rays carry no camera).  With denoising on, the accumulation is plain and the
        filter runs without the variance.  Refused with the library's message while an adaptive rule is set.  None or False: off."""
        if params is None or params is False:
            self.reproject = None
            return
        if not self.progressive:
            raise ValueError("temporal reprojection needs progressive=True")
        if self.adaptive is not None:
            raise capi.SpathHipError("sphip_accum_reproject failed [-3]: sphip_accum_reproject needs a plain accumulation, not an adaptive one")
        self.reproject = capi.Reproject.make(None if params is True else params)

    def set_display(self, params=True, metering=None):
        """The display transform of the progressive mode, like hip_renderer::set_display: with params True (the library's defaults:
        filmic, sRGB, exposure 1), a capi.Display or a dict of its fields, the bitmap of every progressive step goes through exposure,
        tone curve and encoding (capi.Context.accum_display) instead of the linear clamp; metering True (the library's key and
        window), a capi.Metering, a (key, low, high) tuple or a dict: the exposure is metered from each step's image and kept in
        display_exposure.  Composes with denoising (the filtered image is metered and shown; raw_bitmap stays the clamp-only raw
        image) and with set_reproject.  A post-process: it never begins a new accumulation.  None or False: off."""
        if params is None or params is False:
            self.display = None
            return
        if not self.progressive:
            raise ValueError("the display transform needs progressive=True")
        m = None if metering is None or metering is False else capi.Metering.make(None if metering is True else metering)
        self.display = (capi.Display.make(None if params is True else params), m)

    def _flags(self, mode):
        """the flags word of a frame: FLAG_SPECULAR, FLAG_SMOOTH, FLAG_DIELECTRIC, FLAG_ENVIRONMENT, FLAG_GLOSSY, FLAG_TEXTURE and
        FLAG_NORMAL_MAP on while their tables, the maps or the atlas are set, and never on the flat pass"""
        on = off = 0
        for name, _, flag, _ in PARTS:
            if self._parts[name] is None:
                off |= flag
            else:
                on |= flag
        if mode == capi.MODE_FLAT:
            return self.flags & ~(on | off)
        return self.flags | (on & ~off)

    def get_description(self) -> str:
        return self.ctx.description

    def _upload_scene(self, tris, mats, n_tris):
        tris = np.ascontiguousarray(tris, dtype=np.float32).reshape(-1, 12)[:n_tris]
        mats = np.ascontiguousarray(mats, dtype=np.float32).reshape(-1, 6)[:n_tris]
        # the reference's GPU peer re-uploads every frame (cl_renderer.cpp:210-214); upload only on change
        key = (n_tris, hash(tris.tobytes()), hash(mats.tobytes())) + tuple(None if a is None else (a.shape, hash(a.tobytes()))
                                                                           for a in self._parts.values())
        if key != self._scene_key:
            self.ctx.set_scene(tris, mats)
            for name, floats, _, setter in PARTS:
                a = self._parts[name]
                if floats is None:
                    getattr(self.ctx, setter)(a)               # an image is the context's: sent, or cleared, every time
                elif a is not None:
                    getattr(self.ctx, setter)(a[:n_tris])
            self._scene_key = key

    def _begin_rule(self):
        if self.adaptive is None and self.denoise is not None and self.reproject is None:
            return NEVER_STOP
        return self.adaptive

    def _accum_step(self, key, begin, n_samples, out, move=None):
        if self.denoise is not None:
            key = key + ("denoise", self.reproject is not None)   # the rule it begins with; the parameters apply to any step
        if key != self._accum_key:
            old, self._accum_key = self._accum_key, None
            # move: only the camera (key[1], at an unchanged resolution) differs from the live accumulation's key
            if move is not None and old is not None and old[0] == key[0] == "cam" and old[2:] == key[2:]:
                move()
            else:
                begin()
            self._accum_key = key
        try:
            out.values, _ = self.ctx.accum_step(n_samples)
        except capi.SpathHipError:
            self._accum_key = None                             # a failed step ends the accumulation in the library too
            raise
        self.last_stats = self.ctx.stats()
        if self.denoise is not None:
            self.raw_bitmap.res_x, self.raw_bitmap.res_y, self.raw_bitmap.values = out.res_x, out.res_y, out.values
        if self.display is not None:
            out.values, self.display_exposure = self.ctx.accum_display(self.display[0], metering=self.display[1], denoise=self.denoise)
        elif self.denoise is not None:
            out.values = self.ctx.accum_denoise(self.denoise)

    def _render(self, vp, tris, mats, n_tris, n_samples, out, mode):
        self._upload_scene(tris, mats, n_tris)
        out.res_x, out.res_y = vp.res_x, vp.res_y          # cpu_renderer.cpp:120-122
        if self.progressive and mode == capi.MODE_PT:
            rays = np.ascontiguousarray(vp.rays, dtype=np.float32).reshape(-1, 6)
            flags = self._flags(mode)
            key = ("rays", vp.res_x, vp.res_y, rays.tobytes(), self._scene_key, self.seed, flags, self.adaptive)
            self._accum_step(key, lambda: self.ctx.accum_begin(rays=rays, w=vp.res_x, h=vp.res_y, seed=self.seed, flags=flags,
                                                               adaptive=self._begin_rule()),
                             n_samples, out)
            return
        flags = self._flags(mode)                                                               # the flat pass has no materials to mirror
        out.values = self.ctx.render(vp.rays, vp.res_x, vp.res_y, n_samples, seed=self.seed, mode=mode, flags=flags)
        self.last_stats = self.ctx.stats()

    def render_flat(self, vp, tris, mats, n_tris, n_samples, out):
        self._render(vp, tris, mats, n_tris, max(int(n_samples), 1), out, capi.MODE_FLAT)

    def render(self, vp, tris, mats, n_tris, n_samples, out):
        self._render(vp, tris, mats, n_tris, n_samples, out, capi.MODE_PT)

    def render_own_viewport(self, tris, mats, n_tris, n_samples, out: Bitmap, flat: bool = False):
        """get_viewport + render(_flat) without moving rays over PCIe: the viewport is generated on the device
        from this renderer's own camera (bit-identical to get_viewport)."""
        self._upload_scene(tris, mats, n_tris)
        out.res_x, out.res_y = self.vc.res_x, self.vc.res_y
        if self.progressive and not flat:
            ca = capi.CameraArgs.from_camera(self.vc)
            flags = self._flags(capi.MODE_PT)
            key = ("cam", bytes(ca), (ca.res_x, ca.res_y), self._scene_key, self.seed, flags, self.adaptive)

            def move():
                self._moves += 1
                self.ctx.accum_reproject(self.vc, self.seed + self._moves, self.reproject)
            self._accum_step(key, lambda: self.ctx.accum_begin(cam=self.vc, seed=self.seed, flags=flags, adaptive=self._begin_rule()),
                             max(int(n_samples), 1), out, move if self.reproject is not None and self.adaptive is None else None)
            return
        out.values = self.ctx.render_camera(self.vc, max(int(n_samples), 1), seed=self.seed, mode=capi.MODE_FLAT if flat else capi.MODE_PT,
                                            flags=self._flags(capi.MODE_FLAT if flat else capi.MODE_PT))
        self.last_stats = self.ctx.stats()

    def adaptive_counts(self):
        """(counts[h, w], n_active) of the current accumulation (capi.Context.accum_counts)."""
        return self.ctx.accum_counts()

    def close(self):
        self.ctx.close()


def get(w: int, h: int, **kw) -> Renderer:
    """hip_renderer::get(w, h) -- peer of cpu_renderer::get (reference src/cpu_renderer.cpp:205-209)."""
    return HipRenderer(w, h, **kw)
