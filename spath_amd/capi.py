"""ctypes binding of the C ABI in include/spath_hip.h (libspath_hip.so).

This is the only way Python reaches the HIP kernels.  There is no CPU fallback: if the shared
library is missing or the GPU cannot be initialised the calls raise.
"""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libspath_hip.so")

MODE_FLAT = 0
MODE_PT = 1
KERNEL_AUTO = 0
FLAG_PRIMARY_REUSE = 0x100
FLAG_ACCEL = 0x200          # opt-in linear BVH; not the brute-force path
FLAG_NEE = 0x400            # opt-in next-event estimation: light sampling with shadow rays
FLAG_MIS = 0x800            # with FLAG_NEE: multiple importance sampling of its light samples
FLAG_CAMERA_SAMPLES = 0x1000  # per-sample camera rays on the camera paths: pixel antialiasing, thin lens
FLAG_SPECULAR = 0x2000      # mirror and mixed diffuse/mirror materials from the context's specular table
FLAG_SMOOTH = 0x4000        # smooth shading by the context's per-vertex normals
FLAG_DIELECTRIC = 0x8000    # transparency: glass triangles from the context's dielectric table
FLAG_ENVIRONMENT = 0x1000000  # environment lighting by the context's octahedral map
FLAG_GLOSSY = 0x2000000     # with FLAG_SPECULAR: the mirror lobe roughened by the context's roughness table
FLAG_TEXTURE = 0x4000000    # textures: the diffuse reflectance scaled by the context's atlas at the hit's UV
FLAG_NORMAL_MAP = 0x8000000  # normal mapping: the shading normal from the context's normal map at the hit's UV


def flag_chunks(n: int) -> int:
    """flags bits 16..23: number of sample chunks of a path-traced launch (0 = library's choice, 1 = never split)."""
    if not 0 <= n <= 255:
        raise ValueError("chunks must be in [0, 255]")
    return n << 16

# every entry point include/spath_hip.h declares (checked by tests/test_capi_symbols.py)
SYMBOLS = (
    "sphip_create", "sphip_destroy", "sphip_last_error", "sphip_description", "sphip_abi_version",
    "sphip_kernel_name", "sphip_set_scene", "sphip_render", "sphip_set_scene_device",
    "sphip_render_device", "sphip_closest_hit_device", "sphip_get_stats", "sphip_viewport_device", "sphip_render_camera",
    "sphip_create_multi", "sphip_device_count", "sphip_plan_tile_rows", "sphip_plan_shard", "sphip_selftest_device",
    "sphip_kernel_available", "sphip_selftest_stage1", "sphip_selftest_retest", "sphip_build_info",
    "sphip_selftest_sort", "sphip_selftest_bvh_dump", "sphip_selftest_bvh_walk",
    "sphip_render_device_accum", "sphip_accum_begin", "sphip_accum_step",
    "sphip_accum_begin_adaptive", "sphip_accum_counts",
    "sphip_denoise_defaults", "sphip_gbuffer_device", "sphip_denoise_device", "sphip_accum_gbuffer", "sphip_accum_denoise",
    "sphip_reproject_defaults", "sphip_reproject_device", "sphip_temporal_resolve_device", "sphip_accum_reproject", "sphip_accum_history",
    "sphip_display_defaults", "sphip_metering_defaults", "sphip_srgb_thresholds", "sphip_luminance_histogram_device",
    "sphip_exposure_from_histogram", "sphip_display_device", "sphip_accum_display",
    "sphip_set_lens", "sphip_camera_rays_device",
    "sphip_set_specular", "sphip_set_specular_device",
    "sphip_set_vertex_normals", "sphip_set_vertex_normals_device",
    "sphip_set_dielectric", "sphip_set_dielectric_device",
    "sphip_set_environment", "sphip_set_environment_device", "sphip_selftest_env_dump",
    "sphip_set_roughness", "sphip_set_roughness_device",
    "sphip_set_texture", "sphip_set_texture_device", "sphip_set_uv", "sphip_set_uv_device",
    "sphip_set_normal_map", "sphip_set_normal_map_device",
)
GATHER_NONE, GATHER_RCCL, GATHER_PEER = 0, 1, 2
# the per-triangle tables of a scene: (the X of sphip_set_X and sphip_set_X_device, floats per triangle, the ValueError of a table
# whose rows are not the scene's triangles)
TRI_TABLES = (
    ("specular", 4, "one specular row per triangle of the scene"),
    ("vertex_normals", 9, "one row of vertex normals per triangle of the scene"),
    ("dielectric", 4, "one dielectric row per triangle of the scene"),
    ("roughness", 1, "one roughness value per triangle of the scene"),
    ("uv", 6, "one UV row per triangle of the scene"),
)


class Shard(C.Structure):
    _fields_ = [("pixel_base", C.c_uint64), ("tile_px", C.c_uint64), ("tile_stride_px", C.c_uint64)]


class CameraArgs(C.Structure):
    """sphip_camera: view::camera state with the trig values the reference computes on the host (view.h:77-80)."""
    _fields_ = [("pos", C.c_float * 3), ("cos_y", C.c_float), ("sin_y", C.c_float), ("cos_x", C.c_float), ("sin_x", C.c_float),
                ("focal", C.c_float), ("res_x", C.c_uint32), ("res_y", C.c_uint32)]

    @classmethod
    def from_camera(cls, cam):
        """cam: spath_amd.view.Camera"""
        return cls((C.c_float * 3)(*[float(x) for x in cam.pos]), float(cam.cosY), float(cam.sinY), float(cam.cosX), float(cam.sinX),
                   float(cam.focal), int(cam.res_x), int(cam.res_y))


class Lens(C.Structure):
    """sphip_lens: the thin lens of camera samples (include/spath_hip.h)."""
    _fields_ = [("aperture", C.c_float), ("focus_dist", C.c_float), ("reserved", C.c_uint32)]


class Adaptive(C.Structure):
    """sphip_adaptive: the convergence rule of an adaptive accumulation (include/spath_hip.h)."""
    _fields_ = [("rel_error", C.c_double), ("floor", C.c_double), ("min_samples", C.c_uint32), ("reserved", C.c_uint32)]


class Denoise(C.Structure):
    """sphip_denoise: parameters of the a-trous denoiser (include/spath_hip.h)."""
    _fields_ = [("iterations", C.c_uint32), ("normal_log2", C.c_uint32), ("sigma_depth", C.c_float), ("sigma_lum", C.c_float),
                ("reserved", C.c_uint32 * 2)]

    @classmethod
    def defaults(cls):
        d = cls()
        load().sphip_denoise_defaults(C.byref(d))
        return d

    @classmethod
    def make(cls, params=None):
        """None: the library's defaults; a Denoise as is; a dict overrides some of the defaults
        (iterations, normal_log2, sigma_depth, sigma_lum)."""
        if isinstance(params, cls):
            return params
        d = cls.defaults()
        for k, v in (params or {}).items():
            if k not in ("iterations", "normal_log2", "sigma_depth", "sigma_lum"):
                raise ValueError(f"unknown denoise parameter {k!r}")
            setattr(d, k, v)
        return d

    def as_dict(self):
        return {"iterations": self.iterations, "normal_log2": self.normal_log2, "sigma_depth": self.sigma_depth, "sigma_lum": self.sigma_lum}


class Reproject(C.Structure):
    """sphip_reproject: parameters of temporal reprojection (include/spath_hip.h)."""
    _fields_ = [("max_history", C.c_float), ("normal_min", C.c_float), ("plane_tol", C.c_float), ("reserved", C.c_uint32)]

    @classmethod
    def defaults(cls):
        d = cls()
        load().sphip_reproject_defaults(C.byref(d))
        return d

    @classmethod
    def make(cls, params=None):
        """None: the library's defaults; a Reproject as is; a (max_history, normal_min, plane_tol) tuple; a dict overrides some of
        the defaults."""
        if isinstance(params, cls):
            return params
        if isinstance(params, (tuple, list)):
            return cls(*[float(x) for x in params], 0)
        d = cls.defaults()
        for k, v in (params or {}).items():
            if k not in ("max_history", "normal_min", "plane_tol", "reserved"):
                raise ValueError(f"unknown reproject parameter {k!r}")
            setattr(d, k, v)
        return d

    def as_dict(self):
        return {"max_history": self.max_history, "normal_min": self.normal_min, "plane_tol": self.plane_tol}


CURVE_CLAMP, CURVE_REINHARD, CURVE_FILMIC = 0, 1, 2
ENCODE_LINEAR, ENCODE_SRGB = 0, 1
CURVES = {"clamp": CURVE_CLAMP, "reinhard": CURVE_REINHARD, "filmic": CURVE_FILMIC}
LUM_BINS = 2048


class Display(C.Structure):
    """sphip_display: exposure, tone curve and encoding of the display transform (include/spath_hip.h)."""
    _fields_ = [("exposure", C.c_float), ("white", C.c_float), ("curve", C.c_uint32), ("encode", C.c_uint32), ("reserved", C.c_uint32 * 2)]

    @classmethod
    def defaults(cls):
        d = cls()
        load().sphip_display_defaults(C.byref(d))
        return d

    @classmethod
    def make(cls, params=None):
        """None: the library's defaults; a Display as is; a dict overrides some of the defaults (exposure, white, curve -- a CURVE_*
        or its name --, encode -- an ENCODE_*, or "srgb" / "linear")."""
        if isinstance(params, cls):
            return params
        d = cls.defaults()
        for k, v in (params or {}).items():
            if k not in ("exposure", "white", "curve", "encode"):
                raise ValueError(f"unknown display parameter {k!r}")
            if k == "curve" and isinstance(v, str):
                v = CURVES[v]
            if k == "encode" and isinstance(v, str):
                v = {"linear": ENCODE_LINEAR, "srgb": ENCODE_SRGB}[v]
            setattr(d, k, v)
        return d

    def as_dict(self):
        return {"exposure": self.exposure, "white": self.white, "curve": self.curve, "encode": self.encode}


class Metering(C.Structure):
    """sphip_metering: the key and the rank window of auto exposure (include/spath_hip.h)."""
    _fields_ = [("key", C.c_float), ("low", C.c_float), ("high", C.c_float), ("reserved", C.c_uint32)]

    @classmethod
    def defaults(cls):
        d = cls()
        load().sphip_metering_defaults(C.byref(d))
        return d

    @classmethod
    def make(cls, params=None):
        """None: the library's defaults; a Metering as is; a (key, low, high) tuple; a dict overrides some of the defaults."""
        if isinstance(params, cls):
            return params
        if isinstance(params, (tuple, list)):
            return cls(*[float(x) for x in params], 0)
        d = cls.defaults()
        for k, v in (params or {}).items():
            if k not in ("key", "low", "high", "reserved"):
                raise ValueError(f"unknown metering parameter {k!r}")
            setattr(d, k, v)
        return d

    def as_dict(self):
        return {"key": self.key, "low": self.low, "high": self.high}


def srgb_thresholds():
    """-> T[1] .. T[255] of the sRGB encoding, float32[255] (sphip_srgb_thresholds; needs no GPU)."""
    import numpy as np
    out = np.zeros(255, dtype=np.float32)
    load().sphip_srgb_thresholds(out.ctypes.data)
    return out


def exposure_from_histogram(hist, metering=None):
    """sphip_exposure_from_histogram: the exposure the 2048-bin luminance histogram `hist` meters (host only; metering as for
    Metering.make)."""
    import numpy as np
    hist = np.ascontiguousarray(hist, dtype=np.uint32)
    if hist.shape != (LUM_BINS,):
        raise ValueError("a luminance histogram has 2048 bins")
    m = Metering.make(metering)
    e = C.c_float(0.0)
    L = load()
    rc = L.sphip_exposure_from_histogram(hist.ctypes.data, C.byref(m), C.byref(e))
    if rc != 0:
        raise SpathHipError(f"sphip_exposure_from_histogram failed [{rc}]: {L.sphip_last_error(None).decode()}")
    return e.value


def gbuffer_dtype():
    """numpy dtype of one 32-byte G-buffer entry {nx, ny, nz, dist, ar, ag, ab, mat}."""
    import numpy as np
    return np.dtype([("n", "<f4", 3), ("dist", "<f4"), ("a", "<f4", 3), ("mat", "<i4")])


class Stats(C.Structure):
    _fields_ = [("kernel_ms", C.c_double), ("upload_ms", C.c_double), ("download_ms", C.c_double),
                ("scans_executed", C.c_uint64), ("n_tris", C.c_uint64), ("n_pixels", C.c_uint64),
                ("kernel_variant", C.c_uint32), ("n_launches", C.c_uint32),
                ("n_devices", C.c_uint32), ("gather_kind", C.c_uint32), ("gather_ms", C.c_double), ("kernel_ms_min", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class SpathHipError(RuntimeError):
    """A non-zero status from the C ABI (the C++ adapter throws std::runtime_error at the same point)."""


_lib = None


def load():
    """Load libspath_hip.so; raises if it has not been built (python __graft_entry__.py build)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise SpathHipError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`; "
                            "there is no CPU fallback for the HIP path")
    L = C.CDLL(LIB_PATH)
    vp, sz = C.c_void_p, C.c_size_t
    L.sphip_abi_version.restype = C.c_int
    L.sphip_kernel_name.restype = C.c_char_p
    L.sphip_kernel_name.argtypes = [C.c_int]
    L.sphip_create.restype = C.c_int
    L.sphip_create.argtypes = [C.c_int, C.POINTER(vp)]
    L.sphip_destroy.restype = None
    L.sphip_destroy.argtypes = [vp]
    L.sphip_last_error.restype = C.c_char_p
    L.sphip_last_error.argtypes = [vp]
    L.sphip_description.restype = C.c_char_p
    L.sphip_description.argtypes = [vp]
    L.sphip_set_scene.restype = C.c_int
    L.sphip_set_scene.argtypes = [vp, vp, vp, sz]
    L.sphip_render.restype = C.c_int
    L.sphip_render.argtypes = [vp, vp, sz, sz, sz, C.c_uint64, C.c_int, C.c_int, vp, vp]
    L.sphip_set_scene_device.restype = C.c_int
    L.sphip_set_scene_device.argtypes = [vp, vp, vp, sz, vp]
    L.sphip_render_device.restype = C.c_int
    L.sphip_render_device.argtypes = [vp, vp, sz, C.POINTER(Shard), sz, sz, C.c_uint64, C.c_int, C.c_int, vp, vp, vp]
    L.sphip_closest_hit_device.restype = C.c_int
    L.sphip_closest_hit_device.argtypes = [vp, vp, sz, vp, C.c_int, vp, vp, vp]
    L.sphip_viewport_device.restype = C.c_int
    L.sphip_viewport_device.argtypes = [vp, C.POINTER(CameraArgs), vp, vp]
    L.sphip_render_camera.restype = C.c_int
    L.sphip_render_camera.argtypes = [vp, C.POINTER(CameraArgs), sz, C.c_uint64, C.c_int, C.c_int, vp, vp]
    L.sphip_get_stats.restype = C.c_int
    L.sphip_get_stats.argtypes = [vp, C.POINTER(Stats)]
    L.sphip_selftest_device.restype = C.c_int
    L.sphip_selftest_device.argtypes = [vp, C.c_int, vp, sz, vp]
    # older builds (A/B libraries of earlier rounds) lack the next two: bind them when present
    if hasattr(L, "sphip_kernel_available"):
        L.sphip_kernel_available.restype = C.c_int
        L.sphip_kernel_available.argtypes = [C.c_int]
    if hasattr(L, "sphip_build_info"):
        L.sphip_build_info.restype = C.c_char_p
        L.sphip_build_info.argtypes = []
    if hasattr(L, "sphip_selftest_stage1"):
        L.sphip_selftest_stage1.restype = C.c_int
        L.sphip_selftest_stage1.argtypes = [vp, vp, sz, vp, vp, vp, C.POINTER(C.c_uint32)]
    if hasattr(L, "sphip_selftest_retest"):
        L.sphip_selftest_retest.restype = C.c_int
        L.sphip_selftest_retest.argtypes = [vp, vp, sz, vp, vp, C.POINTER(C.c_uint32)]
    if hasattr(L, "sphip_selftest_sort"):
        L.sphip_selftest_sort.restype = C.c_int
        L.sphip_selftest_sort.argtypes = [vp, vp, vp, sz, C.c_uint32, vp, vp]
        L.sphip_selftest_bvh_dump.restype = C.c_int
        L.sphip_selftest_bvh_dump.argtypes = [vp, C.POINTER(C.c_uint32), vp, vp, vp, vp]
        L.sphip_selftest_bvh_walk.restype = C.c_int
        L.sphip_selftest_bvh_walk.argtypes = [vp, vp, sz, vp, vp, C.c_int, vp, vp, vp, vp]
    L.sphip_render_device_accum.restype = C.c_int
    L.sphip_render_device_accum.argtypes = [vp, vp, sz, C.POINTER(Shard), sz, C.c_uint64, sz, C.c_uint64, C.c_int, vp, vp, vp, vp]
    L.sphip_accum_begin.restype = C.c_int
    L.sphip_accum_begin.argtypes = [vp, vp, C.POINTER(CameraArgs), sz, sz, C.c_uint64, C.c_int]
    L.sphip_accum_step.restype = C.c_int
    L.sphip_accum_step.argtypes = [vp, sz, vp, vp, C.POINTER(C.c_uint64)]
    L.sphip_accum_begin_adaptive.restype = C.c_int
    L.sphip_accum_begin_adaptive.argtypes = [vp, vp, C.POINTER(CameraArgs), sz, sz, C.c_uint64, C.c_int, C.POINTER(Adaptive)]
    L.sphip_accum_counts.restype = C.c_int
    L.sphip_accum_counts.argtypes = [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
    L.sphip_denoise_defaults.restype = None
    L.sphip_denoise_defaults.argtypes = [C.POINTER(Denoise)]
    L.sphip_gbuffer_device.restype = C.c_int
    L.sphip_gbuffer_device.argtypes = [vp, vp, sz, C.c_int, vp, vp]
    L.sphip_denoise_device.restype = C.c_int
    L.sphip_denoise_device.argtypes = [vp, C.POINTER(Denoise), sz, sz, vp, vp, vp, vp, vp, vp]
    L.sphip_accum_gbuffer.restype = C.c_int
    L.sphip_accum_gbuffer.argtypes = [vp, vp]
    L.sphip_accum_denoise.restype = C.c_int
    L.sphip_accum_denoise.argtypes = [vp, C.POINTER(Denoise), vp, vp]
    L.sphip_reproject_defaults.restype = None
    L.sphip_reproject_defaults.argtypes = [C.POINTER(Reproject)]
    L.sphip_reproject_device.restype = C.c_int
    L.sphip_reproject_device.argtypes = [vp, C.POINTER(Reproject), C.POINTER(CameraArgs), sz, sz, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.sphip_temporal_resolve_device.restype = C.c_int
    L.sphip_temporal_resolve_device.argtypes = [vp, sz, vp, C.c_uint32, vp, vp, vp, vp, vp]
    L.sphip_accum_reproject.restype = C.c_int
    L.sphip_accum_reproject.argtypes = [vp, C.POINTER(CameraArgs), C.c_uint64, C.POINTER(Reproject)]
    L.sphip_accum_history.restype = C.c_int
    L.sphip_accum_history.argtypes = [vp, vp]
    L.sphip_display_defaults.restype = None
    L.sphip_display_defaults.argtypes = [C.POINTER(Display)]
    L.sphip_metering_defaults.restype = None
    L.sphip_metering_defaults.argtypes = [C.POINTER(Metering)]
    L.sphip_srgb_thresholds.restype = None
    L.sphip_srgb_thresholds.argtypes = [vp]
    L.sphip_luminance_histogram_device.restype = C.c_int
    L.sphip_luminance_histogram_device.argtypes = [vp, sz, vp, vp, vp]
    L.sphip_exposure_from_histogram.restype = C.c_int
    L.sphip_exposure_from_histogram.argtypes = [vp, C.POINTER(Metering), C.POINTER(C.c_float)]
    L.sphip_display_device.restype = C.c_int
    L.sphip_display_device.argtypes = [vp, C.POINTER(Display), sz, vp, vp, vp, vp]
    L.sphip_accum_display.restype = C.c_int
    L.sphip_accum_display.argtypes = [vp, C.POINTER(Display), C.POINTER(Metering), C.POINTER(Denoise), vp, vp, C.POINTER(C.c_float)]
    L.sphip_set_lens.restype = C.c_int
    L.sphip_set_lens.argtypes = [vp, C.POINTER(Lens)]
    L.sphip_camera_rays_device.restype = C.c_int
    L.sphip_camera_rays_device.argtypes = [vp, C.POINTER(CameraArgs), C.c_uint64, C.c_uint32, vp, vp]
    for name, _, _ in TRI_TABLES:
        host, dev = getattr(L, "sphip_set_" + name), getattr(L, "sphip_set_" + name + "_device")
        host.restype = dev.restype = C.c_int
        host.argtypes, dev.argtypes = [vp, vp], [vp, vp, vp]
    L.sphip_set_texture.restype = C.c_int
    L.sphip_set_texture.argtypes = [vp, vp, C.c_uint32, C.c_uint32]
    L.sphip_set_texture_device.restype = C.c_int
    L.sphip_set_texture_device.argtypes = [vp, vp, C.c_uint32, C.c_uint32, vp]
    L.sphip_set_normal_map.restype = C.c_int
    L.sphip_set_normal_map.argtypes = [vp, vp, C.c_uint32, C.c_uint32]
    L.sphip_set_normal_map_device.restype = C.c_int
    L.sphip_set_normal_map_device.argtypes = [vp, vp, C.c_uint32, C.c_uint32, vp]
    L.sphip_set_environment.restype = C.c_int
    L.sphip_set_environment.argtypes = [vp, vp, C.c_uint32]
    L.sphip_set_environment_device.restype = C.c_int
    L.sphip_set_environment_device.argtypes = [vp, vp, C.c_uint32, vp]
    L.sphip_selftest_env_dump.restype = C.c_int
    L.sphip_selftest_env_dump.argtypes = [vp, C.POINTER(C.c_uint32), vp, vp, vp, vp, vp]
    L.sphip_create_multi.restype = C.c_int
    L.sphip_create_multi.argtypes = [C.POINTER(C.c_int), C.c_int, C.POINTER(vp)]
    L.sphip_device_count.restype = C.c_int
    L.sphip_device_count.argtypes = [vp]
    L.sphip_plan_tile_rows.restype = C.c_int
    L.sphip_plan_tile_rows.argtypes = [sz, C.c_int]
    L.sphip_plan_shard.restype = C.c_int
    L.sphip_plan_shard.argtypes = [sz, sz, C.c_int, sz, C.c_int, C.POINTER(Shard), C.POINTER(sz)]
    _lib = L
    return L


def kernel_variants():
    """{name: id} of the scan-kernel variants the library exposes (id 0 = auto)."""
    L = load()
    out, i = {}, 0
    while True:
        n = L.sphip_kernel_name(i)
        if n is None:
            break
        out[n.decode()] = i
        i += 1
    return out


def build_source_hash() -> str:
    """The source/flags hash compiled into the loaded library ("unknown" for hand-made builds and libraries of earlier rounds)."""
    L = load()
    if not hasattr(L, "sphip_build_info"):
        return "unknown"
    return L.sphip_build_info().decode().split("src=")[-1]


def available_variants():
    """ids (> 0) of the kernel variants the library carries: 1, 2, 8, 15, 16 (the numbers of the earlier filter generations
    keep their names and are refused)."""
    L = load()
    ids = sorted(v for v in kernel_variants().values() if v > 0)
    if not hasattr(L, "sphip_kernel_available"):
        return ids
    return [v for v in ids if L.sphip_kernel_available(v)]


def plan_tile_rows(height: int, n_devices: int) -> int:
    """The library's row-tile height for a frame of `height` rows on n_devices GPUs (pure host arithmetic)."""
    return load().sphip_plan_tile_rows(height, n_devices)


def plan_shard(width: int, height: int, n_devices: int, tile_rows: int, rank: int):
    """((pixel_base, tile_px, tile_stride_px), n_rays) of device `rank` in the library's round-robin row-tile plan."""
    sh, n = Shard(), C.c_size_t(0)
    rc = load().sphip_plan_shard(width, height, n_devices, tile_rows, rank, C.byref(sh), C.byref(n))
    if rc != 0:
        raise SpathHipError(f"sphip_plan_shard: bad arguments [{rc}]")
    return (sh.pixel_base, sh.tile_px, sh.tile_stride_px), n.value


class Context:
    """One sphip_t: a device (or, from Context.multi, several), its cached buffers and its scene."""

    def __init__(self, device: int = 0, _handle=None):
        self._L = load()
        if _handle is not None:
            self._h, self.device = _handle, None
            return
        h = C.c_void_p()
        rc = self._L.sphip_create(device, C.byref(h))
        if rc != 0:
            raise SpathHipError(f"sphip_create({device}) failed [{rc}]: {self._L.sphip_last_error(None).decode()}")
        self._h = h
        self.device = device

    @classmethod
    def multi(cls, device_ids=None):
        """sphip_create_multi: every listed device behind one context (None: all visible devices / SPATH_HIP_DEVICES).
        Only the host-pointer calls (set_scene, render, render_camera, stats) work on it."""
        L = load()
        h = C.c_void_p()
        if device_ids is None:
            rc = L.sphip_create_multi(None, 0, C.byref(h))
        else:
            arr = (C.c_int * len(device_ids))(*[int(d) for d in device_ids])
            rc = L.sphip_create_multi(arr, len(device_ids), C.byref(h))
        if rc != 0:
            raise SpathHipError(f"sphip_create_multi({device_ids}) failed [{rc}]: {L.sphip_last_error(None).decode()}")
        return cls(_handle=h)

    @property
    def device_count(self) -> int:
        return self._L.sphip_device_count(self._h)

    def close(self):
        if getattr(self, "_h", None):
            self._L.sphip_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            raise SpathHipError(f"{what} failed [{rc}]: {self._L.sphip_last_error(self._h).decode()}")

    @property
    def description(self) -> str:
        return self._L.sphip_description(self._h).decode()

    # host-pointer path -------------------------------------------------------------------------
    def set_scene(self, tris, mats):
        import numpy as np
        tris = np.ascontiguousarray(tris, dtype=np.float32).reshape(-1, 12)
        mats = np.ascontiguousarray(mats, dtype=np.float32).reshape(-1, 6)
        if tris.shape[0] != mats.shape[0]:
            raise ValueError("one material per triangle")
        self._check(self._L.sphip_set_scene(self._h, tris.ctypes.data, mats.ctypes.data, tris.shape[0]), "sphip_set_scene")
        self._n_tris = tris.shape[0]

    def _set_table(self, name, rows):
        """sphip_set_<name> of TRI_TABLES: rows as (n_tris, floats) f32 for the scene last set, or None to clear the table."""
        import numpy as np
        what = "sphip_set_" + name
        if rows is not None:
            floats, mismatch = next(t[1:] for t in TRI_TABLES if t[0] == name)
            rows = np.ascontiguousarray(rows, dtype=np.float32).reshape(-1, floats)
            if rows.shape[0] != getattr(self, "_n_tris", rows.shape[0]):
                raise ValueError(mismatch)
        self._check(getattr(self._L, what)(self._h, None if rows is None else rows.ctypes.data), what)

    def _set_table_device(self, name, d_rows, stream):
        what = "sphip_set_" + name + "_device"
        self._check(getattr(self._L, what)(self._h, d_rows, stream), what)

    def set_specular(self, spec):
        """sphip_set_specular: the specular table of FLAG_SPECULAR renders, (n_tris, 4) f32 rows ks.r, ks.g, ks.b, p for the scene last
        set (scene.specular_table builds one); None clears it.  Every set_scene clears it too."""
        self._set_table("specular", spec)

    def set_vertex_normals(self, vn):
        """sphip_set_vertex_normals: the per-vertex normals of FLAG_SMOOTH renders, (n_tris, 9) f32 rows n0.xyz n1.xyz n2.xyz for the
        scene last set (scene.vertex_normals builds them); None clears them.  Every set_scene clears them too."""
        self._set_table("vertex_normals", vn)

    def set_dielectric(self, glass):
        """sphip_set_dielectric: the dielectric table of FLAG_DIELECTRIC renders, (n_tris, 4) f32 rows kt.r, kt.g, kt.b, ior for the
        scene last set (scene.dielectric_table builds one); None clears it.  Every set_scene clears it too."""
        self._set_table("dielectric", glass)

    def set_roughness(self, alpha):
        """sphip_set_roughness: the roughness table of FLAG_GLOSSY renders, n_tris f32, the GGX alpha of each triangle's mirror lobe for
        the scene last set (scene.roughness_table builds one); None clears it.  Every set_scene clears it too."""
        self._set_table("roughness", alpha)

    def set_uv(self, uv):
        """sphip_set_uv: the UV table of FLAG_TEXTURE renders, (n_tris, 6) f32: s0 t0 s1 t1 s2 t2 for v0 v1 v2 of each triangle of the
        scene last set (scene.uv_table and scene.planar_uv build one); a row of zeros leaves its triangle untextured; None clears it.
        Every set_scene clears it too."""
        self._set_table("uv", uv)

    def set_texture(self, texels):
        """sphip_set_texture: the atlas of FLAG_TEXTURE renders, (th, tw, 3) f32 with texel (i, j) at [j, i] (scene.checker_texture
        builds one); None clears it.  set_scene keeps it."""
        import numpy as np
        if texels is None:
            self._check(self._L.sphip_set_texture(self._h, None, 0, 0), "sphip_set_texture")
            return
        texels = np.ascontiguousarray(texels, dtype=np.float32)
        if texels.ndim != 3 or texels.shape[2] != 3:
            raise ValueError("an atlas is (th, tw, 3)")
        self._check(self._L.sphip_set_texture(self._h, texels.ctypes.data, texels.shape[1], texels.shape[0]), "sphip_set_texture")

    def set_environment(self, texels):
        """sphip_set_environment: the octahedral environment map, (n, n, 3) f32 with texel (i, j) at [j, i] (scene.sky_environment and
        scene.environment_from_latlong build one); None clears it.  set_scene keeps it."""
        import numpy as np
        if texels is None:
            self._check(self._L.sphip_set_environment(self._h, None, 0), "sphip_set_environment")
            return
        texels = np.ascontiguousarray(texels, dtype=np.float32)
        if texels.ndim != 3 or texels.shape[0] != texels.shape[1] or texels.shape[2] != 3:
            raise ValueError("an environment map is (n, n, 3)")
        self._check(self._L.sphip_set_environment(self._h, texels.ctypes.data, texels.shape[0]), "sphip_set_environment")

    def render(self, rays, w, h, n_samples, seed=1, mode=MODE_PT, flags=0, want_accum=False):
        import numpy as np
        rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 6)
        if rays.shape[0] != w * h:
            raise ValueError("rays must hold w*h entries")
        out = np.zeros((w * h, 4), dtype=np.uint8)
        acc = np.zeros((w * h, 3), dtype=np.float32) if want_accum else None
        self._check(self._L.sphip_render(self._h, rays.ctypes.data, w, h, n_samples, seed, mode, flags,
                                         out.ctypes.data, acc.ctypes.data if want_accum else None), "sphip_render")
        return (out, acc) if want_accum else out

    # device-resident path ----------------------------------------------------------------------
    def set_scene_device(self, d_tris: int, d_mats: int, n_tris: int, stream: int = 0):
        self._check(self._L.sphip_set_scene_device(self._h, d_tris, d_mats, n_tris, stream), "sphip_set_scene_device")
        self._n_tris = n_tris

    def set_specular_device(self, d_spec: int, stream: int = 0):
        """sphip_set_specular_device: the table from a device pointer (n_tris * 4 f32, copied in stream order, NOT validated)."""
        self._set_table_device("specular", d_spec, stream)

    def set_vertex_normals_device(self, d_vn: int, stream: int = 0):
        """sphip_set_vertex_normals_device: the normals from a device pointer (n_tris * 9 f32, copied in stream order, NOT validated)."""
        self._set_table_device("vertex_normals", d_vn, stream)

    def set_dielectric_device(self, d_glass: int, stream: int = 0):
        """sphip_set_dielectric_device: the table from a device pointer (n_tris * 4 f32, copied in stream order, NOT validated)."""
        self._set_table_device("dielectric", d_glass, stream)

    def set_roughness_device(self, d_alpha: int, stream: int = 0):
        """sphip_set_roughness_device: the table from a device pointer (n_tris f32, copied in stream order, NOT validated)."""
        self._set_table_device("roughness", d_alpha, stream)

    def set_uv_device(self, d_uv: int, stream: int = 0):
        """sphip_set_uv_device: the table from a device pointer (n_tris * 6 f32, copied in stream order, NOT validated)."""
        self._set_table_device("uv", d_uv, stream)

    def set_normal_map(self, texels):
        """sphip_set_normal_map: the normal map of FLAG_NORMAL_MAP renders, (nh, nw, 3) f32 with texel (i, j) at [j, i], each a signed
        tangent-space vector (scene.normal_map_from_height and scene.decode_normal_map build one); None clears it.  set_scene keeps it."""
        import numpy as np
        if texels is None:
            self._check(self._L.sphip_set_normal_map(self._h, None, 0, 0), "sphip_set_normal_map")
            return
        texels = np.ascontiguousarray(texels, dtype=np.float32)
        if texels.ndim != 3 or texels.shape[2] != 3:
            raise ValueError("a normal map is (nh, nw, 3)")
        self._check(self._L.sphip_set_normal_map(self._h, texels.ctypes.data, texels.shape[1], texels.shape[0]), "sphip_set_normal_map")

    def set_normal_map_device(self, d_texels: int, nw: int, nh: int, stream: int = 0):
        """sphip_set_normal_map_device: the map from a device pointer (nw * nh * 3 f32, copied in stream order, NOT validated)."""
        self._check(self._L.sphip_set_normal_map_device(self._h, d_texels or None, nw, nh, stream or None), "sphip_set_normal_map_device")

    def set_texture_device(self, d_texels: int, tw: int, th: int, stream: int = 0):
        """sphip_set_texture_device: the atlas from a device pointer (tw * th * 3 f32, copied in stream order, NOT validated)."""
        self._check(self._L.sphip_set_texture_device(self._h, d_texels or None, tw, th, stream or None), "sphip_set_texture_device")

    def set_environment_device(self, d_texels: int, n: int, stream: int = 0):
        """sphip_set_environment_device: the map from a device pointer (n * n * 3 f32, copied in stream order, NOT validated)."""
        self._check(self._L.sphip_set_environment_device(self._h, d_texels or None, n, stream or None), "sphip_set_environment_device")

    def render_device(self, d_rays: int, n_rays: int, n_samples: int, d_out_rgba: int, *, seed=1, mode=MODE_PT,
                      flags=0, shard=None, image_width=0, d_out_accum: int = 0, stream: int = 0):
        sh = None
        if shard is not None:
            sh = C.byref(Shard(*[int(v) for v in shard]))
        self._check(self._L.sphip_render_device(self._h, d_rays, n_rays, sh, image_width, n_samples, seed, mode, flags,
                                                d_out_rgba, d_out_accum or None, stream or None), "sphip_render_device")

    def render_device_accum(self, d_rays: int, n_rays: int, sample_base: int, n_samples: int, d_sum: int, d_out_rgba: int, *,
                            seed=1, flags=0, shard=None, image_width=0, d_out_mean: int = 0, stream: int = 0):
        """Progressive step on device pointers: global samples [sample_base, sample_base + n_samples) added to the running sum
        d_sum (n_rays*3 f32, in place; not read when sample_base == 0); the outputs are those of a render of all of them."""
        sh = None
        if shard is not None:
            sh = C.byref(Shard(*[int(v) for v in shard]))
        self._check(self._L.sphip_render_device_accum(self._h, d_rays, n_rays, sh, image_width, sample_base, n_samples, seed, flags,
                                                      d_sum or None, d_out_rgba, d_out_mean or None, stream or None),
                    "sphip_render_device_accum")

    def closest_hit_device(self, d_rays: int, n_rays: int, d_out_idx: int, d_out_dist: int, *, d_src_idx: int = 0,
                           flags=0, stream: int = 0):
        self._check(self._L.sphip_closest_hit_device(self._h, d_rays, n_rays, d_src_idx or None, flags,
                                                     d_out_idx, d_out_dist, stream or None), "sphip_closest_hit_device")

    def viewport_device(self, cam, d_rays_out: int, stream: int = 0):
        """camera::get_viewport on the device (cam: spath_amd.view.Camera); writes res_x*res_y*6 floats."""
        ca = CameraArgs.from_camera(cam)
        self._check(self._L.sphip_viewport_device(self._h, C.byref(ca), d_rays_out, stream or None), "sphip_viewport_device")

    def set_lens(self, aperture=0.0, focus_dist=0.0, reserved=0):
        """sphip_set_lens: the thin lens of later FLAG_CAMERA_SAMPLES renders (aperture 0 = pinhole); an accumulation keeps the lens of
        its begin."""
        lens = Lens(float(aperture), float(focus_dist), int(reserved))
        self._check(self._L.sphip_set_lens(self._h, C.byref(lens)), "sphip_set_lens")

    def camera_rays_device(self, cam, sample: int, d_rays_out: int, *, seed=1, stream: int = 0):
        """sphip_camera_rays_device: the res_x*res_y primary rays of global sample `sample` with the context's lens (6 floats each)."""
        ca = CameraArgs.from_camera(cam)
        self._check(self._L.sphip_camera_rays_device(self._h, C.byref(ca), seed, sample, d_rays_out, stream or None),
                    "sphip_camera_rays_device")

    def render_camera(self, cam, n_samples, seed=1, mode=MODE_PT, flags=0, want_accum=False):
        """get_viewport + render in one call; the rays never leave the device."""
        import numpy as np
        ca = CameraArgs.from_camera(cam)
        n = cam.res_x * cam.res_y
        out = np.zeros((n, 4), dtype=np.uint8)
        acc = np.zeros((n, 3), dtype=np.float32) if want_accum else None
        self._check(self._L.sphip_render_camera(self._h, C.byref(ca), n_samples, seed, mode, flags, out.ctypes.data,
                                                acc.ctypes.data if want_accum else None), "sphip_render_camera")
        return (out, acc) if want_accum else out

    # progressive rendering -------------------------------------------------------------------
    def accum_begin(self, rays=None, cam=None, w=None, h=None, seed=1, flags=0, adaptive=None):
        """Start accumulating the viewport given by exactly one of `rays` (w*h rays, uploaded once) and `cam`
        (spath_amd.view.Camera, generated on the device; w and h default to its resolution).
        adaptive=(t, floor, min_samples): adaptive sampling, converged pixels stop (sphip_accum_begin_adaptive); accum_step's
        total is then the sample count of the still-active pixels, accum_counts() gives every pixel's."""
        import numpy as np
        ca = None
        if cam is not None:
            ca = CameraArgs.from_camera(cam)
            w = cam.res_x if w is None else w
            h = cam.res_y if h is None else h
        ptr = None
        if rays is not None:
            rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 6)
            if w is None or h is None or rays.shape[0] != w * h:
                raise ValueError("rays must hold w*h entries")
            ptr = rays.ctypes.data
        self._accum_shape = (int(w or 0), int(h or 0))
        cap = C.byref(ca) if ca is not None else None
        if adaptive is None:
            self._check(self._L.sphip_accum_begin(self._h, ptr, cap, int(w or 0), int(h or 0), seed, flags), "sphip_accum_begin")
            return
        t, floor, min_samples = adaptive
        rule = Adaptive(float(t), float(floor), int(min_samples), 0)
        self._check(self._L.sphip_accum_begin_adaptive(self._h, ptr, cap, int(w or 0), int(h or 0), seed, flags, C.byref(rule)),
                    "sphip_accum_begin_adaptive")

    def accum_step(self, n, want_mean=False):
        """n more samples of the current accumulation -> (img, total) or (img, mean, total): the image (and mean) of all
        `total` samples so far, bit-identical to render(..., total, ...)."""
        import numpy as np
        w, h = getattr(self, "_accum_shape", (0, 0))
        out = np.zeros((w * h, 4), dtype=np.uint8)
        mean = np.zeros((w * h, 3), dtype=np.float32) if want_mean else None
        total = C.c_uint64(0)
        self._check(self._L.sphip_accum_step(self._h, n, out.ctypes.data if w * h else None, mean.ctypes.data if want_mean and w * h else None,
                                             C.byref(total)), "sphip_accum_step")
        return (out, mean, total.value) if want_mean else (out, total.value)

    def accum_counts(self):
        """-> (counts[h, w] uint32, n_active): every pixel's sample count in the current accumulation and the number of pixels
        still active (a plain accumulation: `total` everywhere, all active)."""
        import numpy as np
        w, h = getattr(self, "_accum_shape", (0, 0))
        counts = np.zeros((h, w), dtype=np.uint32)
        n_active = C.c_uint64(0)
        self._check(self._L.sphip_accum_counts(self._h, counts.ctypes.data_as(C.POINTER(C.c_uint32)) if w * h else None, C.byref(n_active)),
                    "sphip_accum_counts")
        return counts, n_active.value

    # denoising -------------------------------------------------------------------------------
    def gbuffer_device(self, d_rays: int, n_rays: int, d_out_gbuf: int, *, flags=0, stream: int = 0):
        """G-buffer of n_rays primary rays into d_out_gbuf (n_rays * 32 B, see gbuffer_dtype()); asynchronous."""
        self._check(self._L.sphip_gbuffer_device(self._h, d_rays, n_rays, flags, d_out_gbuf, stream or None), "sphip_gbuffer_device")

    def denoise_device(self, w: int, h: int, d_mean: int, d_gbuf: int, d_out_rgba: int, *, d_var: int = 0, d_out_rgb: int = 0,
                       params=None, stream: int = 0):
        """The a-trous filter on device pointers (d_var 0: no luminance weight); params as for Denoise.make."""
        p = Denoise.make(params)
        self._check(self._L.sphip_denoise_device(self._h, C.byref(p), w, h, d_mean, d_var or None, d_gbuf, d_out_rgba, d_out_rgb or None,
                                                 stream or None), "sphip_denoise_device")

    def accum_gbuffer(self):
        """-> the current accumulation's G-buffer, a structured array [w*h] of gbuffer_dtype()."""
        import numpy as np
        w, h = getattr(self, "_accum_shape", (0, 0))
        out = np.zeros(w * h, dtype=gbuffer_dtype())
        self._check(self._L.sphip_accum_gbuffer(self._h, out.ctypes.data if w * h else None), "sphip_accum_gbuffer")
        return out

    def accum_denoise(self, params=None, want_rgb=False):
        """The current accumulation denoised (it is not altered) -> img, or (img, rgb) with want_rgb."""
        import numpy as np
        w, h = getattr(self, "_accum_shape", (0, 0))
        p = Denoise.make(params)
        out = np.zeros((w * h, 4), dtype=np.uint8)
        rgb = np.zeros((w * h, 3), dtype=np.float32) if want_rgb else None
        self._check(self._L.sphip_accum_denoise(self._h, C.byref(p), out.ctypes.data if w * h else None,
                                                rgb.ctypes.data if want_rgb and w * h else None), "sphip_accum_denoise")
        return (out, rgb) if want_rgb else out

    # temporal reprojection -------------------------------------------------------------------
    def reproject_device(self, params, cam_prev, w: int, h: int, d_rays_cur: int, d_gbuf_cur: int, d_rays_prev: int, d_gbuf_prev: int,
                         d_mean_prev: int, d_hist_prev: int, d_out_mean: int, d_out_hist: int, stream: int = 0):
        """The previous view's (mean, history count) resampled at the current view's primary hits (device pointers; asynchronous).
        cam_prev: the previous view's view.Camera or CameraArgs; params as for Reproject.make."""
        p = Reproject.make(params)
        ca = cam_prev if isinstance(cam_prev, CameraArgs) or cam_prev is None else CameraArgs.from_camera(cam_prev)
        self._check(self._L.sphip_reproject_device(self._h, C.byref(p), C.byref(ca) if ca is not None else None, w, h, d_rays_cur or None,
                                                   d_gbuf_cur or None, d_rays_prev or None, d_gbuf_prev or None, d_mean_prev or None,
                                                   d_hist_prev or None, d_out_mean or None, d_out_hist or None, stream or None),
                    "sphip_reproject_device")

    def temporal_resolve_device(self, n: int, d_sum: int, n_samples: int, d_out_rgba: int = 0, d_out_mean: int = 0, *, d_hist_mean: int = 0,
                                d_hist: int = 0, stream: int = 0):
        """The blend of the running sum of n_samples samples with a history (none: the plain resolve) on device pointers; asynchronous."""
        self._check(self._L.sphip_temporal_resolve_device(self._h, n, d_sum or None, n_samples, d_hist_mean or None, d_hist or None,
                                                          d_out_rgba or None, d_out_mean or None, stream or None), "sphip_temporal_resolve_device")

    def accum_reproject(self, cam_new, seed, params=None):
        """Moves the current accumulation to the view cam_new (view.Camera) and keeps what it has gathered as history; pass a seed other
        than the history's.  params as for Reproject.make."""
        p = Reproject.make(params)
        ca = cam_new if isinstance(cam_new, CameraArgs) or cam_new is None else CameraArgs.from_camera(cam_new)
        self._check(self._L.sphip_accum_reproject(self._h, C.byref(ca) if ca is not None else None, seed, C.byref(p)), "sphip_accum_reproject")

    def accum_history(self):
        """-> the per-pixel history counts of the current accumulation, float32 [w*h] (all 0 without a history)."""
        import numpy as np
        w, h = getattr(self, "_accum_shape", (0, 0))
        out = np.zeros(w * h, dtype=np.float32)
        self._check(self._L.sphip_accum_history(self._h, out.ctypes.data if w * h else None), "sphip_accum_history")
        return out

    # display transform ------------------------------------------------------------------------
    def luminance_histogram_device(self, n: int, d_mean: int, d_out_hist: int, stream: int = 0):
        """The 2048-bin luminance histogram of the n pixels of d_mean (n*3 f32) into d_out_hist (2048 u32); asynchronous."""
        self._check(self._L.sphip_luminance_histogram_device(self._h, n, d_mean or None, d_out_hist or None, stream or None),
                    "sphip_luminance_histogram_device")

    def display_device(self, n: int, d_mean: int, d_out_rgba: int, *, d_out_rgb: int = 0, params=None, stream: int = 0):
        """Exposure, tone curve and encoding of n pixels on device pointers; params as for Display.make; asynchronous."""
        p = Display.make(params)
        self._check(self._L.sphip_display_device(self._h, C.byref(p), n, d_mean or None, d_out_rgba or None, d_out_rgb or None, stream or None),
                    "sphip_display_device")

    def accum_display(self, params=None, metering=None, denoise=None, want_rgb=False):
        """The current accumulation through the display transform (it is not altered) -> (img, exposure) or (img, rgb, exposure).
        metering: None = params' exposure as given, True = the default window, else as for Metering.make; denoise: None = the raw
        mean, True = the default filter, else as for Denoise.make."""
        import numpy as np
        w, h = getattr(self, "_accum_shape", (0, 0))
        p = Display.make(params)
        m = None if metering is None or metering is False else Metering.make(None if metering is True else metering)
        dn = None if denoise is None or denoise is False else Denoise.make(None if denoise is True else denoise)
        out = np.zeros((w * h, 4), dtype=np.uint8)
        rgb = np.zeros((w * h, 3), dtype=np.float32) if want_rgb else None
        e = C.c_float(0.0)
        self._check(self._L.sphip_accum_display(self._h, C.byref(p), C.byref(m) if m is not None else None, C.byref(dn) if dn is not None else None,
                                                out.ctypes.data if w * h else None, rgb.ctypes.data if want_rgb and w * h else None, C.byref(e)),
                    "sphip_accum_display")
        return (out, rgb, e.value) if want_rgb else (out, e.value)

    SELFTEST_OUT = {0: ("float32", 2), 1: ("float32", 1), 2: ("float64", 2), 3: ("float32", 3), 4: ("float32", 1), 5: ("uint32", 1), 6: ("float32", 2),
                    7: ("float32", 6), 8: ("float32", 6), 9: ("float32", 4), 10: ("float32", 6), 11: ("float32", 8), 12: ("float32", 6),
                    13: ("float32", 6)}

    def selftest(self, what: int, inp, n: int):
        """sphip_selftest_device (test-only): one device function of the path on n caller-supplied inputs."""
        import numpy as np
        dt, k = self.SELFTEST_OUT[what]
        inp = np.ascontiguousarray(inp)
        out = np.zeros(n * k, dtype=dt)
        self._check(self._L.sphip_selftest_device(self._h, what, inp.ctypes.data, n, out.ctypes.data), "sphip_selftest_device")
        return out

    def selftest_sort(self, keys, vals, key_bits=32):
        """sphip_selftest_sort (test-only): the context's stable radix sort on caller (key, value) pairs -> (keys, vals) sorted."""
        import numpy as np
        keys = np.ascontiguousarray(keys, dtype=np.uint32)
        vals = np.ascontiguousarray(vals, dtype=np.uint32)
        assert keys.shape == vals.shape and keys.ndim == 1
        ok, ov = np.zeros_like(keys), np.zeros_like(vals)
        self._check(self._L.sphip_selftest_sort(self._h, keys.ctypes.data, vals.ctypes.data, keys.size, key_bits, ok.ctypes.data, ov.ctypes.data),
                    "sphip_selftest_sort")
        return ok, ov

    def selftest_bvh_dump(self):
        """sphip_selftest_bvh_dump (test-only): the linear BVH of the context's scene as built -> dict(n_leaves, meta u32[16],
        nodes f32[2 n_leaves, 8] (row 0 is never written), rec f32[4 n_leaves + 256, 12], idx i32[4 n_leaves + 256])."""
        import numpy as np
        nl = C.c_uint32(0)
        self._check(self._L.sphip_selftest_bvh_dump(self._h, C.byref(nl), None, None, None, None), "sphip_selftest_bvh_dump")
        n = nl.value
        meta = np.zeros(16, dtype=np.uint32)
        nodes = np.zeros((2 * n, 8), dtype=np.float32)
        rec = np.zeros((4 * n + 256, 12), dtype=np.float32)
        idx = np.zeros(4 * n + 256, dtype=np.int32)
        self._check(self._L.sphip_selftest_bvh_dump(self._h, C.byref(nl), meta.ctypes.data, nodes.ctypes.data, rec.ctypes.data, idx.ctypes.data),
                    "sphip_selftest_bvh_dump")
        assert nl.value == n
        return {"n_leaves": n, "meta": meta, "nodes": nodes, "rec": rec, "idx": idx}

    def selftest_env_dump(self):
        """sphip_selftest_env_dump (test-only): the importance tables of the context's map and scene -> dict(n, wt f64[n, n], rc f64[n, n],
        marg f64[n], tpdf f32[n, n], T, w_env, W), the 2-d arrays indexed [j, i]."""
        import numpy as np
        nn = C.c_uint32(0)
        self._check(self._L.sphip_selftest_env_dump(self._h, C.byref(nn), None, None, None, None, None), "sphip_selftest_env_dump")
        n = nn.value
        wt, rc, marg = np.zeros((n, n)), np.zeros((n, n)), np.zeros(n)
        tpdf, s = np.zeros((n, n), dtype=np.float32), np.zeros(3)
        self._check(self._L.sphip_selftest_env_dump(self._h, C.byref(nn), wt.ctypes.data, rc.ctypes.data, marg.ctypes.data, tpdf.ctypes.data,
                                                    s.ctypes.data), "sphip_selftest_env_dump")
        assert nn.value == n
        return {"n": n, "wt": wt, "rc": rc, "marg": marg, "tpdf": tpdf, "T": float(s[0]), "w_env": float(s[1]), "W": float(s[2])}

    def selftest_bvh_walk(self, rays, src=None, tmax=None, any_hit=False):
        """sphip_selftest_bvh_walk (test-only): the BVH traversal itself on caller rays -> (idx i32[n], d f32[n], steps u32[n], leaves u32[n])."""
        import numpy as np
        rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 6)
        n = rays.shape[0]
        src = None if src is None else np.ascontiguousarray(src, dtype=np.int32)
        tmax = None if tmax is None else np.ascontiguousarray(tmax, dtype=np.float32)
        assert (src is None or src.shape == (n,)) and (tmax is None or tmax.shape == (n,))
        idx, d = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.float32)
        steps, leaves = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
        self._check(self._L.sphip_selftest_bvh_walk(self._h, rays.ctypes.data, n, None if src is None else src.ctypes.data,
                                                    None if tmax is None else tmax.ctypes.data, int(bool(any_hit)), idx.ctypes.data, d.ctypes.data,
                                                    steps.ctypes.data, leaves.ctypes.data), "sphip_selftest_bvh_walk")
        return idx, d, steps, leaves

    def selftest_stage1(self, rays, per_triangle=True):
        """sphip_selftest_stage1 (test-only): stage 1 of the default scan alone for the given rays (padded to a multiple of 64)
        against the context's scene.  Returns (group_survives, tri_survives, order): both [ray, stream position] bool -- the
        position's OCTET (its group of four and the partner group two further on) survives the bound of the octet / the triangle itself survives
        the per-pair form of the test
        (None unless per_triangle) -- and order[stream position] = triangle index (n_tris = padding)."""
        import numpy as np
        rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 6)
        n = rays.shape[0]
        n_pad = (n + 63) // 64 * 64
        if n_pad != n:
            rays = np.concatenate([rays, np.repeat(rays[-1:], n_pad - n, axis=0)])
        tiles = C.c_uint32(0)
        self._check(self._L.sphip_selftest_stage1(self._h, None, 0, None, None, None, C.byref(tiles)), "sphip_selftest_stage1")
        t, T, octets = tiles.value & 0xFFFFF, (tiles.value >> 20) & 0x7FF, bool(tiles.value >> 31)
        G = T // 4                                                       # groups of four per tile
        W = max(1, T // 512) if octets else T // 256                     # words per ray block: 2 (octets) or 4 (groups) bits per fragment
        words = np.zeros(n_pad * t * 2 * W, dtype=np.uint32)
        tri = np.zeros(n_pad * t * 2 * (T // 64), dtype=np.uint32) if per_triangle else None
        order = np.zeros(t * T, dtype=np.int32)
        self._check(self._L.sphip_selftest_stage1(self._h, rays.ctypes.data, n_pad, words.ctypes.data, tri.ctypes.data if per_triangle else None,
                                                  order.ctypes.data, C.byref(tiles)), "sphip_selftest_stage1")
        nb = n_pad // 64
        # words[(64 b + l), tile, rb, w], bit 31 - k, ray 64 b + (l & 31) + 32 rb:
        #   group bits:  k = 4 f + j <-> group 8 (8 w + f) + 2 j + (l >> 5) = 64 w + 2 k + (l >> 5)
        #   octet bits:  k = 2 f + q <-> groups g = 8 (16 w + f) + 4 q + (l >> 5) = 128 w + 4 k + (l >> 5) and g + 2
        w = words.reshape(nb, 2, 32, t, 2, W)                            # [block, half, column, tile, rb, word]
        bits = ((w[..., None] >> (31 - np.arange(32, dtype=np.uint32))) & 1).astype(bool)     # [..., k]
        wi, k = np.meshgrid(np.arange(W), np.arange(32), indexing="ij")
        surv = np.zeros((nb, 64, t, G), dtype=bool)                      # [block, ray in block, tile, group of four]
        for hh in range(2):
            g0 = ((128 * wi + 4 * k if octets else 64 * wi + 2 * k) + hh).reshape(-1)
            keep = g0 + (2 if octets else 0) < G                         # (a 256-triangle tile with octet bits uses the upper half of its one word)
            for rb in range(2):
                b = bits[:, hh, :, :, rb].reshape(nb, 32, t, W * 32)[..., keep]
                surv[:, 32 * rb:32 * rb + 32, :, g0[keep]] = b
                if octets:
                    surv[:, 32 * rb:32 * rb + 32, :, g0[keep] + 2] = b
        surv = np.repeat(surv.reshape(n_pad, t * G), 4, axis=1)          # per stream position
        tsurv = None
        if per_triangle:
            # tri[(64 b + l), tile, rb, q]: bit 31 - (16 (f & 1) + 4 j + i), f = 2 q + (bit >= 16) <-> triangle 32 f + 8 j + 4 (l >> 5) + i
            Q = T // 64
            tw = tri.reshape(nb, 2, 32, t, 2, Q)
            tb = ((tw[..., None] >> (31 - np.arange(32, dtype=np.uint32))) & 1).astype(bool)   # [block, half, column, tile, rb, q, bit]
            tsurv = np.zeros((nb, 64, t, T), dtype=bool)
            q, bit = np.meshgrid(np.arange(Q), np.arange(32), indexing="ij")
            f, j, i = 2 * q + bit // 16, (bit % 16) // 4, bit % 4
            for hh in range(2):
                pos = (32 * f + 8 * j + 4 * hh + i).reshape(-1)
                for rb in range(2):
                    tsurv[:, 32 * rb:32 * rb + 32, :, pos] = tb[:, hh, :, :, rb].reshape(nb, 32, t, Q * 32)
            tsurv = tsurv.reshape(n_pad, t * T)[:n]
        return surv[:n], tsurv, order

    def selftest_retest(self, rays):
        """sphip_selftest_retest (test-only): the re-test of stage 2 of the default scan alone for the given rays (padded to a multiple
        of 64) against every triangle of the stream.  Returns (survives, order, T): survives[ray, stream position] bool, order[stream
        position] = triangle index (n_tris = padding), T = triangles per tile of the shape that ran."""
        import numpy as np
        rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 6)
        n = rays.shape[0]
        n_pad = (n + 63) // 64 * 64
        if n_pad != n:
            rays = np.concatenate([rays, np.repeat(rays[-1:], n_pad - n, axis=0)])
        tiles = C.c_uint32(0)
        self._check(self._L.sphip_selftest_retest(self._h, None, 0, None, None, C.byref(tiles)), "sphip_selftest_retest")
        t, T = tiles.value & 0xFFFFF, (tiles.value >> 20) & 0x7FF
        bits = np.zeros(n_pad * t * (T // 4), dtype=np.uint8)
        order = np.zeros(t * T, dtype=np.int32)
        self._check(self._L.sphip_selftest_retest(self._h, rays.ctypes.data, n_pad, bits.ctypes.data, order.ctypes.data, C.byref(tiles)),
                    "sphip_selftest_retest")
        # bits[ray, tile, group]: bit 3 - u = place u of the group
        surv = ((bits.reshape(n_pad, t * (T // 4), 1) >> (3 - np.arange(4, dtype=np.uint8))) & 1).astype(bool).reshape(n_pad, t * T)
        return surv[:n], order, T

    def stats(self) -> dict:
        s = Stats()
        self._check(self._L.sphip_get_stats(self._h, C.byref(s)), "sphip_get_stats")
        return s.as_dict()
