"""Textures (include/spath_hip.h "textures"), restated in numpy: the UV of a hit, repeat addressing, the
bilinear footprint and the lerp, in f32 with every operation rounded on its own and in the header's order.  tex_lookup is the device
function of the same name (spath_amd/csrc/sp_integrator.h, selftest 12), tex_albedo what the kernels call.  bilinear64 is the float64
restatement that the f32 one is measured against.

Not a test module: tests/test_hip_texture.py holds the kernels and this model to each other."""
import numpy as np

from model_primitives import F, _cross, _dot


def hit_uv(o, d, tv, uvr):
    """rules bary and interp for rays (o, d) on triangles with vertices tv [k, 9] and UV rows uvr [k, 6] -> (s, t)"""
    with np.errstate(all="ignore"):
        v0 = tv[:, 0:3]
        e1, e2 = tv[:, 3:6] - v0, tv[:, 6:9] - v0
        h = _cross(d, e2)
        a = _dot(e1, h)
        f = F(1) / a
        sv = o - v0
        u = f * _dot(sv, h)
        q = _cross(sv, e1)
        v = f * _dot(d, q)
        w = (F(1) - u) - v
        s = (uvr[:, 0] * w + uvr[:, 2] * u) + uvr[:, 4] * v
        t = (uvr[:, 1] * w + uvr[:, 3] * u) + uvr[:, 5] * v
    return s.astype(F), t.astype(F)


def axis(s, n):
    """rules wrap and texel along one axis of n texels for finite f32 s -> (i0, i1, fx, fs)"""
    s = np.asarray(s, F)
    fs = (s - np.floor(s)).astype(F)
    fs = np.where(fs < F(1), fs, F(0)).astype(F)
    x = (fs * F(n) - F(0.5)).astype(F)
    x0 = np.floor(x).astype(F)
    fx = (x - x0).astype(F)
    i0 = x0.astype(np.int64)
    i0 = np.where(i0 < 0, i0 + n, i0)
    i1 = np.where(i0 + 1 == n, 0, i0 + 1)
    return i0, i1, fx, fs


def sample(atlas, s, t):
    """rule lerp: the bilinear sample of atlas [th, tw, 3] (texel (i, j) at [j, i]) at finite (s, t) -> c [k, 3]"""
    atlas = np.asarray(atlas, F)
    th, tw = atlas.shape[:2]
    i0, i1, fx, _ = axis(s, tw)
    j0, j1, fy, _ = axis(t, th)
    t00, t10, t01, t11 = atlas[j0, i0], atlas[j0, i1], atlas[j1, i0], atlas[j1, i1]
    fx, fy = fx[:, None], fy[:, None]
    top = (t00 + ((t10 - t00) * fx).astype(F)).astype(F)
    bot = (t01 + ((t11 - t01) * fx).astype(F)).astype(F)
    return (top + ((bot - top) * fy).astype(F)).astype(F)


def textured(uvr, s, t):
    """the row is not all zero and s, t are finite"""
    return (uvr != F(0)).any(axis=1) & np.isfinite(s) & np.isfinite(t)


def tex_lookup(atlas, o, d, tv, uvr):
    """-> (s, t, c, textured): c = 1 where the hit is not textured"""
    s, t = hit_uv(o, d, tv, uvr)
    tx = textured(uvr, s, t)
    c = np.ones((s.shape[0], 3), F)
    k = np.flatnonzero(tx)
    if k.size:
        c[k] = sample(atlas, s[k], t[k])
    return s, t, c, tx


def tex_albedo(atlas, o, d, tv, uvr, rho):
    """rho * c per channel on a textured hit, rho itself otherwise"""
    _, _, c, tx = tex_lookup(atlas, o, d, tv, uvr)
    return np.where(tx[:, None], (np.asarray(rho, F) * c).astype(F), np.asarray(rho, F)).astype(F)


def bilinear64(atlas, s, t):
    """the same filter in float64 from the f32 coordinates: what the f32 statement is an approximation of"""
    a = np.asarray(atlas, np.float64)
    th, tw = a.shape[:2]

    def ax(s, n):
        s = np.asarray(s, np.float64)
        x = (s - np.floor(s)) * n - 0.5
        x0 = np.floor(x)
        i0 = x0.astype(np.int64) % n
        return i0, (i0 + 1) % n, x - x0
    i0, i1, fx = ax(s, tw)
    j0, j1, fy = ax(t, th)
    fx, fy = fx[:, None], fy[:, None]
    top = a[j0, i0] + (a[j0, i1] - a[j0, i0]) * fx
    bot = a[j1, i0] + (a[j1, i1] - a[j1, i0]) * fx
    return top + (bot - top) * fy


def tile_atlas(colours, tile=8, across=3):
    """an atlas of tile x tile-texel tiles of the given colours [n, 3], `across` tiles per row -> [rows * tile, across * tile, 3]"""
    colours = np.asarray(colours, F)
    rows = (colours.shape[0] + across - 1) // across
    a = np.zeros((rows * tile, across * tile, 3), F)
    for k, col in enumerate(colours):
        a[(k // across) * tile:(k // across + 1) * tile, (k % across) * tile:(k % across + 1) * tile] = col
    return a
