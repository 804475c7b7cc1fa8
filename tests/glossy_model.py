"""Glossy reflection in the numpy model (include/spath_hip.h, "glossy reflection"), operation by operation: the
GGX visible-normal draw and its Smith weight in f32 (gloss_bounce), the same in float64, and the unwind's step at a glossy hit.
tests/path_model.py's loop (its `rough` table) calls them: a hit that took the mirror lobe of a triangle of roughness alpha > 0 (not an
interface) reflects about the drawn microfacet normal, and the unwind scales the mirror's term once more by the weight g.

Not a test module: tests/test_hip_glossy.py holds the device function and, through path_model, the path kernels to it at tolerance 0."""
import numpy as np

from model_primitives import F, _cross, _dot
from oracle import oracle as O

ONE, HALF, ZERO = F(1), F(0.5), F(0)
GLOSS_STREAM = 48


def _sincos(phi):
    sc = O.device_math(0, np.ascontiguousarray(phi, F), phi.size).reshape(-1, 2)
    return sc[:, 0], sc[:, 1]


def gloss_bounce(d, ns, al, u1, u2, parts=None):
    """gloss_bounce for rays d [k, 3], shading normals ns [k, 3] (turned against d), roughness al [k] and uniforms u1, u2 [k] (float64)
    -> (m, nd, g, ok).  parts: a dict that receives the intermediate vh, T1, T2, nh"""
    d, ns, al = np.ascontiguousarray(d, F), np.ascontiguousarray(ns, F), np.ascontiguousarray(al, F)
    u1, u2 = np.asarray(u1, np.float64), np.asarray(u2, np.float64)
    with np.errstate(all="ignore"):
        c = _dot(d, ns)
        nx, ny, nz = ns[:, 0], ns[:, 1], ns[:, 2]
        sg = np.where(nz < ZERO, F(-1), ONE)
        a = F(-1) / (sg + nz)
        b = (nx * ny) * a
        t = np.stack([ONE + (sg * (nx * nx)) * a, sg * b, (-sg) * nx], 1)
        bt = np.stack([b, sg + (ny * ny) * a, -ny], 1)
        v = np.stack([-_dot(d, t), -_dot(d, bt), -c], 1)
        h = np.stack([al * v[:, 0], al * v[:, 1], v[:, 2]], 1)
        vh = h / np.sqrt(_dot(h, h))[:, None]
        l2 = vh[:, 0] * vh[:, 0] + vh[:, 1] * vh[:, 1]
        ln = np.sqrt(l2)
        pos = l2 > ZERO
        T1 = np.stack([np.where(pos, -vh[:, 1] / ln, ONE), np.where(pos, vh[:, 0] / ln, ZERO), np.zeros_like(l2)], 1).astype(F)
        T2 = _cross(vh, T1)
        r = np.sqrt(u1).astype(F)
        phi = ((u2 * np.pi) * 2.0).astype(F)
        sn, cs = _sincos(phi)
        p1 = r * cs
        p2 = r * sn
        s = HALF * (ONE + vh[:, 2])
        q = ONE - p1 * p1
        q = np.where(q > ZERO, q, ZERO)
        p2 = (ONE - s) * np.sqrt(q) + s * p2
        z2 = (ONE - p1 * p1) - p2 * p2
        z = np.sqrt(np.where(z2 > ZERO, z2, ZERO))
        nh = (T1 * p1[:, None] + T2 * p2[:, None]) + vh * z[:, None]
        ne = np.stack([al * nh[:, 0], al * nh[:, 1], np.where(nh[:, 2] > ZERO, nh[:, 2], ZERO)], 1)
        ml = ne / np.sqrt(_dot(ne, ne))[:, None]
        m = (t * ml[:, 0:1] + bt * ml[:, 1:2]) + ns * ml[:, 2:3]
        cm = _dot(d, m)
        nd = (d - m * (cm + cm)[:, None]).astype(F)                # spec_reflect about m
        cl = _dot(nd, ns)
        ok = cl > ZERO
        g = (cl + cl) / (cl + np.sqrt(al * al + (ONE - al * al) * (cl * cl)))
        g = np.where(g > ONE, ONE, g)
    for x in (vh, T1, T2, nh, m, nd, g):
        assert x.dtype == F, x.dtype
    if parts is not None:
        parts.update(vh=vh, T1=T1, T2=T2, nh=nh, t=t, bt=bt)
    return m.astype(F), nd, g, ok


def gloss_bounce64(d, ns, al, u1, u2):
    """the same formulas in float64 (sin and cos numpy's), from the same f32 inputs -> (m, nd, g, cl)"""
    d, ns, al = np.asarray(d, F).astype(np.float64), np.asarray(ns, F).astype(np.float64), np.asarray(al, F).astype(np.float64)
    u1, u2 = np.asarray(u1, np.float64), np.asarray(u2, np.float64)
    dot = lambda p, q: (p * q).sum(1)
    with np.errstate(all="ignore"):
        c = dot(d, ns)
        nx, ny, nz = ns[:, 0], ns[:, 1], ns[:, 2]
        sg = np.where(nz < 0, -1.0, 1.0)
        a = -1.0 / (sg + nz)
        b = nx * ny * a
        t = np.stack([1.0 + sg * nx * nx * a, sg * b, -sg * nx], 1)
        bt = np.stack([b, sg + ny * ny * a, -ny], 1)
        v = np.stack([-dot(d, t), -dot(d, bt), -c], 1)
        h = np.stack([al * v[:, 0], al * v[:, 1], v[:, 2]], 1)
        vh = h / np.sqrt(dot(h, h))[:, None]
        l2 = vh[:, 0] ** 2 + vh[:, 1] ** 2
        ln = np.sqrt(l2)
        pos = l2 > 0
        T1 = np.stack([np.where(pos, -vh[:, 1] / ln, 1.0), np.where(pos, vh[:, 0] / ln, 0.0), np.zeros_like(l2)], 1)
        T2 = np.cross(vh, T1)
        r = np.sqrt(u1)
        phi = u2 * np.pi * 2.0
        p1, p2 = r * np.cos(phi), r * np.sin(phi)
        s = 0.5 * (1.0 + vh[:, 2])
        p2 = (1.0 - s) * np.sqrt(np.maximum(1.0 - p1 * p1, 0.0)) + s * p2
        z = np.sqrt(np.maximum(1.0 - p1 * p1 - p2 * p2, 0.0))
        nh = T1 * p1[:, None] + T2 * p2[:, None] + vh * z[:, None]
        ne = np.stack([al * nh[:, 0], al * nh[:, 1], np.maximum(nh[:, 2], 0.0)], 1)
        ml = ne / np.sqrt(dot(ne, ne))[:, None]
        m = t * ml[:, 0:1] + bt * ml[:, 1:2] + ns * ml[:, 2:3]
        cm = dot(d, m)
        nd = d - m * (cm + cm)[:, None]
        cl = dot(nd, ns)
        g = np.minimum((cl + cl) / (cl + np.sqrt(al * al + (1.0 - al * al) * cl * cl)), 1.0)
    return m, nd, g, cl


def gloss_unwind(q, e, rec, g):
    """the unwind's step at a glossy hit: E + (((ks * rec) * wS) * g)"""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        wS = (F(1) / q[:, 3])[:, None]
        return (e + ((q[:, 0:3] * rec) * wS) * g[:, None]).astype(F)


def covered(info, smooth=False):
    """a replay case proves something only where its rules fire"""
    for k in ("glossy", "ended", "two_glossy"):
        assert info[k] > 0, (k, info)
    assert info["ended"] < info["glossy"], info
    assert info["emit_after_glossy"] + info["miss_after_glossy"] > 0, info
    if smooth:
        assert info["ended_above"] > 0 and info["ended_below"] > 0, info
