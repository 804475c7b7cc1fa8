"""Transparency in the numpy model (include/spath_hip.h "transparency"): the arithmetic of an interface, Snell's
law and the Fresnel reflectance in f32, and the same in float64.  tests/path_model.py's loop (its `glass` table) calls it: a hit on a
triangle whose row of the dielectric table has ior > 0 is a specular hit whose lobe is drawn against the Fresnel reflectance; it
reflects by spec_reflect or transmits by Snell's law, and the unwind adds E_d + rec_{d+1} or E_d + kt * rec_{d+1}.

Not a test module: tests/test_hip_dielectric.py holds the device function and, through path_model, the kernels to it."""
import numpy as np

from model_primitives import F, _dot


def dielectric(d, ns, ior, entering):
    """the header's statement for rays d on shading normals ns (turned against d) at interfaces of index ior, entering from the vacuum
    side or not -> (Fr, tir, nt, c); f32, every operation rounded on its own"""
    d, ns, ior = np.asarray(d, F), np.asarray(ns, F), np.asarray(ior, F)
    with np.errstate(all="ignore"):
        eta = np.where(entering, F(1) / ior, ior).astype(F)
        c = _dot(d, ns)
        ci = -c
        k = F(1) - (eta * eta) * (F(1) - ci * ci)
        tir = ~(k > F(0))
        ct = np.sqrt(k)
        a, b = eta * ci, eta * ct
        rs, rp = (a - ct) / (a + ct), (ci - b) / (ci + b)
        Fr = F(0.5) * (rs * rs + rp * rp)
        nt = d * eta[:, None] + ns * (a - ct)[:, None]
    return Fr.astype(F), tir, nt.astype(F), c.astype(F)


def dielectric64(d, ns, ior, entering):
    """Snell and Fresnel in float64 on the same f32 inputs, from the textbook forms (sines and cosines of the two angles) -> (Fr, tir, nt)"""
    d, ns, ior = np.asarray(d, F).astype(np.float64), np.asarray(ns, F).astype(np.float64), np.asarray(ior, F).astype(np.float64)
    with np.errstate(all="ignore"):
        eta = np.where(entering, 1.0 / ior, ior)                  # n_incident / n_transmitted
        ci = -(d * ns).sum(1)
        s2t = eta * eta * (1.0 - ci * ci)                          # sin^2 of the refracted angle
        tir = ~(s2t < 1.0)
        ct = np.sqrt(1.0 - s2t)
        rs = (eta * ci - ct) / (eta * ci + ct)
        rp = (ci - eta * ct) / (ci + eta * ct)
        Fr = 0.5 * (rs * rs + rp * rp)
        nt = eta[:, None] * d + (eta * ci - ct)[:, None] * ns
    return Fr, tir, nt
