"""What every module of the numpy replay stands on: the f32 type, the header's constants, the rounded-step dot and cross products, and
the oracle's device math (the Philox draws, the diffuse direction).  A leaf: the step modules (tests/dielectric_model.py,
env_model.py, glossy_model.py) import it, tests/path_model.py imports them and re-exports these names.

Not a test module."""
import numpy as np

from oracle import oracle as O

F = np.float32
INV_PI = np.array([0x3EA2F983], np.uint32).view(F)[0]
INV_P = np.array([0x40C90FDB], np.uint32).view(F)[0]
MARGIN = F(1.0 - 2.0 ** -10)
TWO_PI = F(2.0 * np.pi)
PI_SQ = F(np.pi * np.pi)
TWO_OVER_PI = F(2.0 / np.pi)


def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _philox(seed, pix, smp, depth):
    n = pix.size
    q = np.zeros((n, 5), np.uint32)
    q[:, 0], q[:, 1] = seed & 0xFFFFFFFF, seed >> 32
    q[:, 2], q[:, 3], q[:, 4] = pix, smp, depth
    r = O.device_math(2, q, n).reshape(n, 2)
    return r[:, 0], r[:, 1]


def _unit_vec(n, r1, r2):
    q = np.zeros((n.shape[0], 5), np.float64)
    q[:, :3], q[:, 3], q[:, 4] = n, r1, r2
    return O.device_math(3, q, n.shape[0]).reshape(-1, 3)


def _u(sxz, dist2, cos_y, ipdf):
    """mis_u: u = p_l / q, a NaN quotient (0/0, inf/inf) counting as 0"""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        u = ((PI_SQ * sxz) * dist2) / (cos_y * ipdf)
    return np.where(np.isnan(u), F(0), u).astype(F)
