"""Not a test module: a numpy restatement of the device build of the opt-in linear BVH (spath_amd/csrc/sp_bvh_build.h), f32 operation
by f32 operation in the written order, and of the walk over it (sp_bvh.h, scan_bvh).  The library is built with -ffp-contract=off and
a correctly rounded division, numpy's float32 arithmetic is IEEE, min / max are exact: the structure is reachable bit for bit.
tests/test_hip_bvh_build.py checks the model's own invariants without a GPU and the device dump against the model.

fminf / fmaxf are np.fmin / np.fmax (the other operand where one is NaN).  A tie between -0.0 and +0.0, the one case where the two could
differ, does not arise: scene bounds are taken over ordered uints, where -0.0 < +0.0, and every box coordinate has had a positive
padding added or subtracted before two of them are compared.

Also here: the float64 rule that recognises a rounding-noise accept of the strict float test."""
import numpy as np

F = np.float32
U = np.uint32
K_MAX_BIG = 256
INF = F(np.inf)


def f2ord(f):
    """float -> uint whose unsigned order is the float order (-0.0 below +0.0)"""
    b = np.asarray(f, F).view(U)
    return np.where(b & U(0x80000000), ~b, b | U(0x80000000)).astype(U)


def ord2f(o):
    o = np.asarray(o, U)
    return np.where(o & U(0x80000000), o & U(0x7fffffff), ~o).astype(U).view(F)


def _finite(v):
    with np.errstate(invalid="ignore"):
        return (v - v) == 0


def scene_meta_box(tris):
    """meta words 0..5: the box over the finite vertex coordinates as ordered uints (0xffffffff / 0 on an axis without any)"""
    v = np.asarray(tris, F).reshape(-1, 12)[:, :9].reshape(-1, 3)              # rows of xyz
    meta = np.zeros(16, U)
    for a in range(3):
        c = v[:, a]
        o = f2ord(c[_finite(c)])
        meta[a] = o.min() if o.size else U(0xffffffff)
        meta[3 + a] = o.max() if o.size else U(0)
    return meta


def scene_box(meta):
    """lo[3], ext[3], max_ext, scale of scene_box()"""
    lo, ext = np.zeros(3, F), np.zeros(3, F)
    max_ext = scale = F(0)
    for a in range(3):
        l, h = ord2f(meta[a])[()], ord2f(meta[3 + a])[()]
        if meta[a] == U(0xffffffff) or not (h >= l):
            l = h = F(0)
        lo[a] = l
        ext[a] = F(h - l)
        max_ext = np.fmax(max_ext, ext[a])
        scale = np.fmax(scale, np.fmax(np.abs(l), np.abs(h)))
    return lo, ext, F(max_ext), F(scale)


def tri_extent(tris):
    """largest side of each triangle's box; NaN / inf where a coordinate is"""
    t = np.asarray(tris, F).reshape(-1, 12)
    e = np.zeros(t.shape[0], F)
    with np.errstate(invalid="ignore"):
        for a in range(3):
            v0, v1, v2 = t[:, a], t[:, 3 + a], t[:, 6 + a]
            d = np.fmax(v0, np.fmax(v1, v2)) - np.fmin(v0, np.fmin(v1, v2))
            e = np.where((d > e) | (d != d), d, e)
    return e.astype(F)


def big_threshold(c4, c2, max_ext):
    """the ladder: 1/4 of the scene, 1/2 if that gives more than K_MAX_BIG big triangles, none if that does too"""
    return F(0.25) * max_ext if c4 <= K_MAX_BIG else (F(0.5) * max_ext if c2 <= K_MAX_BIG else INF)


def morton10(x):
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.fmin(np.fmax(x * F(1024.0), F(0)), F(1023.0)).astype(U)
    v = (v | (v << U(16))) & U(0x030000FF)
    v = (v | (v << U(8))) & U(0x0300F00F)
    v = (v | (v << U(4))) & U(0x030C30C3)
    v = (v | (v << U(2))) & U(0x09249249)
    return v


def n_leaves_for(n):
    nl = 1
    while nl * 4 < n:
        nl <<= 1
    return nl


def build(tris):
    """dict with what sphip_selftest_bvh_dump returns (n_leaves, meta, nodes, rec, idx; nodes[0] zero here, unwritten there) plus the
    intermediate results: ext (per triangle), thr, big, keys, order (the stable sort), n_big, n_tree"""
    t = np.ascontiguousarray(tris, F).reshape(-1, 12)
    n = t.shape[0]
    meta = scene_meta_box(t)
    lo, ext, max_ext, scale = scene_box(meta)
    e = tri_extent(t)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        c4 = int((~(e <= F(0.25) * max_ext)).sum())                      # NaN extents count
        c2 = int((~(e <= F(0.5) * max_ext)).sum())
        thr = big_threshold(c4, c2, max_ext)
        big = ~(e <= thr) & (thr != INF)
        code = np.zeros(n, U)
        for a in range(3):
            cen = ((t[:, a] + t[:, 3 + a]) + t[:, 6 + a]) * (F(1.0) / F(3.0))
            u = (cen - lo[a]) / ext[a] if ext[a] > 0 else np.zeros(n, F)
            code |= morton10(np.where(_finite(u), u, F(0)).astype(F)) << U(a)
    keys = np.where(big, U(0xffffffff), code).astype(U)
    order = np.argsort(keys, kind="stable")
    n_big = int(big.sum())
    n_tree = n - n_big
    meta[6], meta[7], meta[8] = c4, c2, n_big

    nl = n_leaves_for(n)
    slots = 4 * nl + K_MAX_BIG
    idx = np.full(slots, -1, np.int32)
    rec = np.zeros((slots, 12), F)
    pos = np.concatenate([np.arange(n_tree), 4 * nl + np.arange(n_big)])      # slot of order[k]
    s = t[order]
    idx[pos] = order
    with np.errstate(invalid="ignore", over="ignore"):
        rec[pos, 0:3] = s[:, 0:3]
        rec[pos, 3:6] = s[:, 3:6] - s[:, 0:3]                                 # e1, e2: one float subtraction each
        rec[pos, 6:9] = s[:, 6:9] - s[:, 0:3]

    # leaf boxes over the finite coordinates of the leaf's triangles; an empty leaf keeps its inverted box
    c = np.full((4 * nl, 3, 3), np.nan, F)
    c[:n_tree] = s[:n_tree, :9].reshape(-1, 3, 3)
    c[~_finite(c)] = np.nan
    c = c.reshape(nl, 12, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        blo = np.fmin(INF, np.fmin.reduce(c, axis=1)).astype(F)
        bhi = np.fmax(-INF, np.fmax.reduce(c, axis=1)).astype(F)
        m = np.fmax(np.fmax(np.abs(blo), np.abs(bhi)), bhi - blo)
        pad = (F(1e-5) * m + F(1e-6) * scale) + F(1e-30)
        padded = (bhi[:, 0] >= blo[:, 0])[:, None]
        blo = np.where(padded, blo - pad, blo).astype(F)
        bhi = np.where(padded, bhi + pad, bhi).astype(F)
    nodes = np.zeros((2 * nl, 8), F)
    nodes[nl:, 0:3] = blo
    nodes[nl:, 3:6] = bhi
    first = nl >> 1
    while first >= 1:                                                          # the refit, level by level
        l, r = nodes[2 * first:4 * first:2], nodes[2 * first + 1:4 * first:2]
        nodes[first:2 * first, 0:3] = np.fmin(l[:, 0:3], r[:, 0:3])
        nodes[first:2 * first, 3:6] = np.fmax(l[:, 3:6], r[:, 3:6])
        first >>= 1
    return {"n_leaves": nl, "meta": meta, "nodes": nodes, "rec": rec, "idx": idx,
            "ext": e, "thr": thr, "big": big, "keys": keys, "order": order, "n_big": n_big, "n_tree": n_tree, "max_ext": max_ext}


def same_bits(a, b):
    """float arrays equal bit for bit; two NaNs count as equal whatever their payload"""
    a, b = np.asarray(a, F), np.asarray(b, F)
    return a.shape == b.shape and bool(np.all((a.view(U) == b.view(U)) | (np.isnan(a) & np.isnan(b))))


# ---------------------------------------------------------------------------------------------------------------- the walk
def _box_hit(nd, o, inv, tbest):
    """box_hit of sp_bvh.h on float32 scalars -> (hit, tnear)"""
    with np.errstate(invalid="ignore", over="ignore"):
        x0, x1 = (nd[0] - o[0]) * inv[0], (nd[3] - o[0]) * inv[0]
        y0, y1 = (nd[1] - o[1]) * inv[1], (nd[4] - o[1]) * inv[1]
        z0, z1 = (nd[2] - o[2]) * inv[2], (nd[5] - o[2]) * inv[2]
        tmin = np.fmax(np.fmax(np.fmin(x0, x1), np.fmin(y0, y1)), np.fmax(np.fmin(z0, z1), F(0)))
        tmax = np.fmin(np.fmin(np.fmax(x0, x1), np.fmax(y0, y1)), np.fmin(np.fmax(z0, z1), tbest))
        return bool(nd[0] <= nd[3]) and bool(tmin <= tmax * F(1.00001) + F(1e-30)), tmin


def walk(bvh, pair_d, ray, src=-1, tmax=None, any_hit=False):
    """scan_bvh for one ray over a structure of build() / the dump.  pair_d(slot) -> the strict float test's value for the ray and
    the slot's record (the caller evaluates it with the oracle).  Returns (idx, d, steps, leaves) as the selftest kernel does."""
    nodes, idx, nl = bvh["nodes"], bvh["idx"], bvh["n_leaves"]
    ray = np.asarray(ray, F)
    o, dr = ray[:3], ray[3:]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        inv = (F(1.0) / dr).astype(F)
    bd = F(1e12) if tmax is None else F(tmax)
    bi = -1

    def take(j, bd, bi):
        orig = int(idx[j])
        if orig < 0 or orig == src:
            return bd, bi
        d = F(pair_d(j))
        if d > 0 and (d < bd or (d == bd and orig < bi)):
            return d, orig
        return bd, bi

    for j in range(4 * nl, 4 * nl + int(bvh["meta"][8])):
        bd, bi = take(j, bd, bi)
    if any_hit and bi >= 0:
        return bi, bd, 0, 0
    node, trail, steps, leaves = 1, 0, 0, 0
    while steps < 4 * nl + 64:
        steps += 1
        descended = False
        if node < nl:
            c0, c1 = 2 * node, 2 * node + 1
            cull = F(bd * F(1.00001))
            h0, t0 = _box_hit(nodes[c0], o, inv, cull)
            h1, t1 = _box_hit(nodes[c1], o, inv, cull)
            if h0 or h1:
                both = h0 and h1
                node = c1 if (bool(t1 < t0) if both else h1) else c0
                trail = (trail << 1) | int(both)
                descended = True
        else:
            leaves += 1
            for k in range(4):
                bd, bi = take((node - nl) * 4 + k, bd, bi)
            if any_hit and bi >= 0:
                break
        if not descended:
            found = False
            while trail:
                up = (trail & -trail).bit_length() - 1
                node >>= up
                trail >>= up
                node ^= 1
                trail ^= 1
                if _box_hit(nodes[node], o, inv, F(bd * F(1.00001)))[0]:
                    found = True
                    break
            if not found:
                break
    return bi, bd, steps, leaves


# ------------------------------------------------------------------------------------------------- noise accepts (float64)
def noise_accept(o, d, verts):
    """one (ray, triangle) pair per row, f32 inputs: True where the exact barycentric point lies outside the triangle -- u and v of
    Moeller-Trumbore recomputed in double; outside when u < 0, v < 0, u + v > 1 or the ray is parallel to the plane in double.  An accept
    of the strict float test with this property is one of the reference's rounding-noise accepts."""
    o = np.asarray(o, F).reshape(-1, 3).astype(np.float64)
    d = np.asarray(d, F).reshape(-1, 3).astype(np.float64)
    v = np.asarray(verts, F).reshape(-1, 9).astype(np.float64)
    v0, e1, e2 = v[:, 0:3], v[:, 3:6] - v[:, 0:3], v[:, 6:9] - v[:, 0:3]
    h = np.cross(d, e2)
    a = (e1 * h).sum(1)
    with np.errstate(all="ignore"):
        f = 1.0 / a
        s = o - v0
        u = f * (s * h).sum(1)
        vv = f * (d * np.cross(s, e1)).sum(1)
        return ~((u >= 0.0) & (vv >= 0.0) & (u + vv <= 1.0))


def noise_accept_share(accepts, tris):
    """the share of the float test's accepted hits that are noise accepts (tools/accel_noise_rate.py); accepts: a list of
    (origins, directions, triangle indices) -> (share, count)"""
    o = np.concatenate([a[0] for a in accepts])
    d = np.concatenate([a[1] for a in accepts])
    i = np.concatenate([a[2] for a in accepts])
    outside = noise_accept(o, d, np.asarray(tris, F).reshape(-1, 12)[i, :9])
    return float(outside.mean()), int(outside.size)
