"""Not a test module: what the tests of the opt-in linear BVH share -- the scenes that reach every branch of the build
(test_hip_bvh_build.py), the structural invariants of a built tree, the ray families, and the exact parity check of the walk
(test_hip_bvh_walk.py, test_hip_accel.py, test_hip_robustness.py).

The parity check (check_walk) holds (index, distance bits) of the walk to the C oracle ray by ray.  Where they differ, the walk's own
answer must be an accept of the strict float test, and every accept the reference would have preferred to it must be EXPLAINED by a
predicate computed from the oracle and float64 alone: it is a rounding-noise accept (bvh_model.noise_accept), a hit whose exact
barycentric point lies outside its triangle, which no bounding volume can contain."""
import numpy as np

import bvh_model
from bvh_model import F
from spath_amd import scene, view

MAX_DIST = F(1e12)                                 # the reference's miss distance
NOISE_RAY_CAP = 0.005                              # rays carrying any noise accept: below this share, or the parity check says little


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# ------------------------------------------------------------------------------------------------------------------ scenes
def _soup(rng, n, lo, hi, size):
    """n axis-aligned right triangles of the given box extent inside [lo, hi]^3"""
    p = rng.uniform(lo, hi - size, (n, 3))
    t = np.zeros((n, 12), F)
    t[:, 0:3] = p
    t[:, 3:6] = p + [size, 0, 0]
    t[:, 6:9] = p + [0, size, size * 0.5]
    return t


def _ladder_scene(n_quarter, n_half, n_small=150):
    """a scene 8 units wide with n_half triangles 5 wide (more than 1/2), n_quarter - n_half triangles 3 wide (more than 1/4 only)
    and n_small triangles 0.1 wide; two of the small ones pin the scene box to [0, 8]^3"""
    rng = np.random.default_rng(n_quarter * 1000 + n_half)
    t = np.concatenate([_soup(rng, n_small, 0.0, 8.0, 0.1), _soup(rng, n_quarter - n_half, 0.0, 8.0, 3.0), _soup(rng, n_half, 0.0, 8.0, 5.0)])
    t[0, :9] = [0, 0, 0, 0.1, 0, 0, 0, 0.1, 0.1]
    t[1, :9] = [8, 8, 8, 7.9, 8, 8, 8, 7.9, 7.9]
    return scene.flat_normals(t[rng.permutation(t.shape[0])])


def _moved(n, scale, shift):
    t = scene.closed_room(n)[0].copy()
    t[:, :9] = (t[:, :9].astype(np.float64) * scale + shift).astype(F)
    t[20, 1] = F(-0.0)
    t[21, 1] = F(0.0)
    return t


def _with(t, row, col, value):
    t = t.copy()
    t[row, col] = value
    return t


def _plane():
    rng = np.random.default_rng(31)
    t = _soup(rng, 40, -1.0, 1.0, 0.2)
    t[:, [1, 4, 7]] = F(0.25)                       # every vertex in the plane y = 0.25: that axis has no extent
    return scene.flat_normals(t)


def _dups():
    t0 = scene.default_scene()[0]
    return np.concatenate([t0, t0, t0[::-1]])


SCENES = {
    **{f"n{n}": (lambda n=n: scene.open_clutter(9)[0][:n]) for n in (1, 3, 4, 5, 8, 9)},
    "default": lambda: scene.default_scene()[0],
    **{f"closed_room_{n}": (lambda n=n: scene.closed_room(n)[0]) for n in (14, 300, 1025, 4097)},     # 4097: 2048 leaves, refit levels of several workgroups
    **{f"open_clutter_{n}": (lambda n=n: scene.open_clutter(n)[0]) for n in (7, 1500)},
    "dups": _dups,                                                               # equal centroids: equal keys, ties by index
    "plane": _plane,
    "identical": lambda: np.repeat(scene.default_scene()[0][:1], 6, axis=0),     # every triangle as wide as the scene: all big, an empty tree
    "point": lambda: np.tile(np.array([[0.5, -0.25, 2.0] * 3 + [0, 1, 0]], F), (5, 1)),   # max_ext == 0
    "moved_small_neg": lambda: _moved(300, 1e-4, -3e4),
    "moved_large_pos": lambda: _moved(300, 1e4, 3e4),
    "big_256": lambda: _ladder_scene(256, 10),                                   # exactly kBvhMaxBig wider than 1/4: they are the big list
    "big_257": lambda: _ladder_scene(257, 10),                                   # one more: the ladder moves to 1/2
    "big_none": lambda: _ladder_scene(400, 300),                                 # more than kBvhMaxBig wider than 1/2: no big list
    "inf_vertex": lambda: _with(scene.closed_room(300)[0], 20, 0, np.inf),       # set_scene takes non-finite vertices (test_hip_robustness.py)
    "nan_vertex": lambda: _with(scene.closed_room(300)[0], 21, 4, np.nan),
}
EXPECT_N_BIG = {"identical": 6, "point": 0, "big_256": 256, "big_257": 10, "big_none": 0}

_scene_cache = {}


def scene_tris(name):
    if name not in _scene_cache:
        t = np.ascontiguousarray(SCENES[name](), F)
        t.setflags(write=False)
        _scene_cache[name] = t
    return _scene_cache[name]


def mats_for(t):
    return np.full((t.shape[0], 6), 0.5, F)


# ---------------------------------------------------------------------------------------------------- structural invariants
def check_structure(tris, b, n_big_expected=None):
    """what must hold of a built structure (the model's or the device's dump), stated on its arrays alone and in plain terms"""
    t = np.asarray(tris, F).reshape(-1, 12)
    n, nl = t.shape[0], b["n_leaves"]
    idx, rec, nodes, n_big = b["idx"], b["rec"], b["nodes"], int(b["meta"][8])
    n_tree = n - n_big
    assert nl >= 1 and nl & (nl - 1) == 0 and 4 * nl >= n and (nl == 1 or 2 * nl < n) and idx.shape == (4 * nl + 256,)
    # every triangle exactly once across the tree and the big list, each part packed to the front, padding -1 with zero records
    assert np.array_equal(np.sort(idx[idx >= 0]), np.arange(n))
    assert (idx[:n_tree] >= 0).all() and (idx[n_tree:4 * nl] == -1).all()
    assert (idx[4 * nl:4 * nl + n_big] >= 0).all() and (idx[4 * nl + n_big:] == -1).all()
    assert not _bits(rec[idx < 0]).any()
    assert not _bits(rec[:, 9:]).any()
    used = idx >= 0
    s = t[idx[used]]
    with np.errstate(invalid="ignore", over="ignore"):
        want = np.concatenate([s[:, 0:3], s[:, 3:6] - s[:, 0:3], s[:, 6:9] - s[:, 0:3]], axis=1)
    assert bvh_model.same_bits(rec[used][:, :9], want)
    # the ladder: triangles wider than 1/4 (1/2) of the scene's widest side, counted one by one
    v = t[:, :9].reshape(n, 3, 3)
    fin = np.isfinite(v)
    span = [v[..., a][fin[..., a]].max() - v[..., a][fin[..., a]].min() if fin[..., a].any() else F(0) for a in range(3)]
    widest = F(max(span))                                                          # a float subtraction per axis, as the build has it
    with np.errstate(invalid="ignore"):                                            # (min and max leave a NaN coordinate out; inf - inf is NaN, which counts as wide)
        ext = (np.fmax.reduce(v, axis=1) - np.fmin.reduce(v, axis=1)).max(axis=1)
        c4, c2 = int((~(ext <= F(0.25) * widest)).sum()), int((~(ext <= F(0.5) * widest)).sum())
        thr = F(0.25) * widest if c4 <= 256 else F(0.5) * widest if c2 <= 256 else np.inf
        is_big = ~(ext <= thr) & np.isfinite(thr)
    assert (int(b["meta"][6]), int(b["meta"][7])) == (c4, c2)
    assert n_big <= 256 and n_big == int(is_big.sum()) and (n_big_expected is None or n_big == n_big_expected)
    assert np.array_equal(np.sort(idx[4 * nl:4 * nl + n_big]), np.flatnonzero(is_big))
    assert (np.diff(idx[4 * nl:4 * nl + n_big]) > 0).all()                          # equal keys: index order
    # tree order: ascending key, ties in ascending index (keys from the model: the structure does not store them)
    keys = bvh_model.build(t)["keys"]
    k, i = keys[idx[:n_tree]].astype(np.int64), idx[:n_tree].astype(np.int64)
    assert ((k[1:] > k[:-1]) | ((k[1:] == k[:-1]) & (i[1:] > i[:-1]))).all()
    # every finite vertex of a leaf's triangles inside the leaf box
    lv = np.full((4 * nl, 9), np.nan, F)
    lv[:n_tree] = t[idx[:n_tree], :9]
    lv = lv.reshape(nl, 12, 3)
    lo, hi = nodes[nl:, None, 0:3], nodes[nl:, None, 3:6]
    f = np.isfinite(lv)
    with np.errstate(invalid="ignore"):
        assert ((lv >= lo) & (lv <= hi))[f].all()
    # a leaf without a finite x coordinate, and every subtree of such leaves, is inverted; an inner node is the union of its children
    empty = ~f[:, :, 0].any(axis=1)
    assert (nodes[nl:][empty, 0] == np.inf).all() and (nodes[nl:][empty, 3] == -np.inf).all()
    first = nl >> 1
    while first >= 1:
        l, r = nodes[2 * first:4 * first:2], nodes[2 * first + 1:4 * first:2]
        assert bvh_model.same_bits(nodes[first:2 * first, 0:3], np.fmin(l[:, 0:3], r[:, 0:3]))
        assert bvh_model.same_bits(nodes[first:2 * first, 3:6], np.fmax(l[:, 3:6], r[:, 3:6]))
        empty = empty[0::2] & empty[1::2]
        assert (nodes[first:2 * first][empty, 0] == np.inf).all() and (nodes[first:2 * first][empty, 3] == -np.inf).all()
        first >>= 1
    assert not _bits(nodes[1:, 6:]).any()


# ------------------------------------------------------------------------------------------------------------- ray families
def random_rays(rng, n, box=1.4):
    o = rng.uniform(-box, box, (n, 3)) * [1, 0.5, 1]
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([o, d], axis=1).astype(F)


def mixed_rays(seed, n=2048, w=64, h=32):
    return np.concatenate([random_rays(np.random.default_rng(seed), n), view.Camera(w, h).get_viewport()])


def axis_rays(seed, n, zeros):
    """directions with `zeros` (1 or 2) components exactly zero, of either sign"""
    rng = np.random.default_rng(seed)
    r = random_rays(rng, n)
    for k in range(n):
        r[k, 3 + rng.permutation(3)[:zeros]] = F(0.0) if k % 2 else F(-0.0)
    return r


def box_origin_rays(seed, tris, n):
    """origins exactly on a face of a leaf box of the model's tree (first half) and exactly on a vertex of one (second half).
    (Vertices of the boxes, not of the triangles: a ray that starts on a triangle's vertex forms a degenerate pair with that triangle,
    a noise accept by construction -- 2.5 % of such rays on closed_room(300) -- and the family would break the cap on those.)"""
    rng = np.random.default_rng(seed)
    b = bvh_model.build(tris)
    nl = b["n_leaves"]
    boxes = b["nodes"][nl:][b["idx"][:4 * nl:4] >= 0]
    r = random_rays(rng, n)
    for k in range(n):
        bx = boxes[rng.integers(boxes.shape[0])]
        p = bx[0:3] + (bx[3:6] - bx[0:3]) * rng.uniform(0, 1, 3).astype(F)
        for a in ([rng.integers(3)] if k < n // 2 else range(3)):
            p[a] = bx[a + 3 * rng.integers(2)]
        r[k, :3] = p
    return r


def grazing_rays(seed, tris, n=4096):
    """aimed at a Dirichlet-random interior point of a random triangle, at 1e-4 .. 3e-2 rad to its plane, from 0.2 .. 2 units away"""
    rng = np.random.default_rng(seed)
    v = np.asarray(tris, F)[:, :9].reshape(-1, 3, 3).astype(np.float64)
    k = rng.integers(0, v.shape[0], n)
    p = (v[k] * rng.dirichlet([1.0, 1.0, 1.0], n)[:, :, None]).sum(axis=1)
    e1, e2 = v[k, 1] - v[k, 0], v[k, 2] - v[k, 0]
    nrm = np.cross(e1, e2)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    phi = rng.uniform(0, 2 * np.pi, (n, 1))
    u = e1 / np.linalg.norm(e1, axis=1, keepdims=True)
    w = np.cross(nrm, u)
    inpl = u * np.cos(phi) + w * np.sin(phi)
    ang = np.exp(rng.uniform(np.log(1e-4), np.log(3e-2), (n, 1))) * rng.choice([-1.0, 1.0], (n, 1))
    back = inpl * np.cos(ang) + nrm * np.sin(ang)                     # from the point back towards the origin
    o = p + back * rng.uniform(0.2, 2.0, (n, 1))
    return np.concatenate([o, -back], axis=1).astype(F)


def shadow_rays(seed, tris, emitters, rays, hit_i, hit_d):
    """from the closest-hit points of `rays` towards random points on the emitter triangles: (rays, src, distance to the point)"""
    rng = np.random.default_rng(seed)
    ok = hit_i >= 0
    r, hi, hd = rays[ok], hit_i[ok], hit_d[ok]
    x = (r[:, :3] + r[:, 3:] * hd[:, None]).astype(F)                 # o + dir * d in float, as the integrator forms it
    v = np.asarray(tris, F)[:, :9].reshape(-1, 3, 3).astype(np.float64)
    e = np.asarray(emitters)[rng.integers(0, len(emitters), x.shape[0])]
    p = (v[e] * rng.dirichlet([1.0, 1.0, 1.0], x.shape[0])[:, :, None]).sum(axis=1)
    d = p - x
    dist = np.linalg.norm(d, axis=1)
    keep = dist > 1e-6
    d = d[keep] / dist[keep, None]
    return np.concatenate([x[keep], d], axis=1).astype(F), hi[keep].astype(np.int32), dist[keep]


# ------------------------------------------------------------------------------------------------------------ exact parity
def pair_values(O, rays, tris, chunk=1 << 20):
    """the strict float test's value (distance or -1) of every (ray, triangle) pair, by the oracle: f32 [n_rays, n_tris]"""
    rays = np.asarray(rays, F).reshape(-1, 6)
    v = np.asarray(tris, F).reshape(-1, 12)[:, :9]
    n = v.shape[0]
    out = np.zeros((rays.shape[0], n), F)
    step = max(1, chunk // n)
    for a in range(0, rays.shape[0], step):
        r = rays[a:a + step]
        inp = np.concatenate([np.repeat(r, n, axis=0), np.tile(v, (r.shape[0], 1))], axis=1)
        out[a:a + step] = O.device_math(4, inp, inp.shape[0]).reshape(r.shape[0], n)
    return out


def noise_pairs(rays, tris, P):
    """of the accepts in P (pair_values), which are noise accepts: bool [n_rays, n_tris]"""
    out = np.zeros(P.shape, bool)
    r, c = np.nonzero(P > 0)
    v = np.asarray(tris, F).reshape(-1, 12)[:, :9]
    out[r, c] = bvh_model.noise_accept(rays[r, :3], rays[r, 3:], v[c])
    return out


def check_walk(O, tris, rays, walked, n_leaves, src=None, tmax=None, any_hit=False, P=None, tag=""):
    """walked = (idx, d, steps, leaves) of the walk for `rays` (closest form; with tmax the bounded form; with any_hit the shadow form).
    P: pair_values of ALL the rays if the caller has them (then the cap on rays that carry a noise accept is asserted too);
    otherwise the pairs of the differing rays are evaluated here.  Returns the counts it prints."""
    tris = np.asarray(tris, F).reshape(-1, 12)
    rays = np.asarray(rays, F).reshape(-1, 6)
    n, nt = rays.shape[0], tris.shape[0]
    wi, wd, steps, _ = walked
    assert (steps < 4 * n_leaves + 64).all(), (tag, "a walk was ended by the step bound", int(steps.max()))
    srcv = np.full(n, -1, np.int32) if src is None else np.asarray(src, np.int32)
    bound = np.full(n, MAX_DIST, F) if tmax is None else np.asarray(tmax, F)
    oi, od = O.closest_hits(rays, tris, src)
    ref_hit = (oi >= 0) & (od < bound)
    cols = np.arange(nt)
    if not any_hit:
        ri, rd = np.where(ref_hit, oi, -1), np.where(ref_hit, od, bound).astype(F)
        differ = (wi != ri) | (_bits(wd) != _bits(rd))
    else:
        differ = (wi < 0) & ref_hit                                  # a reported miss although something is in the way
        hit = np.flatnonzero(wi >= 0)
        if hit.size:                                                 # a reported hit is an accept below tmax, whichever it is
            v = tris[wi[hit], :9]
            own = O.device_math(4, np.concatenate([rays[hit], v], axis=1), hit.size)
            assert np.array_equal(_bits(own), _bits(wd[hit])) and (wd[hit] > 0).all() and (wd[hit] < bound[hit]).all() and (wi[hit] != srcv[hit]).all(), tag
        assert np.array_equal(_bits(wd[wi < 0]), _bits(bound[wi < 0])), tag
    rows = np.flatnonzero(differ)
    counts = {"rays": n, "differ": int(rows.size), "noise": 0, "unexplained": 0}
    if rows.size:
        Pd = P[rows] if P is not None else pair_values(O, rays[rows], tris)
        acc = (Pd > 0) & (cols[None, :] != srcv[rows, None]) & (Pd < bound[rows, None])
        w_i, w_d = wi[rows], wd[rows]
        if any_hit:
            below = acc
        else:
            got = w_i >= 0                                           # the walk's own answer is an accept of its triangle, or the miss
            own = Pd[np.flatnonzero(got), w_i[got]]
            assert np.array_equal(_bits(own), _bits(w_d[got])) and acc[np.flatnonzero(got), w_i[got]].all(), tag
            assert np.array_equal(_bits(w_d[~got]), _bits(bound[rows][~got])), tag
            below = acc & ((Pd < w_d[:, None]) | ((Pd == w_d[:, None]) & (cols[None, :] < w_i[:, None])))
        noise = noise_pairs(rays[rows], tris, np.where(below, Pd, F(-1)))
        counts["noise"] = int((below & noise).sum())
        counts["unexplained"] = int((below & ~noise).sum())
        bad = rows[(below & ~noise).any(axis=1)]
    print(f"{tag}: {counts}")
    assert counts["unexplained"] == 0, (tag, counts, bad[:8].tolist())
    if P is not None:
        share = float(noise_pairs(rays, tris, P).any(axis=1).mean())
        print(f"{tag}: rays that carry a noise accept among their pairs: {share:.5f}")
        assert share < NOISE_RAY_CAP, (tag, share)
    return counts
