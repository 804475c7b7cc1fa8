"""Smooth shading (include/spath_hip.h: SPHIP_FLAG_SMOOTH with sphip_set_vertex_normals): per-vertex normals
beside the scene; every hit shades with the normal interpolated at the hit point, the stored normal guards the surface's upper side.

The arithmetic is stated operation by operation in the header, so it is replayed in numpy (tests/path_model.py with normals `vn`):
the four rules bary/interp, diffuse, mirror and light in f32 in the stated order.  STATED TOLERANCE: 0 -- images, means, scan
counts, G-buffer normals and the selftest bit for bit.  The one statistical bar (plain against NEE|MIS under the flag) is the
project's: |z| < 4 for the image and < 5 in every cell of a 4 x 4 grid over 16 seeds x 256 spp at 32 x 32, for two disjoint seed
sets, as tests/test_hip_specular.py::test_unbiased_plain_vs_mis.

CPU part: the flag and the symbols; scene.vertex_normals, scene.icosphere and the normals file; the model by hand; a table of zeros
and a table of the stored normals against the model without normals; the coverage of the replay cases; the null-context contract.
GPU part: selftest 7; the replay for variants 1 and 16, both estimators, three scenes, with and without a specular table; variant
16 in both workgroup shapes; zero table = no flag; the BVH's parity; the G-buffer; the compositions; plain against NEE|MIS; the
error contract; the front ends."""
import ctypes as C
import os

import numpy as np
import pytest

import hip_checks as hc
import path_model
from bvh_model import noise_accept_share
from hip_checks import (E_INVALID, E_STATE, ESTIMATORS, NEE_MIS, REPLAY_SEED, SPP, H, W, _torch_first, shape,  # noqa: F401
                        smooth_case as _case)                                               # (_torch_first, shape: fixtures)
from oracle import oracle as O
from path_model import F, _bits, _dot, shade_normal
from spath_amd import capi, scene, view

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMOOTH = capi.FLAG_SMOOTH
SPEC = capi.FLAG_SPECULAR
SCENES = hc.SMOOTH_SCENES
_MODEL = {}


def _model(name, mixed, est):
    """the replay's reference, computed once per case"""
    key = (name, mixed, est)
    if key not in _MODEL:
        t, m, s, vn = _case(name, mixed)
        fn = []
        _MODEL[key] = path_model.render(hc.rays(), t, m, SPP, REPLAY_SEED, est, s, vn, first_ns=fn, collect=("accepts",)) + (fn[0],)
    return _MODEL[key]


def _covered(info, name, mixed, mis):
    """a replay case proves something only where its rules fire, so every share is asserted > 0 wherever it can be non-zero.  The
    smooth triangles are the sphere's 80 in the sphere scenes and all 200 in the room.  A share is structurally zero, and only then
    left out, in these cases:
    ended_diffuse -- the mirror sphere, with and without the mixed table elsewhere: its smooth triangles keep p = 1, so no smooth hit
                     has a diffuse lobe;
    ended_mirror  -- a case without a mixed table whose smooth triangles have p = 0 (the diffuse sphere, the room): no mirror lobe;
    lights_cut    -- the plain estimator draws no light sample; a pure mirror hit (p = 1) draws none either, and every other
                     triangle of the mirror-sphere scene is flat; in the convex room no emitter lies below a wall's plane (the panel is
                     in front of every wall) and an isolated clutter triangle has ns = n up to rounding, so the guard cannot fire.
                     The diffuse sphere's silhouette under NEE|MIS is where it does."""
    assert info["sm"] > 0, info
    if name != "mirror_sphere":
        assert info["ended_diffuse"] > 0, info
    if mixed or name == "mirror_sphere":
        assert info["ended_mirror"] > 0, info
    if mis and name == "diffuse_sphere":
        assert info["lights_cut"] > 0, info
    if not mis:
        assert info["lights"] == 0 and info["lights_cut"] == 0, info


# ---------------------------------------------------------------------------------------------------------------- CPU part
def test_flag_value_and_symbols():
    assert capi.FLAG_SMOOTH == 0x4000
    assert capi.FLAG_SMOOTH & (capi.FLAG_NEE | capi.FLAG_MIS | capi.FLAG_ACCEL | capi.FLAG_PRIMARY_REUSE | capi.FLAG_CAMERA_SAMPLES |
                               capi.FLAG_SPECULAR | 0xFF | 0xFF0000) == 0
    assert {"sphip_set_vertex_normals", "sphip_set_vertex_normals_device"} <= set(capi.SYMBOLS)
    lib = C.CDLL(capi.LIB_PATH)
    assert hasattr(lib, "sphip_set_vertex_normals") and hasattr(lib, "sphip_set_vertex_normals_device")
    assert capi.load().sphip_abi_version() == 3
    hdr = open(os.path.join(ROOT, "include", "spath_hip.h")).read()
    assert "SPHIP_FLAG_SMOOTH = 0x4000" in hdr


def test_null_context_is_refused():
    """the error contract that needs no device: a null context is SPHIP_E_INVALID for both forms"""
    L = capi.load()
    vn = np.zeros(9, F)
    assert L.sphip_set_vertex_normals(None, None) == -1
    assert L.sphip_set_vertex_normals(None, vn.ctypes.data) == -1
    assert L.sphip_set_vertex_normals_device(None, None, None) == -1


@pytest.mark.parametrize("subdiv", [0, 1, 2])
def test_icosphere_and_vertex_normals(subdiv):
    centre, radius = np.array([0.3, -0.2, 1.5]), 0.7
    t, m = scene.icosphere(subdiv, centre, radius, (0.1, 0.2, 0.3, 0, 0, 0.5))
    n = 20 * 4 ** subdiv
    assert t.shape == (n, 12) and m.shape == (n, 6) and t.dtype == F and m.dtype == F
    assert np.array_equal(m, np.tile(np.array([0.1, 0.2, 0.3, 0, 0, 0.5], F), (n, 1)))
    assert np.array_equal(_bits(t), _bits(scene.flat_normals(t)))
    v = t[:, :9].reshape(n, 3, 3).astype(np.float64)
    assert np.abs(np.sqrt(((v - centre) ** 2).sum(2)) - radius).max() < 1e-6
    assert (np.einsum("ij,ij->i", t[:, 9:12].astype(np.float64), v.mean(1) - centre) > 0).all()          # outward
    uniq = {p.tobytes() for p in t[:, :9].reshape(-1, 3)}
    assert len(uniq) == 10 * 4 ** subdiv + 2                                                               # bitwise-shared vertices
    # on the icosahedron and its first subdivision every vertex normal is (v - centre) / radius: the faces round a vertex are
    # arranged symmetrically about its radius.  From the second subdivision on they are not (the midpoints pushed outwards
    # make unequal faces), and the area-weighted sum leans by up to a few hundredths
    vn = scene.vertex_normals(t)
    assert vn.dtype == F and vn.shape == (n, 9)
    assert np.abs(vn.reshape(n, 3, 3) - (v - centre) / radius).max() < (1e-6 if subdiv <= 1 else 0.05)
    # crease_deg = 0: the face normals
    fn = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    fn /= np.sqrt((fn * fn).sum(1))[:, None]
    assert np.array_equal(scene.vertex_normals(t, 0.0), np.tile(fn.astype(F), (1, 3)))
    # which is honoured: an index list and a mask
    part = scene.vertex_normals(t, which=[1, 5])
    assert np.flatnonzero(part.any(1)).tolist() == [1, 5] and np.array_equal(part[[1, 5]], vn[[1, 5]])
    mask = np.arange(n) % 3 == 0
    assert np.array_equal(scene.vertex_normals(t, which=mask), np.where(mask[:, None], vn, F(0)))


def test_crease_angle_splits_a_box():
    """closed_room's box: at 180 degrees a corner vertex averages its three walls, at 45 degrees every wall keeps its own normal"""
    t, _ = scene.closed_room(14)
    sharp = scene.vertex_normals(t, 45.0)
    assert np.abs(sharp - np.tile(t[:, 9:12], (1, 3))).max() < 1e-6
    soft = scene.vertex_normals(t, 180.0)
    assert np.abs(soft[:12] - np.tile(t[:12, 9:12], (1, 3))).max() > 0.3


def test_normals_file_round_trip(tmp_path):
    t, _ = scene.icosphere(1)
    vn = scene.vertex_normals(t)
    p = str(tmp_path / "n.bin")
    scene.write_vertex_normals(p, vn)
    raw = open(p, "rb").read()
    assert raw[:4] == b"SPVN" and int(np.frombuffer(raw[4:8], np.uint32)[0]) == 80 and len(raw) == 8 + 80 * 36
    assert np.array_equal(_bits(np.frombuffer(raw[8:], F).reshape(80, 9)), _bits(vn))


@pytest.mark.parametrize("est", sorted(ESTIMATORS))
def test_model_by_hand(est):
    """one mirror triangle in the plane y = 0 with p = 1, ks = (0.5, 0.25, 1), hit from straight above.  Vertex normals (1, 2, 0) turn
    the reflection into (0.8, 0.6, 0), which reaches the emitter in the plane x = 2 that the flat normal's reflection (straight up)
    misses: exactly ks * E against 0 without the table.  Vertex normals (2, 1, 0) send it to (0.8, -0.6, 0), below the surface: the
    path ends after the first hit, which keeps its own emission"""
    t, m, s, rays = hc.hand_scene()
    rays = rays[2:3]
    vn = np.zeros((3, 9), F)
    flat, scans, _ = path_model.samples(rays, t, m, 7, 0, 3, est, s, vn)
    assert not flat.any() and scans == 3 * 2                      # mirror, miss
    vn[0] = [1, 2, 0] * 3
    rec, scans, info = path_model.samples(rays, t, m, 7, 0, 3, est, s, vn)
    want = s[0, 0:3] * m[1, 3:6]
    for k in range(3):
        assert np.array_equal(_bits(rec[0, k]), _bits(want)), rec[0, k]
    assert scans == 3 * 3                                         # mirror, emitter, miss
    assert info["sm"] == 3 and info["hits"] == 6 and info["ended_mirror"] == 0 and info["ended_diffuse"] == 0
    vn[0] = [2, 1, 0] * 3
    m = m.copy()
    m[0, 3:6] = (0.25, 0.5, 1.0)
    rec, scans, info = path_model.samples(rays, t, m, 7, 0, 3, est, s, vn)
    for k in range(3):
        assert np.array_equal(_bits(rec[0, k]), _bits(m[0, 3:6])), rec[0, k]
    assert scans == 3 * 1 and info["ended_mirror"] == 3 and info["hits"] == 3
    # the same tilt on a diffuse triangle: some directions about ns fall below the surface and end the path there
    s = s.copy()
    s[0] = 0
    rec, scans, info = path_model.samples(np.repeat(rays, 16, 0), t, m, 7, 0, 4, est, s, vn)
    assert 0 < info["ended_diffuse"] < 64
    assert scans >= 64 + (64 - info["ended_diffuse"])


@pytest.mark.parametrize("est", sorted(ESTIMATORS))
@pytest.mark.parametrize("name", ["closed_room_200", "open_clutter_100"])
def test_zero_and_stored_normals_are_the_specular_model(name, est):
    """a table of zeros, and a table of the stored normal at all three vertices on the triangles where m / sqrtf(dot3(m, m))
    reproduces n bitwise at every hit, each reproduce the model without vertex normals bit for bit, scans included"""
    if name == "closed_room_200":
        t, m, s = hc.mixed_room()
    else:
        t, m = scene.open_clutter(100)
        s = np.zeros((100, 4), F)
    rays = hc.rays(16, 12)
    want, want_scans, _ = path_model.samples(rays, t, m, 5, 1, 3, est, s)
    rec, scans, info = path_model.samples(rays, t, m, 5, 1, 3, est, s, np.zeros((t.shape[0], 9), F))
    assert np.array_equal(_bits(rec), _bits(want)) and scans == want_scans and info["sm"] == 0
    vn = np.tile(t[:, 9:12], (1, 3))
    for _ in range(8):                                            # drop the triangles where a hit does not reproduce n, until none is left
        rec, scans, info = path_model.samples(rays, t, m, 5, 1, 3, est, s, vn, collect=("inexact",))
        if not info["inexact"]:
            break
        vn[sorted(info["inexact"])] = 0
    share = vn.any(1).mean()
    print(name, est, "share of triangles whose stored normal is reproduced:", share, "smooth hits", info["sm"], "of", info["hits"])
    # an axis-parallel stored normal (one component +-1, two zeros) is reproduced exactly whatever u and v are: 0 * x = +-0, and
    # c = fl(fl(w) + fl(u)) + fl(v) squared, rounded and rooted gives |c| back, so m / sqrtf(l2) = +-1.  Every such triangle
    # (the room's walls, floor, ceiling and panel) must therefore have stayed in; for the others rounding decides
    axis = (np.abs(t[:, 9:12]) == F(1)).sum(1) == 1
    assert vn[axis].any(1).all(), np.flatnonzero(axis & ~vn.any(1))
    assert not info["inexact"] and share >= 0.05 and info["sm"] >= 0.5 * info["hits"]
    assert np.array_equal(_bits(rec), _bits(want)) and scans == want_scans


@pytest.mark.parametrize("est", sorted(ESTIMATORS))
@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_replay_cases_are_covered(name, mixed, est):
    info = _model(name, mixed, est)[3]
    p = info["samples"]
    print(f"{name} mixed={mixed} {est}: sm {info['sm'] / info['hits']:.3f} of hits, ended diffuse {info['ended_diffuse'] / p:.4f} "
          f"mirror {info['ended_mirror'] / p:.4f} of paths, lights cut {info['lights_cut'] / max(info['lights'], 1):.4f} of {info['lights']}")
    _covered(info, name, mixed, bool(ESTIMATORS[est]))


# ---------------------------------------------------------------------------------------------------------------- GPU part
@pytest.mark.gpu
def test_selftest_shade_normal():
    """the device function the kernels call against numpy for 4096 random triangles and rays, degenerate tables included: zero rows,
    normals that cancel, a zero-area triangle, huge and tiny lengths"""
    n = 4096
    rng = np.random.default_rng(11)
    q = np.zeros((n, 24), F)
    q[:, 6:15] = rng.uniform(-1, 1, (n, 9))
    bary = rng.dirichlet((1, 1, 1), n)
    tgt = (q[:, 6:15].reshape(n, 3, 3).astype(np.float64) * bary[:, :, None]).sum(1)
    q[:, 0:3] = tgt + rng.normal(0, 2, (n, 3))
    dv = tgt - q[:, 0:3].astype(np.float64)
    q[:, 3:6] = dv / np.sqrt((dv * dv).sum(1))[:, None]
    q[:, 15:24] = rng.normal(0, 1, (n, 9))
    q[0:64, 15:24] = 0                                            # flat rows
    q[64:128, 18:21] = q[64:128, 15:18]
    q[64:128, 21:24] = -q[64:128, 15:18]                          # n1 = n0, n2 = -n0
    q[128:160, 12:15] = q[128:160, 9:12]                          # zero area: a = 0
    q[160:192, 15:24] *= F(1e25)                                  # l2 overflows
    q[192:224, 15:24] *= F(1e-25)                                 # l2 underflows
    q[224:256, 15:24] = np.tile(q[224:256, 15:18], (1, 3))        # one normal at all three vertices
    with np.errstate(all="ignore"):
        nrm = scene.flat_normals(np.concatenate([q[:, 6:15], np.zeros((n, 3), F)], 1))[:, 9:12]
        flip = _dot(nrm, q[:, 3:6]) > F(0)
        nrm[flip] = nrm[flip] * F(-1)
        u, v, ns, sm = shade_normal(q[:, 0:3], q[:, 3:6], q[:, 6:15], q[:, 15:24], nrm)
    assert 0.8 * n < sm.sum() < n - 64 and not sm[0:64].any() and not sm[160:224].any()
    c = capi.Context(0)
    got = c.selftest(7, q, n).reshape(n, 6)
    c.close()
    want = np.concatenate([u[:, None], v[:, None], ns, sm.astype(F)[:, None]], 1).astype(F)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(_bits(got)[~nan], _bits(want)[~nan])


@pytest.mark.gpu
@pytest.mark.parametrize("est", sorted(ESTIMATORS))
@pytest.mark.parametrize("variant", [1, 16])
@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_model_bit_exact(name, mixed, variant, est):
    t, m, s, vn = _case(name, mixed)
    rays = hc.rays()
    want_img, want_mean, want_scans, info, _ = _model(name, mixed, est)
    _covered(info, name, mixed, bool(ESTIMATORS[est]))
    c = hc.ctx(t, m, s, vn)
    img, mean = c.render(rays, W, H, SPP, seed=REPLAY_SEED, flags=SMOOTH | SPEC | ESTIMATORS[est] | variant, want_accum=True)
    st = c.stats()
    c.close()
    assert st["kernel_variant"] == variant
    assert np.array_equal(_bits(mean), _bits(want_mean))
    assert np.array_equal(img, want_img)
    assert st["scans_executed"] == want_scans


@pytest.mark.gpu
@pytest.mark.parametrize("est", sorted(ESTIMATORS))
@pytest.mark.parametrize("name", ["mirror_sphere", "bad_room"])
def test_both_block_shapes(shape, name, est):
    """variant 16 in its 256- and its 512-thread shape: the replay, a progressive and an adaptive split, primary-hit reuse, camera
    samples, and zero table = no flag; the tile size of the stream says which shape ran"""
    t, m, s, vn = _case(name, True)
    c = hc.ctx(t, m, s, vn)
    hc.check_both_block_shapes(c, shape, ESTIMATORS[est] | 16 | SPEC, SMOOTH, _model(name, True, est)[:3],
                               lambda c: c.set_vertex_normals(np.zeros_like(vn)))
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("est", sorted(ESTIMATORS))
@pytest.mark.parametrize("spec", [False, True])
@pytest.mark.parametrize("variant", [1, capi.FLAG_ACCEL, 16])
def test_zero_table_is_no_flag(variant, spec, est):
    """a table of zeros: the flagged render is the unflagged one bit for bit, scans included, from rays and, with and without camera
    samples, from a camera; with and without a specular table"""
    t, m, s, vn = _case("bad_room", spec)
    rays = hc.rays()
    f = ESTIMATORS[est] | variant | (SPEC if spec else 0)
    c = hc.ctx(t, m, s if spec else None, np.zeros_like(vn))
    hc.check_zero_table_is_no_flag(c, f, SMOOTH)
    c.set_vertex_normals(vn)                                       # and the table matters
    assert not hc.same(c.render(rays, W, H, SPP, seed=6, flags=f | SMOOTH, want_accum=True), c.render(rays, W, H, SPP, seed=6, flags=f, want_accum=True))
    c.close()


@pytest.mark.parametrize("est", sorted(ESTIMATORS))
def test_accel_parity_scene_keeps_noise_accepts_rare(est):
    """the BVH against variant 16 is asked for 99 % of the pixels; the scene must not be one where the strict scan's own
    rounding-noise accepts are common.  On the CPU model of the very render test_accel_geometric_parity compares: of all hits the
    float test accepts, path rays at every depth and shadow rays alike, fewer than 1 % have their exact (double) barycentric point
    outside the triangle"""
    t = _case("diffuse_sphere", True)[0]
    info = _model("diffuse_sphere", True, est)[3]
    share, n = noise_accept_share(info["accepts"], t)
    print(f"diffuse_sphere mixed {est}: noise accepts {share:.5f} of {n} accepted hits")
    assert n >= info["hits"] and share < 0.01, (share, n)


@pytest.mark.gpu
@pytest.mark.parametrize("est", sorted(ESTIMATORS))
def test_accel_geometric_parity(est):
    """the BVH gives the same image up to its rare rounding-noise accepts: agreement in at least 99 % of the pixels (section 5.7's bar)"""
    t, m, s, vn = _case("diffuse_sphere", True)
    c = hc.ctx(t, m, s, vn)
    f = SMOOTH | SPEC | ESTIMATORS[est]
    b = hc.check_accel_parity(c, f)
    assert c.stats()["kernel_variant"] == 8
    unflagged = c.render(hc.rays(), W, H, SPP, seed=3, flags=(f & ~SMOOTH) | capi.FLAG_ACCEL, want_accum=True)[1]
    c.close()
    assert not np.array_equal(_bits(b), _bits(unflagged))


@pytest.mark.gpu
@pytest.mark.parametrize("est", sorted(ESTIMATORS))
def test_gbuffer_and_denoise(est):
    """the G-buffer's normals are the model's ns of the primary ray; dist, albedo and mat are the unflagged G-buffer's; the flagged
    G-buffer differs from the unflagged one on the sphere and equals it elsewhere; denoising repeats bit for bit"""
    t, m, s, vn = _case("diffuse_sphere", False)
    rays = hc.rays()
    f = ESTIMATORS[est] | 16
    pixn = _model("diffuse_sphere", False, est)[4]
    c = hc.ctx(t, m, s, vn)
    c.accum_begin(rays=rays, w=W, h=H, seed=REPLAY_SEED, flags=f | SMOOTH)
    c.accum_step(SPP)
    g1 = c.accum_gbuffer()
    den0, den1 = c.accum_denoise(), c.accum_denoise()
    assert den0.shape == (W * H, 4) and np.array_equal(den0, den1)
    c.accum_begin(rays=rays, w=W, h=H, seed=REPLAY_SEED, flags=f)
    c.accum_step(SPP)
    g0 = c.accum_gbuffer()
    idx, _ = O.closest_hits(rays, t, np.full(rays.shape[0], -1, np.int32))
    c.close()
    pix, ns = pixn
    first = np.unique(pix, return_index=True)[1]                  # every sample of a pixel has the same primary ray
    assert np.array_equal(_bits(g1["n"][pix[first]]), _bits(ns[first]))
    for k in ("dist", "a", "mat"):
        assert g1[k].tobytes() == g0[k].tobytes(), k
    on = idx >= 7
    differs = (_bits(g1["n"]) != _bits(g0["n"])).any(1)
    assert on.sum() > 50 and differs[on].mean() > 0.9 and not differs[~on].any()


@pytest.mark.gpu
def test_gbuffer_device_direct():
    """sphip_gbuffer_device itself: with the flag and a table it writes the accumulation's flagged G-buffer (the model's ns), without
    the flag the unflagged one although a table is set; the flag without a table is SPHIP_E_STATE and leaves the context usable"""
    import torch
    t, m, s, vn = _case("diffuse_sphere", False)
    rays = hc.rays()
    pix, ns = _model("diffuse_sphere", False, "plain")[4]
    first = np.unique(pix, return_index=True)[1]
    d_rays = torch.from_numpy(rays).to("cuda")
    st = torch.cuda.current_stream().cuda_stream

    def direct(c, flags):
        d_g = torch.zeros(W * H * 32, dtype=torch.uint8, device="cuda")
        c.gbuffer_device(d_rays.data_ptr(), W * H, d_g.data_ptr(), flags=flags, stream=st)
        torch.cuda.synchronize()
        return d_g.cpu().numpy().view(capi.gbuffer_dtype())

    c = hc.ctx(t, m)
    g0 = direct(c, 0)
    with pytest.raises(RuntimeError, match=E_STATE):
        direct(c, SMOOTH)
    assert capi.load().sphip_last_error(c._h)
    assert direct(c, 0).tobytes() == g0.tobytes()
    c.set_vertex_normals(vn)
    assert direct(c, 0).tobytes() == g0.tobytes()
    g1 = direct(c, SMOOTH)
    assert np.array_equal(_bits(g1["n"][pix[first]]), _bits(ns[first]))
    for k in ("dist", "a", "mat"):
        assert g1[k].tobytes() == g0[k].tobytes(), k
    c.accum_begin(rays=rays, w=W, h=H, seed=REPLAY_SEED, flags=16 | SMOOTH)
    c.accum_step(1)
    assert c.accum_gbuffer().tobytes() == g1.tobytes()
    c.set_vertex_normals(np.zeros_like(vn))                        # every row flat: the unflagged G-buffer
    assert direct(c, SMOOTH).tobytes() == g0.tobytes()
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("est", sorted(ESTIMATORS))
@pytest.mark.parametrize("variant", [16, 1, capi.FLAG_ACCEL])
def test_progressive_adaptive(variant, est):
    c = hc.ctx(*_case("bad_room", True))
    hc.check_progressive_adaptive_denoise(c, SMOOTH | SPEC | ESTIMATORS[est] | variant)
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("est", sorted(ESTIMATORS))
def test_reuse_chunks_multi_device(est):
    t, m, s, vn = _case("mirror_sphere", True)

    def gbuffer_is_there(mc):
        assert mc.accum_gbuffer().shape[0] == W * H
    hc.check_reuse_chunks_multi_device(t, m, SMOOTH | SPEC | ESTIMATORS[est], (16 | capi.FLAG_PRIMARY_REUSE, 1 | capi.FLAG_PRIMARY_REUSE),
                                       spec=s, vn=vn, unflag=SMOOTH, each_multi=gbuffer_is_there)


@pytest.mark.gpu
@pytest.mark.parametrize("est", sorted(ESTIMATORS))
@pytest.mark.parametrize("variant", [1, capi.FLAG_ACCEL, 16])
def test_camera_samples_and_device_table(variant, est):
    """camera samples with the flag are the chain of one-sample accumulations over sphip_camera_rays_device's rays; the normals come
    from a device pointer here"""
    t, m, s, vn = _case("mirror_sphere", True)
    c = hc.ctx(t, m, s)
    hc.set_device_table(c.set_vertex_normals_device, vn)
    hc.check_camera_samples(c, SMOOTH | SPEC | ESTIMATORS[est] | variant)
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("seed0", [100, 300])
@pytest.mark.parametrize("name", ["bad_room", "mirror_sphere"])
def test_unbiased_plain_vs_mis(name, seed0):
    """plain and NEE|MIS estimate the same image under the flag (both integrate over {w . ns > 0, w . n > 0}): the project's criterion
    and sample count, for two disjoint sets of 16 seeds"""
    t, m, s, vn = _case(name, False)
    w = h = 32
    rays = hc.rays(w, h)
    seeds = list(range(seed0, seed0 + 16))
    c = hc.ctx(t, m, s, vn)
    a = hc.seeds_means(c, rays, w, h, 256, SMOOTH | SPEC | NEE_MIS, seeds)
    b = hc.seeds_means(c, rays, w, h, 256, SMOOTH | SPEC, seeds)
    c.close()
    hc.z_grid(a, b, h, w, f"{name}: MIS vs plain under SMOOTH, seeds {seed0}..{seed0 + 15}", alike_is_zero=True)


@pytest.mark.gpu
def test_unbiased_plain_vs_mis_where_the_guard_fires():
    """the same criterion on the diffuse-sphere scene, the one case where the light sample's geometric guard fires (on the sphere's
    silhouette, test_replay_cases_are_covered): a guard that cut too much or too little would bias NEE|MIS against plain there"""
    t, m, s, vn = _case("diffuse_sphere", False)
    w = h = 32
    rays = hc.rays(w, h)
    seeds = list(range(500, 516))
    c = hc.ctx(t, m, s, vn)
    a = hc.seeds_means(c, rays, w, h, 256, SMOOTH | SPEC | NEE_MIS, seeds)
    b = hc.seeds_means(c, rays, w, h, 256, SMOOTH | SPEC, seeds)
    c.close()
    hc.z_grid(a, b, h, w, "diffuse_sphere: MIS vs plain under SMOOTH, seeds 500..515", alike_is_zero=True)


@pytest.mark.gpu
def test_error_contract():
    t, m, s, vn = _case("bad_room", False)
    rays = hc.rays()
    c = hc.ctx(t, m)
    L = capi.load()

    def refused(code, fn):
        with pytest.raises(RuntimeError, match=code):
            fn()
        assert L.sphip_last_error(c._h), "sphip_last_error is set"
        c.render(rays, W, H, 1, seed=1)                    # the context stays usable

    refused(E_STATE, lambda: c.render(rays, W, H, 2, seed=1, flags=SMOOTH))                     # flag without table
    refused(E_STATE, lambda: c.accum_begin(rays=rays, w=W, h=H, seed=1, flags=SMOOTH))
    c.set_vertex_normals(vn)
    good = c.render(rays, W, H, 2, seed=1, flags=SMOOTH, want_accum=True)
    refused(E_INVALID, lambda: c.render(rays, W, H, 1, seed=1, mode=capi.MODE_FLAT, flags=SMOOTH))  # flag with FLAT
    refused(E_INVALID, lambda: c.render(rays, W, H, 2, seed=1, flags=SMOOTH | capi.FLAG_NEE))       # flag with NEE alone
    refused(E_INVALID, lambda: c.accum_begin(rays=rays, w=W, h=H, seed=1, flags=SMOOTH | capi.FLAG_NEE))
    for v in (2, 15, 9):                                                                          # the A/B scans, an unshipped variant
        refused(E_INVALID, lambda: c.render(rays, W, H, 2, seed=1, flags=SMOOTH | v))
        refused(E_INVALID, lambda: c.accum_begin(rays=rays, w=W, h=H, seed=1, flags=SMOOTH | v))
    # hit queries ignore the flag
    import torch
    d_rays = torch.from_numpy(rays).to("cuda")
    d_idx = [torch.zeros(W * H, dtype=torch.int32, device="cuda") for _ in range(2)]
    d_d = [torch.zeros(W * H, dtype=torch.float32, device="cuda") for _ in range(2)]
    for k, fl in enumerate((0, SMOOTH)):
        c.closest_hit_device(d_rays.data_ptr(), W * H, d_idx[k].data_ptr(), d_d[k].data_ptr(), flags=fl)
    torch.cuda.synchronize()
    assert torch.equal(d_idx[0], d_idx[1]) and torch.equal(d_d[0], d_d[1])
    for col, bad in ((0, np.nan), (4, np.inf), (8, -np.inf)):                                      # non-finite values
        vb = vn.copy()
        vb[40, col] = bad
        vb[90, col] = bad
        with pytest.raises(RuntimeError, match=E_INVALID) as e:
            c.set_vertex_normals(vb)
        assert "triangle 40 " in str(e.value), str(e.value)
        assert hc.same(c.render(rays, W, H, 2, seed=1, flags=SMOOTH, want_accum=True), good)         # the table stays as it was
    # without the flag the table is ignored
    c.set_vertex_normals(None)
    refused(E_STATE, lambda: c.render(rays, W, H, 2, seed=1, flags=SMOOTH))                     # NULL cleared it
    unflagged = c.render(rays, W, H, 2, seed=1, want_accum=True)
    c.set_vertex_normals(vn)
    assert hc.same(c.render(rays, W, H, 2, seed=1, want_accum=True), unflagged)
    assert not hc.same(good, unflagged)
    # set_scene clears the table
    c.set_scene(t, m)
    refused(E_STATE, lambda: c.render(rays, W, H, 2, seed=1, flags=SMOOTH))
    # the setter ends an accumulation, in the same way and with the same code as set_scene does
    c.set_vertex_normals(vn)
    c.accum_begin(rays=rays, w=W, h=H, seed=1, flags=SMOOTH)
    c.accum_step(2)
    c.set_scene(t, m)
    with pytest.raises(RuntimeError, match=E_STATE) as by_scene:
        c.accum_step(2)
    c.set_vertex_normals(vn)
    c.accum_begin(rays=rays, w=W, h=H, seed=1, flags=SMOOTH)
    c.accum_step(2)
    c.set_vertex_normals(vn)
    with pytest.raises(RuntimeError, match=E_STATE) as by_setter:
        c.accum_step(2)
    assert str(by_setter.value) == str(by_scene.value)
    assert hc.same(c.render(rays, W, H, 2, seed=1, flags=SMOOTH, want_accum=True), good)
    c.close()
    # table before scene
    c = capi.Context(0)
    with pytest.raises(RuntimeError, match=E_STATE):
        c.set_vertex_normals(vn)
    with pytest.raises(RuntimeError, match=E_STATE):
        c.set_vertex_normals_device(0)
    assert L.sphip_last_error(c._h)
    c.set_scene(t, m)
    c.set_vertex_normals(vn)
    assert hc.same(c.render(rays, W, H, 2, seed=1, flags=SMOOTH, want_accum=True), good)
    c.close()
    # the device-pointer form on a multi-device context; a multi-device accumulation ended by the setter
    mc = capi.Context.multi([0, 0])
    mc.set_scene(t, m)
    with pytest.raises(RuntimeError, match=E_STATE):
        mc.set_vertex_normals_device(0)
    assert L.sphip_last_error(mc._h)
    with pytest.raises(RuntimeError, match=E_STATE):
        mc.render(rays, W, H, 2, seed=1, flags=SMOOTH)
    mc.set_vertex_normals(vn)
    assert hc.same(mc.render(rays, W, H, 2, seed=1, flags=SMOOTH, want_accum=True), good)
    mc.accum_begin(rays=rays, w=W, h=H, seed=1, flags=SMOOTH)
    mc.accum_step(1)
    mc.set_vertex_normals(vn)
    with pytest.raises(RuntimeError, match=E_STATE):
        mc.accum_step(1)
    mc.accum_begin(rays=rays, w=W, h=H, seed=1, flags=SMOOTH)
    img, mean, _ = mc.accum_step(2, want_mean=True)
    assert hc.same((img, mean), good)
    mc.close()


@pytest.mark.gpu
def test_cli_and_adapter(tmp_path):
    """spath_cli --normals FILE goes through hip_renderer::set_vertex_normals and gives the C ABI's bytes, one-shot, progressive, with
    --mis, with --spec and on the camera path; the flat pass is unchanged; a table of the wrong size, a missing file and --nee alone
    are refused; the Python renderer mirrors the adapter"""
    import subprocess
    cli = os.path.join(ROOT, "spath_amd", "host", "build", "spath_cli")
    t, m, s, vn = _case("mirror_sphere", False)
    sp, ss, sn = str(tmp_path / "s.bin"), str(tmp_path / "s.spec"), str(tmp_path / "s.vn")
    scene.write_scene(sp, t, m)
    scene.write_specular(ss, s)
    scene.write_vertex_normals(sn, vn)
    w, h = 40, 24
    cam = view.Camera(w, h)
    rays = np.ascontiguousarray(cam.get_viewport(), dtype=F)
    c = hc.ctx(t, m, s, vn)
    smooth = c.render(rays, w, h, 8, seed=9, flags=SMOOTH)
    smooth_spec = c.render(rays, w, h, 8, seed=9, flags=SMOOTH | SPEC)
    smooth_mis = c.render(rays, w, h, 8, seed=9, flags=SMOOTH | NEE_MIS)
    smooth_aa = c.render_camera(cam, 8, seed=9, flags=SMOOTH | capi.FLAG_CAMERA_SAMPLES)
    plain = c.render(rays, w, h, 8, seed=9)
    flat = c.render(rays, w, h, 1, mode=capi.MODE_FLAT)
    c.close()
    assert len({smooth.tobytes(), smooth_spec.tobytes(), smooth_mis.tobytes(), smooth_aa.tobytes(), plain.tobytes()}) == 5
    base = [cli, "--scene", sp, "--w", str(w), "--h", str(h), "--spp", "8", "--seed", "9"]
    for extra, want in ((["--normals", sn], smooth), (["--normals", sn, "--progressive", "3"], smooth), (["--normals", sn, "--mis"], smooth_mis),
                        (["--normals", sn, "--spec", ss], smooth_spec), (["--normals", sn, "--aa"], smooth_aa),
                        (["--normals", sn, "--mode", "flat"], flat), ([], plain)):
        out = str(tmp_path / "o.rgba")
        subprocess.run(base + ["--out", out] + extra, check=True, capture_output=True, timeout=120)
        assert open(out, "rb").read() == want.tobytes(), extra
    scene.write_vertex_normals(str(tmp_path / "short.vn"), vn[:50])
    for bad in (["--normals", str(tmp_path / "short.vn")], ["--normals", str(tmp_path / "none.vn")], ["--normals", ss], ["--normals", sn, "--nee"]):
        r = subprocess.run(base + ["--out", str(tmp_path / "x.rgba")] + bad, capture_output=True, timeout=120)
        assert r.returncode != 0, bad
    from spath_amd import renderer
    r = renderer.HipRenderer(w, h, seed=9)                # the table turns the flag on, as in the adapter; the flat pass stays
    r.set_vertex_normals(vn)
    out = renderer.Bitmap()
    r.render(renderer.Viewport(w, h, rays), t, m, t.shape[0], 8, out)
    assert np.asarray(out.values).tobytes() == smooth.tobytes()
    r.render_flat(renderer.Viewport(w, h, rays), t, m, t.shape[0], 1, out)
    assert np.asarray(out.values).tobytes() == flat.tobytes()
    r.set_specular(s)
    r.render(renderer.Viewport(w, h, rays), t, m, t.shape[0], 8, out)
    assert np.asarray(out.values).tobytes() == smooth_spec.tobytes()
    r.set_specular(None)
    r.set_vertex_normals(None)
    r.render(renderer.Viewport(w, h, rays), t, m, t.shape[0], 8, out)
    assert np.asarray(out.values).tobytes() == plain.tobytes()
    r.close()
