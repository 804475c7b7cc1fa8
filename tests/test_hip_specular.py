"""Specular reflection (include/spath_hip.h: SPHIP_FLAG_SPECULAR with sphip_set_specular): a per-triangle table
ks.r ks.g ks.b p; a hit takes the mirror lobe with probability p and the unchanged diffuse lobe otherwise.

The estimator is stated operation by operation in the header, so it is replayed in numpy (tests/path_model.py with a table `spec`).
STATED TOLERANCE: 0 -- images, means and scan counts bit for bit.  The one statistical bar (unbiasedness in p, and plain against
NEE|MIS on a mirror scene) is the project's: |z| < 5 in every cell of a 4 x 4 grid over 16 seeds x 256 spp, as
tests/test_hip_mis.py::test_unbiased.

CPU part: the flag and the symbols; the model by hand on a three-triangle scene and, with a table of zeros, against the model
without a table and the oracle's plain render; the coverage the replay cases need; scene.specular_table; what sphip_set_specular
checks without a device.
GPU part: the replay for variants 1, 2, 15, 16, both estimators and three scenes; zero table = no flag for every shipped variant;
variant 16 in both workgroup shapes (forced as tests/test_hip_shapes.py does);
the BVH's geometric parity; composition with progressive and adaptive accumulation, denoising, chunks, primary-hit reuse,
multi-device contexts and camera samples; unbiasedness; the error contract; the front ends."""
import ctypes as C
import os

import numpy as np
import pytest

import hip_checks as hc
import path_model
from hip_checks import (E_INVALID, E_STATE, ESTIMATORS, NEE_MIS, REPLAY_SEED, SPP, H, W, _torch_first, mixed_room,  # noqa: F401
                        shape)                                                              # (_torch_first, shape: fixtures)
from oracle import oracle as O
from path_model import F, _bits
from spath_amd import capi, scene, view

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPEC = capi.FLAG_SPECULAR
SCENES = hc.SPECULAR_SCENES


def _covered(info, mis):
    """a replay case proves something only if at least 10 % of its samples take a specular bounce and then hit something and, under
    MIS, at least one reaches an emitter directly after a specular bounce"""
    assert info["spec_then_hit"] >= 0.1 * info["samples"], info
    if mis:
        assert info["emitter_after_spec"] >= 1, info


# ---------------------------------------------------------------------------------------------------------------- CPU part
def test_flag_value_and_symbols():
    assert capi.FLAG_SPECULAR == 0x2000
    assert capi.FLAG_SPECULAR & (capi.FLAG_NEE | capi.FLAG_MIS | capi.FLAG_ACCEL | capi.FLAG_PRIMARY_REUSE | capi.FLAG_CAMERA_SAMPLES |
                                 0xFF | 0xFF0000) == 0
    assert {"sphip_set_specular", "sphip_set_specular_device"} <= set(capi.SYMBOLS)
    lib = C.CDLL(capi.LIB_PATH)
    assert hasattr(lib, "sphip_set_specular") and hasattr(lib, "sphip_set_specular_device")
    assert capi.load().sphip_abi_version() == 3
    hdr = open(os.path.join(ROOT, "include", "spath_hip.h")).read()
    assert "SPHIP_FLAG_SPECULAR = 0x2000" in hdr


def test_null_context_is_refused():
    """what sphip_set_specular checks without a device: a null context is SPHIP_E_INVALID for both forms"""
    L = capi.load()
    spec = np.zeros(4, F)
    assert L.sphip_set_specular(None, None) == -1
    assert L.sphip_set_specular(None, spec.ctypes.data) == -1
    assert L.sphip_set_specular_device(None, None, None) == -1


@pytest.mark.parametrize("est", sorted(ESTIMATORS))
def test_model_by_hand(est):
    """a pure mirror ks = (0.5, 0.25, 1), p = 1 in front of one emitter E: exactly ks * E for the ray that reflects into it, 0 for the
    rays that reflect past it, under both estimators (no hit is diffuse, so no shadow ray is drawn), with the scans and the coverage
    counts that follow: per sample ray 0 scans mirror, emitter, miss; ray 1 mirror, black triangle, miss; ray 2 mirror, miss"""
    t, m, s, rays = hc.hand_scene()
    rec, scans, info = path_model.samples(rays, t, m, 7, 0, 3, est, spec=s)
    want = s[0, 0:3] * m[1, 3:6]
    assert list(want) == [F(1.0), F(0.75), F(0.75)]
    for k in range(3):
        assert np.array_equal(_bits(rec[0, k]), _bits(want)), rec[0, k]
    assert not rec[1:].any()
    # rays 0 and 1 hit something after the mirror, ray 2 does not; ray 0 alone reaches the emitter, straight from the mirror
    assert (info["spec_then_hit"], info["emitter_after_spec"], info["samples"]) == (6, 3, 9)
    assert scans == 3 * (3 + 3 + 2)


@pytest.mark.parametrize("name", ["closed_room_200", "open_clutter_100"])
def test_zero_table_is_the_old_models(name):
    """with a table of zeros the model is the model without a table, under both estimators, and the plain one is the oracle's
    counter-RNG render: bit for bit, scans included"""
    t, m = {"closed_room_200": lambda: scene.closed_room(200), "open_clutter_100": lambda: scene.open_clutter(100)}[name]()
    rays = hc.rays(16, 12)
    z = np.zeros((t.shape[0], 4), F)
    z[:, 0:3] = 0.4                                       # ks alone changes nothing
    img, mean, scans, info = path_model.render(rays, t, m, 3, 5, "plain", spec=z)
    want_img, want_mean, want_scans = O.render_counter(rays, t, m, 3, 5)
    assert np.array_equal(_bits(mean), _bits(want_mean)) and np.array_equal(img, want_img) and scans == want_scans
    assert info["spec_then_hit"] == 0
    for est in sorted(ESTIMATORS):
        rec, scans, _ = path_model.samples(rays, t, m, 5, 1, 3, est, spec=z)
        want, want_scans, _ = path_model.samples(rays, t, m, 5, 1, 3, est)
        assert np.array_equal(_bits(rec), _bits(want)) and scans == want_scans, est


@pytest.mark.parametrize("est", sorted(ESTIMATORS))
@pytest.mark.parametrize("name", sorted(SCENES))
def test_replay_cases_are_covered(name, est):
    t, m, s = SCENES[name]()
    *_, info = path_model.render(hc.rays(), t, m, SPP, REPLAY_SEED, est, spec=s)
    print(name, est, info)
    _covered(info, est == "mis")


def test_specular_table_rule():
    t, m = scene.closed_room(50)
    ks = (0.6, 0.3, 0.1)
    s = scene.specular_table(t, m, ks)
    assert s.dtype == F and s.shape == (50, 4)
    k64 = np.asarray(ks, F).astype(np.float64)
    sk = (k64[0] + k64[1]) + k64[2]
    r64 = m[:, 0:3].astype(np.float64)
    r = (r64[:, 0] + r64[:, 1]) + r64[:, 2]
    assert np.array_equal(s[:, 0:3], np.broadcast_to(np.asarray(ks, F), (50, 3)))
    assert np.array_equal(_bits(s[:, 3]), _bits((sk / (sk + r)).astype(F)))
    assert ((s[:, 3] > 0) & (s[:, 3] <= 1)).all()
    # a subset, a given p, ks = 0, no diffuse reflectance
    s = scene.specular_table(t, m, 0.5, which=[3, 7], p=0.25)
    assert np.flatnonzero(s.any(1)).tolist() == [3, 7] and list(s[3]) == [F(0.5), F(0.5), F(0.5), F(0.25)]
    assert not scene.specular_table(t, m, 0.0).any()
    m0 = m.copy()
    m0[:, 0:3] = 0
    assert (scene.specular_table(t, m0, 0.5)[:, 3] == 1).all()
    for bad in (dict(ks=-0.1), dict(ks=np.nan), dict(ks=0.5, p=1.5), dict(ks=0.5, p=-0.1)):
        with pytest.raises(ValueError):
            scene.specular_table(t, m, **bad)


# ---------------------------------------------------------------------------------------------------------------- GPU part
@pytest.mark.gpu
@pytest.mark.parametrize("est", sorted(ESTIMATORS))
@pytest.mark.parametrize("variant", [1, 2, 15, 16])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_model_bit_exact(name, variant, est):
    t, m, s = SCENES[name]()
    rays = hc.rays()
    want_img, want_mean, want_scans, info = path_model.render(rays, t, m, SPP, REPLAY_SEED, est, spec=s)
    _covered(info, est == "mis")
    c = hc.ctx(t, m, s)
    img, mean = c.render(rays, W, H, SPP, seed=REPLAY_SEED, flags=SPEC | ESTIMATORS[est] | variant, want_accum=True)
    st = c.stats()
    c.close()
    assert st["kernel_variant"] == variant
    assert np.array_equal(_bits(mean), _bits(want_mean))
    assert np.array_equal(img, want_img)
    assert st["scans_executed"] == want_scans


@pytest.mark.gpu
@pytest.mark.parametrize("est", sorted(ESTIMATORS))
@pytest.mark.parametrize("name", ["mixed_room", "facing_mirrors"])
def test_both_block_shapes(shape, name, est):
    """variant 16 in its 256- and its 512-thread shape: the replay with a non-zero table, zero table = no flag, a progressive split,
    primary-hit reuse and camera samples against the other paths; the tile size of the stream says which shape ran"""
    t, m, s = SCENES[name]()
    *want, info = path_model.render(hc.rays(), t, m, SPP, REPLAY_SEED, est, spec=s)
    _covered(info, est == "mis")
    z = s.copy()
    z[:, 3] = 0
    c = hc.ctx(t, m, s)
    hc.check_both_block_shapes(c, shape, ESTIMATORS[est] | 16, SPEC, want, lambda c: c.set_specular(z))
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("est", sorted(ESTIMATORS))
@pytest.mark.parametrize("variant", [1, 2, capi.FLAG_ACCEL, 15, 16])
def test_zero_table_is_no_flag(variant, est):
    """p = 0 everywhere (whatever ks): the flagged render is the unflagged one bit for bit, scans included, from rays and, with and
    without camera samples, from a camera"""
    t, m = scene.closed_room(200)
    z = np.zeros((t.shape[0], 4), F)
    z[:, 0:3] = 0.7
    c = hc.ctx(t, m, z)
    hc.check_zero_table_is_no_flag(c, ESTIMATORS[est] | variant, SPEC)
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("est", sorted(ESTIMATORS))
def test_accel_geometric_parity(est):
    """the BVH gives the same image up to its rare rounding-noise accepts (tests/test_hip_mis.py::test_accel_geometric_parity's rule)"""
    c = hc.ctx(*mixed_room())
    b = hc.check_accel_parity(c, SPEC | ESTIMATORS[est])
    assert c.stats()["kernel_variant"] == 8
    plain = c.render(hc.rays(), W, H, SPP, seed=3, flags=ESTIMATORS[est] | capi.FLAG_ACCEL, want_accum=True)[1]
    c.close()
    assert not np.array_equal(_bits(b), _bits(plain))


@pytest.mark.gpu
@pytest.mark.parametrize("est", sorted(ESTIMATORS))
@pytest.mark.parametrize("variant", [16, 15, 2])
def test_progressive_adaptive_denoise(variant, est):
    rays = hc.rays()
    f = SPEC | ESTIMATORS[est] | variant
    c = hc.ctx(*mixed_room())
    hc.check_progressive_adaptive_denoise(c, f)
    g1 = c.accum_gbuffer()
    c.accum_begin(rays=rays, w=W, h=H, seed=9, flags=f & ~SPEC, adaptive=(0.3, 0.05, 4))
    c.accum_step(4)
    assert c.accum_gbuffer().tobytes() == g1.tobytes()      # the G-buffer is unchanged
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("est", sorted(ESTIMATORS))
def test_reuse_chunks_multi_device(est):
    t, m, s = mixed_room()
    hc.check_reuse_chunks_multi_device(t, m, SPEC | ESTIMATORS[est], (15 | capi.FLAG_PRIMARY_REUSE, 2 | capi.FLAG_PRIMARY_REUSE), spec=s,
                                       unflag=SPEC)


@pytest.mark.gpu
@pytest.mark.parametrize("est", sorted(ESTIMATORS))
@pytest.mark.parametrize("variant", [1, 2, capi.FLAG_ACCEL, 15, 16])
def test_camera_samples_and_device_table(variant, est):
    """camera samples with the flag are the chain of one-sample accumulations over sphip_camera_rays_device's rays (as
    tests/test_hip_camera_samples.py composes them); the table comes from a device pointer here"""
    t, m, s = mixed_room()
    c = hc.ctx(t, m)
    hc.set_device_table(c.set_specular_device, s)
    hc.check_camera_samples(c, SPEC | ESTIMATORS[est] | variant)
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("est", sorted(ESTIMATORS))
def test_unbiased_in_p(est):
    """the same (rho, ks) rendered with p = 0.3 and with p = 0.7 everywhere: the difference of the means is noise; 16 seeds x 256
    spp at 32 x 32, the sample count of the MIS test"""
    t, m, s = mixed_room()
    w = h = 32
    rays = hc.rays(w, h)
    seeds = list(range(100, 116))
    res = []
    for p in (0.3, 0.7):
        sp = s.copy()
        sp[:, 3] = F(p)
        c = hc.ctx(t, m, sp)
        res.append(hc.seeds_means(c, rays, w, h, 256, SPEC | ESTIMATORS[est], seeds))
        c.close()
    hc.z_grid(res[0], res[1], h, w, f"p 0.3 vs 0.7, {est}", alike_is_zero=True)


@pytest.mark.gpu
@pytest.mark.parametrize("seed0", [100, 300])
@pytest.mark.parametrize("name", ["mirror_floor", "mixed_room"])
def test_unbiased_plain_vs_mis(name, seed0):
    """plain and NEE|MIS estimate the same image on a mirror scene (same criterion, same sample count), for two disjoint sets of 16
    seeds"""
    t, m, s = SCENES[name]()
    w = h = 32
    rays = hc.rays(w, h)
    seeds = list(range(seed0, seed0 + 16))
    c = hc.ctx(t, m, s)
    a = hc.seeds_means(c, rays, w, h, 256, SPEC | NEE_MIS, seeds)
    b = hc.seeds_means(c, rays, w, h, 256, SPEC, seeds)
    c.close()
    hc.z_grid(a, b, h, w, f"{name}: MIS vs plain, seeds {seed0}..{seed0 + 15}", alike_is_zero=True)


@pytest.mark.gpu
def test_error_contract():
    t, m, s = mixed_room()
    rays = hc.rays()
    c = hc.ctx(t, m)
    L = capi.load()

    def refused(code, fn):
        with pytest.raises(RuntimeError, match=code):
            fn()
        assert L.sphip_last_error(c._h), "sphip_last_error is set"
        c.render(rays, W, H, 1, seed=1)                    # the context stays usable

    refused(E_STATE, lambda: c.render(rays, W, H, 2, seed=1, flags=SPEC))                      # flag without table
    refused(E_STATE, lambda: c.accum_begin(rays=rays, w=W, h=H, seed=1, flags=SPEC))
    c.set_specular(s)
    good = c.render(rays, W, H, 2, seed=1, flags=SPEC, want_accum=True)
    refused(E_INVALID, lambda: c.render(rays, W, H, 1, seed=1, mode=capi.MODE_FLAT, flags=SPEC))   # flag with FLAT
    refused(E_INVALID, lambda: c.render(rays, W, H, 2, seed=1, flags=SPEC | capi.FLAG_NEE))        # flag with NEE alone
    refused(E_INVALID, lambda: c.accum_begin(rays=rays, w=W, h=H, seed=1, flags=SPEC | capi.FLAG_NEE))
    refused(E_INVALID, lambda: c.render(rays, W, H, 2, seed=1, flags=SPEC | 9))                    # an unshipped variant
    refused(E_INVALID, lambda: c.accum_begin(rays=rays, w=W, h=H, seed=1, flags=SPEC | 9))
    for col, bad in ((0, -0.5), (1, np.nan), (2, np.inf), (3, 1.5), (3, -0.25), (3, np.nan)):       # bad table values
        sb = s.copy()
        sb[40, col] = bad
        sb[90, col] = bad
        with pytest.raises(RuntimeError, match=E_INVALID) as e:
            c.set_specular(sb)
        assert "triangle 40 " in str(e.value), str(e.value)
        assert hc.same(c.render(rays, W, H, 2, seed=1, flags=SPEC, want_accum=True), good)           # the table stays as it was
    # without the flag the table is ignored
    c.set_specular(None)
    refused(E_STATE, lambda: c.render(rays, W, H, 2, seed=1, flags=SPEC))                      # NULL cleared it
    unflagged = c.render(rays, W, H, 2, seed=1, want_accum=True)
    c.set_specular(s)
    assert hc.same(c.render(rays, W, H, 2, seed=1, want_accum=True), unflagged)
    # set_scene clears the table
    c.set_scene(t, m)
    refused(E_STATE, lambda: c.render(rays, W, H, 2, seed=1, flags=SPEC))
    # set_specular ends an accumulation, in the same way and with the same code as set_scene does
    c.set_specular(s)
    c.accum_begin(rays=rays, w=W, h=H, seed=1, flags=SPEC)
    c.accum_step(2)
    c.set_scene(t, m)
    with pytest.raises(RuntimeError, match=E_STATE) as by_scene:
        c.accum_step(2)
    c.set_specular(s)
    c.accum_begin(rays=rays, w=W, h=H, seed=1, flags=SPEC)
    c.accum_step(2)
    c.set_specular(s)
    with pytest.raises(RuntimeError, match=E_STATE) as by_spec:
        c.accum_step(2)
    assert str(by_spec.value) == str(by_scene.value)
    assert hc.same(c.render(rays, W, H, 2, seed=1, flags=SPEC, want_accum=True), good)
    c.close()
    # table before scene
    c = capi.Context(0)
    with pytest.raises(RuntimeError, match=E_STATE):
        c.set_specular(s)
    with pytest.raises(RuntimeError, match=E_STATE):
        c.set_specular_device(0)
    assert L.sphip_last_error(c._h)
    c.set_scene(t, m)
    c.set_specular(s)
    assert hc.same(c.render(rays, W, H, 2, seed=1, flags=SPEC, want_accum=True), good)
    c.close()
    # the device-pointer form on a multi-device context
    mc = capi.Context.multi([0, 0])
    mc.set_scene(t, m)
    with pytest.raises(RuntimeError, match=E_STATE):
        mc.set_specular_device(0)
    assert L.sphip_last_error(mc._h)
    with pytest.raises(RuntimeError, match=E_STATE):
        mc.render(rays, W, H, 2, seed=1, flags=SPEC)
    mc.set_specular(s)
    assert hc.same(mc.render(rays, W, H, 2, seed=1, flags=SPEC, want_accum=True), good)
    mc.accum_begin(rays=rays, w=W, h=H, seed=1, flags=SPEC)
    mc.accum_step(1)
    mc.set_specular(s)                                   # ends the accumulation of a multi-device context too
    with pytest.raises(RuntimeError, match=E_STATE):
        mc.accum_step(1)
    mc.accum_begin(rays=rays, w=W, h=H, seed=1, flags=SPEC)
    img, mean, _ = mc.accum_step(2, want_mean=True)
    assert hc.same((img, mean), good)
    mc.close()


@pytest.mark.gpu
def test_cli_and_adapter(tmp_path):
    """spath_cli --spec FILE goes through hip_renderer::set_specular and gives the capi image, one-shot, progressive, with --mis and
    on the camera path; the flat pass is unchanged; a table of the wrong size, a missing file and --nee alone are refused; the
    Python renderer mirrors the adapter"""
    import subprocess
    cli = os.path.join(ROOT, "spath_amd", "host", "build", "spath_cli")
    t, m, s = mixed_room()
    sp, ss = str(tmp_path / "s.bin"), str(tmp_path / "s.spec")
    scene.write_scene(sp, t, m)
    scene.write_specular(ss, s)
    w, h = 40, 24
    cam = view.Camera(w, h)
    rays = np.ascontiguousarray(cam.get_viewport(), dtype=F)
    c = hc.ctx(t, m, s)
    spec = c.render(rays, w, h, 8, seed=9, flags=SPEC)
    spec_mis = c.render(rays, w, h, 8, seed=9, flags=SPEC | NEE_MIS)
    spec_aa = c.render_camera(cam, 8, seed=9, flags=SPEC | capi.FLAG_CAMERA_SAMPLES)
    plain = c.render(rays, w, h, 8, seed=9)
    flat = c.render(rays, w, h, 1, mode=capi.MODE_FLAT)
    c.close()
    assert len({spec.tobytes(), spec_mis.tobytes(), spec_aa.tobytes(), plain.tobytes()}) == 4
    base = [cli, "--scene", sp, "--w", str(w), "--h", str(h), "--spp", "8", "--seed", "9"]
    for extra, want in ((["--spec", ss], spec), (["--spec", ss, "--progressive", "3"], spec), (["--spec", ss, "--mis"], spec_mis),
                        (["--spec", ss, "--aa"], spec_aa), (["--spec", ss, "--mode", "flat"], flat), ([], plain)):
        out = str(tmp_path / "o.rgba")
        subprocess.run(base + ["--out", out] + extra, check=True, capture_output=True, timeout=120)
        assert open(out, "rb").read() == want.tobytes(), extra
    scene.write_specular(str(tmp_path / "short.spec"), s[:50])
    for bad in (["--spec", str(tmp_path / "short.spec")], ["--spec", str(tmp_path / "none.spec")], ["--spec", ss, "--nee"]):
        r = subprocess.run(base + ["--out", str(tmp_path / "x.rgba")] + bad, capture_output=True, timeout=120)
        assert r.returncode != 0, bad
    from spath_amd import renderer
    r = renderer.HipRenderer(w, h, seed=9)                # the table turns the flag on, as in the adapter; the flat pass stays
    r.set_specular(s)
    out = renderer.Bitmap()
    r.render(renderer.Viewport(w, h, rays), t, m, t.shape[0], 8, out)
    assert np.asarray(out.values).tobytes() == spec.tobytes()
    r.render_flat(renderer.Viewport(w, h, rays), t, m, t.shape[0], 1, out)
    assert np.asarray(out.values).tobytes() == flat.tobytes()
    r.set_specular(None)
    r.render(renderer.Viewport(w, h, rays), t, m, t.shape[0], 8, out)
    assert np.asarray(out.values).tobytes() == plain.tobytes()
    r.close()
