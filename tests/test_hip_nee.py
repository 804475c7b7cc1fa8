"""Next-event estimation (include/spath_hip.h: SPHIP_FLAG_NEE): a light sample and one shadow (any-hit)
ray at each of the first four hits of a path.

The estimator is stated operation by operation in the header, so it is replayed in numpy (tests/path_model.py, est="nee"), the
light table in float64 like the host builds it.  STATED TOLERANCE: 0 -- images, means and scan counts bit for bit.

CPU part: the flag's value and the numpy light table on a hand-made scene.
GPU part: the replay for every shipped scan variant and scene kind; unchanged paths; composition with progressive and adaptive
accumulation, primary-hit reuse, sample chunks and multi-device contexts; unbiasedness against the plain estimator and lower
noise; the error contract."""
import os

import numpy as np
import pytest

import hip_checks as hc
import path_model
from hip_checks import E_INVALID, SPP, H, W, many_emitters, small_light_room
from path_model import F, _bits, light_table
from spath_amd import capi, scene, view

SCENES = hc.NEE_SCENES


# ---------------------------------------------------------------------------------------------------------------- CPU part
def test_flag_value():
    assert capi.FLAG_NEE == 0x400
    assert capi.FLAG_NEE & (capi.FLAG_ACCEL | capi.FLAG_PRIMARY_REUSE | 0xFF | 0xFF0000) == 0


def test_light_table_by_hand():
    """two emitters of areas 0.5 and 2 and emittance sums 3 and 1: weights 1.5 and 2, ipdf = W / Esum"""
    t = np.zeros((3, 12), F)
    t[0, :9] = [0, 0, 0, 1, 0, 0, 0, 1, 0]
    t[1, :9] = [0, 0, 0, 2, 0, 0, 0, 2, 0]
    t[2, :9] = [0, 0, 0, 1, 0, 0, 0, 1, 0]
    m = np.zeros((3, 6), F)
    m[0, 3:6] = [1, 1, 1]
    m[2, 3:6] = [0, 0.5, 0.5]
    m[1, 3:6] = 0
    idx, cdf, ipdf, Wt = light_table(t, m)
    assert list(idx) == [0, 2]
    assert list(cdf) == [1.5, 2.0] and Wt == 2.0
    assert list(ipdf) == [F(2.0 / 3.0), F(2.0)]


# ---------------------------------------------------------------------------------------------------------------- GPU part
@pytest.mark.gpu
@pytest.mark.parametrize("variant", [1, 2, 15, 16])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_model_bit_exact(name, variant):
    t, m = SCENES[name]()
    rays = hc.rays()
    want_img, want_mean, want_scans, _ = path_model.render(rays, t, m, SPP, 3, "nee")
    c = hc.ctx(t, m)
    img, mean = c.render(rays, W, H, SPP, seed=3, flags=capi.FLAG_NEE | variant, want_accum=True)
    st = c.stats()
    c.close()
    assert st["kernel_variant"] == variant
    assert np.array_equal(_bits(mean), _bits(want_mean))
    assert np.array_equal(img, want_img)
    assert st["scans_executed"] == want_scans


@pytest.mark.gpu
def test_accel_geometric_parity():
    """the BVH gives the same image up to its rare rounding-noise accepts (test_hip_accel.py's rule: almost every pixel equal)"""
    c = hc.ctx(*scene.closed_room(200))
    hc.check_accel_parity(c, capi.FLAG_NEE)
    c.close()


@pytest.mark.gpu
def test_paths_unchanged_and_isolated():
    t, m = scene.closed_room(200)
    rays = hc.rays()
    c = hc.ctx(t, m)
    plain0 = c.render(rays, W, H, SPP, seed=5, want_accum=True)[1]
    nee = c.render(rays, W, H, SPP, seed=5, flags=capi.FLAG_NEE, want_accum=True)[1]
    plain1 = c.render(rays, W, H, SPP, seed=5, want_accum=True)[1]
    nee1 = c.render(rays, W, H, SPP, seed=5, flags=capi.FLAG_NEE, want_accum=True)[1]
    flat0 = c.render(rays, W, H, 1, mode=capi.MODE_FLAT)
    flat1 = c.render(rays, W, H, 1, mode=capi.MODE_FLAT, flags=capi.FLAG_NEE)
    c.accum_begin(rays=rays, w=W, h=H, seed=5)
    c.accum_step(2)
    g0 = c.accum_gbuffer()
    c.accum_begin(rays=rays, w=W, h=H, seed=5, flags=capi.FLAG_NEE)
    c.accum_step(2)
    g1 = c.accum_gbuffer()
    c.close()
    assert np.array_equal(_bits(plain0), _bits(plain1)) and np.array_equal(_bits(nee), _bits(nee1))
    assert not np.array_equal(_bits(plain0), _bits(nee))
    assert np.array_equal(flat0, flat1)
    assert g0.tobytes() == g1.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [16, 15])
def test_progressive_and_adaptive(variant):
    c = hc.ctx(*many_emitters())
    cnt = hc.check_progressive_adaptive_denoise(c, capi.FLAG_NEE | variant)
    c.close()
    assert len(np.unique(cnt)) > 1                   # some pixels stopped early


@pytest.mark.gpu
def test_reuse_chunks_multi_device():
    hc.check_reuse_chunks_multi_device(*scene.open_clutter(100), capi.FLAG_NEE, ())


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["open_clutter_100", "small_light_room"])
def test_unbiased(name):
    """16 seeds x 256 spp of each estimator on the same paths: the difference of the means is noise (|z| < 4 for the image mean,
    < 5 in every cell of a 4 x 4 grid)"""
    t, m = scene.open_clutter(100) if name == "open_clutter_100" else small_light_room()
    w = h = 32
    rays = hc.rays(w, h)
    c = hc.ctx(t, m)
    seeds = list(range(100, 116))
    a = hc.seeds_means(c, rays, w, h, 256, capi.FLAG_NEE, seeds)
    b = hc.seeds_means(c, rays, w, h, 256, 0, seeds)
    c.close()
    hc.z_grid(a, b, h, w, f"{name}: NEE vs plain")


@pytest.mark.gpu
def test_lower_noise():
    """small light, 16 spp: the RMS error against a 4096-spp plain reference is at most half the plain estimator's"""
    t, m = small_light_room()
    w = h = 32
    rays = hc.rays(w, h)
    c = hc.ctx(t, m)
    ref = c.render(rays, w, h, 4096, seed=77, want_accum=True)[1].astype(np.float64)
    plain = c.render(rays, w, h, 16, seed=1, want_accum=True)[1]
    nee = c.render(rays, w, h, 16, seed=1, flags=capi.FLAG_NEE, want_accum=True)[1]
    c.close()
    rp = np.sqrt(np.mean((plain - ref) ** 2))
    rn = np.sqrt(np.mean((nee - ref) ** 2))
    print(f"small-light room 16 spp: RMS plain {rp:.4f}, NEE {rn:.4f}, ratio {rn / rp:.3f}")
    assert rn <= 0.5 * rp, (rn, rp)


@pytest.mark.gpu
def test_error_contract():
    t, m = scene.closed_room(200)
    rays = hc.rays()
    for bad in (-0.5, np.nan, np.inf):
        mb = m.copy()
        mb[40, 4] = bad
        c = hc.ctx(t, mb)
        with pytest.raises(RuntimeError, match=E_INVALID):
            c.render(rays, W, H, 2, seed=1, flags=capi.FLAG_NEE)
        c.render(rays, W, H, 2, seed=1)                   # the plain estimator does not look at it
        c.close()
    # no emitter: black, as without the flag
    m0 = m.copy()
    m0[:, 3:6] = 0
    c = hc.ctx(t, m0)
    img = c.render(rays, W, H, 2, seed=1, flags=capi.FLAG_NEE)
    assert not img.any()
    # a retired variant number
    with pytest.raises(RuntimeError, match=E_INVALID):
        c.render(rays, W, H, 2, seed=1, flags=capi.FLAG_NEE | 9)
    c.close()


@pytest.mark.gpu
def test_cli_and_adapter(tmp_path):
    """spath_cli --nee goes through hip_renderer::set_nee and gives the capi image, one-shot and progressive"""
    import subprocess
    cli = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "spath_amd", "host", "build", "spath_cli")
    t, m = scene.open_clutter(100)
    sp = str(tmp_path / "s.bin")
    scene.write_scene(sp, t, m)
    w, h = 40, 24
    rays = np.ascontiguousarray(view.Camera(w, h).get_viewport(), dtype=F)
    c = hc.ctx(t, m)
    want = c.render(rays, w, h, 8, seed=9, flags=capi.FLAG_NEE)
    c.close()
    for extra in ([], ["--progressive", "3"]):
        out = str(tmp_path / "o.rgba")
        subprocess.run([cli, "--scene", sp, "--w", str(w), "--h", str(h), "--spp", "8", "--seed", "9", "--nee", "--out", out] + extra,
                       check=True, capture_output=True, timeout=120)
        assert open(out, "rb").read() == want.tobytes(), extra
