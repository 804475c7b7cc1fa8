"""The host side of a render launch that needs no device (spath_amd/csrc/sp_host_plan.h): plan_launch on plans derived by hand from the
sample-chunk rules of DESIGN.md section 3, and the light tables against their numpy statements, bit for bit.  The header is compiled
into a stand-alone program (tests/host_plan_driver.cpp) with the host compiler under AddressSanitizer and UBSan; nothing is loaded into
Python, and no GPU is needed."""
import os
import struct
import subprocess

import numpy as np
import pytest

import env_model as em
import path_model as pm
from path_model import F
from spath_amd import scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AMPLE = 1 << 62
NEE, MIS, SPEC, GLASS, ENV, SMOOTH, CAM, ADAPT, PROG = (1 << k for k in range(9))
CYLM, CYLM512, CYLW4S = (1, 0, 3), (1, 0, 4), (4, 1, 2)       # TwoStage {R, split, scan} of the default scan's two shapes and of rpl_cylw4s


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("host_plan") / "host_plan_driver")
    # the sanitizer runtimes are linked into the program: it runs as it is, with nothing preloaded
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "spath_amd", "csrc"), os.path.join(ROOT, "tests", "host_plan_driver.cpp"), "-o", exe], check=True)
    return exe


def plan(driver, n_rays, spp, ts=CYLM, threads=256, forced=0, pt=1, feat=0, samp_cap=0, work_cap=0, free=AMPLE):
    out = subprocess.run([driver, "plan"] + [str(int(x)) for x in (n_rays, spp, forced, pt, *ts, threads, feat, samp_cap, work_cap, free)],
                         check=True, capture_output=True, text=True).stdout
    return {k: int(v) for k, v in (w.split("=") for w in out.split())}


def test_small_frame_is_split_along_the_samples(driver):
    """6144 rays = 24 workgroups of 256: the chunks double towards 262144 workgroups up to 128, then stop at the 8 samples.  Sample
    buffer: 8 spp x 12 B x 6144 (a multiple of 256 already); work: 6144 lanes (a multiple of 1024) x 8 chunks slots of 40 + 12 B"""
    p = plan(driver, 6144, 8)
    assert (p["chunks"], p["px_blocks"], p["grid_pt"], p["samp_stride"]) == (8, 24, 192, 6144)
    assert (p["samp_bytes"], p["n_work"], p["n_work"] * p["slot_work"], p["n_launches"]) == (589_824, 49_152, 2_555_904, 2)
    assert (p["grid"], p["grid_px"], p["too_large"], p["asked"]) == (192, 24, 0, 1)
    # one sample: nothing to split, no sample buffer, no resolve, nothing asked
    p = plan(driver, 6144, 1)
    assert (p["chunks"], p["samp_bytes"], p["samp_stride"], p["px_blocks"], p["n_launches"], p["asked"]) == (1, 0, 0, 0, 1, 0)
    assert (p["grid"], p["grid_pt"], p["n_work"]) == (24, 24, 6144)


def test_forced_chunks(driver):
    p = plan(driver, 6144, 8, forced=3)
    assert (p["chunks"], p["grid_pt"], p["n_work"], p["asked"]) == (3, 72, 3 * 6144, 0)
    assert plan(driver, 6144, 8, forced=16)["chunks"] == 8            # never more chunks than samples


def test_512_thread_shape(driver):
    """half the workgroups per frame, and half the target: the same number of resident-wave rounds.  2^20 rays are 2048 workgroups of
    512: 64 chunks reach 131072 (with the 256-thread target it would be 128)"""
    p = plan(driver, 6144, 8, ts=CYLM512, threads=512)
    assert (p["chunks"], p["px_blocks"], p["grid_pt"], p["grid_px"], p["grid"]) == (8, 12, 96, 12, 192)
    assert plan(driver, 1 << 20, 256, ts=CYLM512, threads=512)["chunks"] == 64
    assert plan(driver, 1 << 20, 256)["chunks"] == 64


def test_split_variant_counts_lane_iterations(driver):
    """R = 4 samples of one pixel per lane: 6 spp are 2 iterations, so 2 chunks; 4 slots per padded ray and chunk.  The one-scan
    kernels run the same variant with 4 pixels per lane: 6 workgroups"""
    p = plan(driver, 6144, 6, ts=CYLW4S)
    assert (p["chunks"], p["n_work"], p["px_blocks"], p["grid_pt"], p["grid_px"]) == (2, 49_152, 24, 48, 6)


def test_memory_back_off_and_slot_bytes(driver):
    """1920 x 1080 at 256 spp: 8100 workgroups, 64 chunks reach the target.  Sample buffer 256 x 12 x 2073600 = 6.37 GB; work
    2073600 x chunks x 52 B: 64, 32, 16, 8 chunks need 13.27, 9.82, 8.10, 7.23 GB, all above 90 % of 8 GB; 4 need 6.80 GB"""
    n = 1920 * 1080
    p = plan(driver, n, 256)
    assert (p["chunks"], p["asked"], p["samp_bytes"]) == (64, 1, 256 * 12 * n)
    p = plan(driver, n, 256, free=8_000_000_000)
    assert (p["chunks"], p["asked"], p["n_work"], p["n_launches"]) == (4, 1, 4 * n, 2)
    p = plan(driver, n, 256, free=-1)                                  # the device cannot tell: unsplit
    assert (p["chunks"], p["asked"], p["samp_bytes"]) == (1, 1, 0)
    p = plan(driver, n, 256, samp_cap=AMPLE, work_cap=AMPLE, free=0)   # nothing has to grow: nothing is asked
    assert (p["chunks"], p["asked"]) == (64, 0)
    p = plan(driver, n, 2048)                                          # 50.96 GB of samples, above the 16 GiB cap: unsplit, unasked
    assert (p["chunks"], p["asked"]) == (1, 0)
    for feat, want in ((0, (52, 0, 0)), (NEE, (100, 0, 0)), (NEE | MIS, (112, 0, 0)), (ADAPT | PROG, (52, 16, 0)), (ENV, (52, 0, 12)),
                       (NEE | MIS | ADAPT | PROG | ENV | SPEC | GLASS | SMOOTH | CAM, (112, 16, 12))):
        p = plan(driver, n, 256, feat=feat)
        assert (p["slot_work"], p["slot_adp_wst"], p["slot_env_M"]) == want
    # the estimate is the sum of the three: 8 chunks of 112 + 16 + 12 B need 6.37 + 2.32 = 8.69 GB, 4 chunks 7.53 GB, of 9.6 GB x 0.9 = 8.64
    assert plan(driver, n, 256, feat=NEE | MIS | ADAPT | PROG | ENV, free=9_600_000_000)["chunks"] == 4
    assert plan(driver, n, 256, feat=NEE | MIS, free=9_600_000_000)["chunks"] == 8     # 6.37 + 1.86 = 8.23 GB


def test_work_slots_beyond_32_bits_are_refused(driver):
    """2^31 rays on a split variant: 2^31 x 4 slots (one chunk: the frame has workgroups enough) do not fit n_work"""
    assert plan(driver, 1 << 31, 4, ts=CYLW4S)["too_large"] == 1
    assert plan(driver, 1 << 31, 4, ts=CYLW4S, pt=0)["too_large"] == 0     # the one-scan kernels have no work buffer
    assert plan(driver, (1 << 30) - 1024, 4, ts=CYLW4S)["too_large"] == 0


def run_lights(driver, tmp_path, tris, mats, W_env=0.0):
    """-> (bad_tri, bad_comp, tables), a table being (tri, cdf, ipdf, W, tipdf) decoded from the device layout"""
    t = np.ascontiguousarray(tris, F).reshape(-1, 12)
    m = np.ascontiguousarray(mats, F).reshape(-1, 6)
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<Qd", t.shape[0], W_env) + t.tobytes() + m.tobytes())
    subprocess.run([driver, "lights", src, dst], check=True)
    raw = open(dst, "rb").read()
    bad_tri, bad_comp = struct.unpack_from("<qq", raw, 0)
    pos, tables = 16, []
    while pos < len(raw):
        n, W = struct.unpack_from("<Qd", raw, pos)
        pos += 16
        parts = []
        for dtype, count in ((np.float64, n), (np.int32, n), (F, n), (F, t.shape[0])):
            parts.append(np.frombuffer(raw, dtype, count, pos))
            pos += count * np.dtype(dtype).itemsize
        tables.append((parts[1], parts[0], parts[2], W, parts[3]))
    return bad_tri, bad_comp, tables


def same_bits(got, want):
    for g, w in zip(got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape
        if w.dtype.kind == "f":
            assert g.dtype == w.dtype and g.tobytes() == w.tobytes()
        else:
            assert np.array_equal(g, w)


@pytest.mark.parametrize("name", ["closed_room_200", "open_clutter_100"])
def test_light_tables_equal_the_numpy_statements(driver, tmp_path, scenes, name):
    tris, mats = scenes[name]
    plain = scene.light_table(tris, mats)
    n_flagged = 0
    for env in em.replay_maps().values():
        part = em.scene_part(em.tables(env), tris, mats)
        entry = part["w_env"] > 0.0
        bad_tri, _, tables = run_lights(driver, tmp_path, tris, mats, part["W"] if entry else 0.0)
        assert bad_tri == -1 and len(tables) == (2 if entry else 1)
        tri, cdf, ipdf, W = pm.light_table(tris, mats)
        same_bits(tables[0][:4], (tri, cdf, ipdf, np.float64(W)))
        same_bits(tables[0], plain[:3] + (np.float64(plain[3]), plain[4]))
        if entry:
            want = em.flagged_light_table(tris, mats, part)
            assert want[0][-1] == -1 and want[0].size == tri.size + 1
            same_bits(tables[1], want[:3] + (np.float64(want[3]), want[4]))
            n_flagged += 1
    assert n_flagged == 2 and plain[0].size > 0                       # both maps have an entry, both scenes emitters


def test_scene_without_emitters_has_an_empty_table(driver, tmp_path, scenes):
    tris, mats = scenes["open_clutter_100"]
    m = mats.copy().reshape(-1, 6)
    m[:, 3:] = 0
    bad_tri, _, tables = run_lights(driver, tmp_path, tris, m)
    assert bad_tri == -1 and len(tables) == 1
    tri, cdf, ipdf, W, tipdf = tables[0]
    assert tri.size == cdf.size == ipdf.size == 0 and W == 0.0 and tipdf.size == m.shape[0] and not tipdf.any()


@pytest.mark.parametrize("value", [-1.0, float("nan"), float("inf")])
def test_first_invalid_emittance_is_reported(driver, tmp_path, scenes, value):
    tris, mats = scenes["closed_room_200"]
    m = mats.copy().reshape(-1, 6)
    m[7, 4] = value
    m[7, 5] = -2.0
    m[3 + 8, 3] = np.nan
    assert run_lights(driver, tmp_path, tris, m)[:2] == (7, 1)
    m[2, 5] = value
    assert run_lights(driver, tmp_path, tris, m) == (2, 2, [])
