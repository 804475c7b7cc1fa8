"""The device radix sort (spath_amd/csrc/sp_radix_sort.h: k_rs_hist / k_rs_scan / k_rs_scatter behind the context's radix_sort()) on its
own, through the test-only entry sphip_selftest_sort.  Both the default scan's prepass and the BVH build rest on it being a STABLE sort,
which closest hits cannot show.  Reference: numpy's stable argsort; keys and values must equal it element for element.

Sizes: one element, around one wave (64), one scatter round (256), one block (2048), two blocks, and around the point where the scan
kernel's 256 threads take more than one count each (16 counts per block of 2048: 32 768 elements is the last size with one count per
thread, 32 769 the first with two, 34 819 has 272 counts and leaves threads idle), and one size of many blocks."""
import numpy as np
import pytest

import bvh_model
from spath_amd import scene

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4096, 4097, 32768, 32769, 34819, 300001]
PATTERNS = ["uniform", "equal", "ones", "two", "top_digit", "bottom_digit", "ascending", "descending", "morton"]


def make_keys(pattern, n, rng):
    u = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    if pattern == "uniform":
        return u
    if pattern == "equal":                                    # pure stability
        return np.full(n, 0x12345678, np.uint32)
    if pattern == "ones":
        return np.full(n, 0xffffffff, np.uint32)
    if pattern == "two":
        return np.where(u & 1, np.uint32(0x80000001), np.uint32(7)).astype(np.uint32)
    if pattern == "top_digit":
        return ((u & np.uint32(0xf0000000)) | np.uint32(0x0abcdef1)).astype(np.uint32)
    if pattern == "bottom_digit":
        return ((u & np.uint32(0xf)) | np.uint32(0x5a5a5a50)).astype(np.uint32)
    if pattern == "ascending":
        return np.sort(u)
    if pattern == "descending":
        return np.sort(u)[::-1].copy()
    if pattern == "morton":                                   # 30 significant bits, 32 cells per axis: many ties
        c = (rng.integers(0, 32, (n, 3)) * 32).astype(np.float32) / np.float32(1024)
        return (bvh_model.morton10(c[:, 0]) | (bvh_model.morton10(c[:, 1]) << np.uint32(1)) | (bvh_model.morton10(c[:, 2]) << np.uint32(2))).astype(np.uint32)
    raise ValueError(pattern)


def check_sort(hip, keys, key_bits=32):
    n = keys.size
    vals = np.random.default_rng(n).permutation(n).astype(np.uint32)      # not arange: a sort that rebuilt values from positions fails
    ok, ov = hip.selftest_sort(keys, vals, key_bits)
    mask = np.uint32(0xffffffff >> (32 - key_bits))
    order = np.argsort(keys & mask, kind="stable")
    assert np.array_equal(ok, keys[order]), (n, key_bits)
    assert np.array_equal(ov, vals[order]), (n, key_bits)


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n", SIZES)
def test_sort_equals_stable_argsort(hip, n, pattern):
    check_sort(hip, make_keys(pattern, n, np.random.default_rng(1000 + n)))


@pytest.mark.parametrize("pattern", ["uniform", "morton", "bottom_digit"])
@pytest.mark.parametrize("n", SIZES)
def test_sort_odd_pass_count_ignores_high_bits(hip, n, pattern):
    """key_bits = 12: three passes, so the result is in the other half of the double buffer than after the production width's eight,
    and the bits above the twelfth (random here) take no part in the order but travel with the keys"""
    check_sort(hip, make_keys(pattern, n, np.random.default_rng(2000 + n)), key_bits=12)


def test_sort_reuses_its_buffers_and_leaves_built_streams_alone(hip):
    """a smaller sort after a larger one on the same context (grow-only buffers, a histogram sized for more blocks), and a sort
    between two walks of a built BVH: the structure keeps no pointer into the sort's buffers"""
    t, m = scene.closed_room(300)
    hip.set_scene(t, m)
    rays = np.random.default_rng(5).normal(size=(512, 6)).astype(np.float32)
    before = hip.selftest_bvh_walk(rays)
    dump = hip.selftest_bvh_dump()
    rng = np.random.default_rng(6)
    for n in (300001, 257, 34819, 1, 4097):
        check_sort(hip, make_keys("uniform", n, rng))
        check_sort(hip, make_keys("morton", n, rng), key_bits=12)
    after = hip.selftest_bvh_walk(rays)
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(before, after))
    again = hip.selftest_bvh_dump()
    assert all(np.array_equal(dump[k][1:] if k == "nodes" else dump[k], again[k][1:] if k == "nodes" else again[k]) for k in ("meta", "nodes", "rec", "idx"))
