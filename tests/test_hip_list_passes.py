"""The list passes and re-test rounds of stage 2 of the default scan ("Stage 2"), against the oracle, tolerance 0.

Per tile a wave turns its survivor bits into a list and re-tests the list 64 entries per round.  The loop has three ways through it,
and a render takes whichever its scene and rays ask for; each case here is built to force one of them, under both workgroup shapes
(SPATH_HIP_CYLM_SHAPE = 256: quads, 512: octets):

  1  closed_room(300), 64 x 48 x 4 spp        everything fits one list pass and the rounds are short: the loop is left after one pass
  2  closed_room(1200, clutter_scale=10)      long lists: several rounds per tile
  3  closed_room(300) from 1e5 units away     the primary rays are outside the range of stage 1's halves: filter off, every group of
                                              every tile is listed, the list exceeds its capacity and the multi-pass path with words
                                              carried over to the next pass runs (then closest hits of rays aimed at the clutter through
                                              the wall: there the entries of the later passes decide the answer).  The arithmetic: the
                                              286 clutter triangles fall into three classes of about 95, i.e. about 24 quads or 12
                                              octets in a class's tile; with the filter off each of a wave's 64 rays lists them all:
                                              about 1536 / 768 entries against the list's 384, so three or more passes per tile
  4  open_clutter(1500)                       misses, classes whose last tile holds a single fragment, tiles that list nothing
  5  closed_room(n), 32 x 32 x 2 spp          n from 14 to 600: last rounds of many sizes (the case a short form of the last round
                                              would have to pass; DESIGN.md section 8 records why none ships)

RGBA8, float accumulators and the scan count equal the oracle's.  The oracle's results are computed once and shared by the two shapes.
Nothing here needs a statistics build.
"""
import numpy as np
import pytest
import torch

from spath_amd import scene, view

import test_hip_parity as P
from test_hip_shapes import _tiles, shaped  # noqa: F401  (the fixture that forces each workgroup shape in turn)

pytestmark = pytest.mark.gpu
F = np.float32
_want = {}


def far_camera(w, h):
    """The room from 1e5 units in front of it, the focal length stretched so that it still fills the frame: |pos| is beyond 512 times
    any length scale the room can have (its radius is below 7: S < 28), so stage 1's filter is off for every primary ray."""
    cam = view.Camera(w, h, focal=2.0e4)
    cam.set_delta_mov((0.0, 0.0, -1.0e5))
    return cam.get_viewport()


def oracle_render(O, key, rays, t, m, spp, seed):
    if key not in _want:
        _want[key] = O.render_counter(rays, t, m, spp, seed)
    return _want[key]


def check_render(hip, shape, O, key, rays, w, h, t, m, spp, seed):
    hip.set_scene(t, m)
    img, acc = hip.render(rays, w, h, spp, seed=seed, want_accum=True)
    st = hip.stats()
    want_img, want_acc, want_scans = oracle_render(O, key, rays, t, m, spp, seed)
    if t.shape[0] >= 64:                                          # (below 64 triangles the library scans without a filter: nothing is listed)
        assert st["kernel_variant"] == 16 and _tiles(hip, rays)[1] == shape, (key, shape, st["kernel_variant"])
    assert np.array_equal(img, want_img), (key, shape, "image", int((img != want_img).any(axis=1).sum()))
    assert np.array_equal(acc.view(np.uint32), want_acc.view(np.uint32)), (key, shape, "accumulator")
    assert st["scans_executed"] == want_scans, (key, shape, st["scans_executed"], want_scans)
    return want_img


def test_everything_fits_short_rounds(shaped, O):
    hip, shape = shaped
    t, m = scene.closed_room(300)
    check_render(hip, shape, O, "room300", view.Camera(64, 48).get_viewport(), 64, 48, t, m, 4, 11)


def test_long_lists_several_rounds(shaped, O):
    hip, shape = shaped
    t, m = scene.closed_room(1200, clutter_scale=10.0)
    check_render(hip, shape, O, "bigtris1200", view.Camera(64, 48).get_viewport(), 64, 48, t, m, 4, 12)


def test_filter_off_list_overflows(shaped, O):
    hip, shape = shaped
    t, m = scene.closed_room(300)
    rays = far_camera(64, 48)
    assert (np.abs(rays[:, :3]).sum(axis=1) > 512.0 * 28.0).all()
    check_render(hip, shape, O, "room300far", rays, 64, 48, t, m, 4, 13)
    assert _want["room300far"][2] > 64 * 48 * 4                   # the far rays do meet the room: their paths go on to a second scan
    # The room is closed, so what those rays meet is the outside of a wall (one of the few triangles scanned outside the stream), and the
    # frame alone would not notice a list entry lost.  Hence through the wall: the same far origins aimed at points of the clutter
    # triangles, the wall each ray meets first named as its source, so that the closest hit is one the list's entries deliver -- most of
    # them from a pass after the first.
    if "aimed" not in _want:
        rng = np.random.default_rng(20261021)
        n = 3072
        v = t[14:, :9].reshape(-1, 3, 3).astype(np.float64)
        k = rng.integers(0, v.shape[0], n)
        p = (v[k] * rng.dirichlet([1.0, 1.0, 1.0], n)[:, :, None]).sum(1)
        o = rays[rng.integers(0, rays.shape[0], n), :3].astype(np.float64)
        d = p - o
        ar = np.concatenate([o, d / np.linalg.norm(d, axis=1, keepdims=True)], axis=1).astype(F)
        src = O.closest_hits(ar, t, None)[0].astype(np.int32)
        _want["aimed"] = (ar, src) + tuple(O.closest_hits(ar, t, src))
    ar, src, want_idx, want_d = _want["aimed"]
    assert (src >= 0).mean() > 0.9 and (want_idx >= 14).mean() > 0.25, ((src >= 0).mean(), (want_idx >= 14).mean())
    n = ar.shape[0]
    d_rays, d_src = P.dev(ar), P.dev(src)
    d_idx = torch.zeros(n, dtype=torch.int32, device="cuda"); d_d = torch.zeros(n, dtype=torch.float32, device="cuda")
    hip.closest_hit_device(d_rays.data_ptr(), n, d_idx.data_ptr(), d_d.data_ptr(), d_src_idx=d_src.data_ptr(), flags=0)
    torch.cuda.synchronize()
    assert hip.stats()["kernel_variant"] == 16
    assert np.array_equal(d_idx.cpu().numpy(), want_idx), (shape, int((d_idx.cpu().numpy() != want_idx).sum()))
    assert np.array_equal(d_d.cpu().numpy().view(np.uint32), want_d.view(np.uint32)), shape


def test_misses_ragged_classes_and_empty_lists(shaped, O):
    hip, shape = shaped
    t, m = scene.open_clutter(1500)
    check_render(hip, shape, O, "open1500", view.Camera(64, 48).get_viewport(), 64, 48, t, m, 4, 14)


@pytest.mark.parametrize("n", [14, 64, 77, 110, 150, 230, 333, 450, 600])
def test_last_rounds_of_many_sizes(shaped, O, n):
    hip, shape = shaped
    t, m = scene.closed_room(n)
    check_render(hip, shape, O, ("sweep", n), view.Camera(32, 32).get_viewport(), 32, 32, t, m, 2, 15 + n)
