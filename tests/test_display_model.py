"""The display transform on the CPU (include/spath_hip.h "display transform"): the sRGB table against its closed form, the library's
host-only functions (sphip_srgb_thresholds, sphip_exposure_from_histogram, the defaults: none needs a GPU) against tests/display_model.py
bit for bit, and the properties of the curves that the model states."""
import ctypes as C

import numpy as np
import pytest

import display_model as D
from spath_amd import capi

F = np.float32


@pytest.fixture(scope="module")
def T():
    return capi.srgb_thresholds()


def _hist(**bins):
    h = np.zeros(D.BINS, np.uint32)
    for b, n in bins.items():
        h[int(b[1:])] = n
    return h


def _bits(x):
    return np.asarray(x, F).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------- the table
def test_every_threshold_is_within_one_ulp_of_the_closed_form(T):
    want = D.srgb_closed_form()
    assert T.dtype == F and T.shape == (255,)
    ulp = np.spacing(np.abs(T)).astype(np.float64)
    err = np.abs(T.astype(np.float64) - want)
    print("largest error in ulp:", float((err / ulp).max()))
    assert np.all(err <= ulp)
    # the literals were rounded to nearest: half an ulp, but for the error of the double pow itself
    assert np.all(err <= 0.5 * ulp * (1 + 1e-6))


def test_the_table_is_strictly_increasing_inside_the_unit_interval(T):
    assert np.all(np.diff(T) > 0)
    assert 0 < T[0] and T[-1] < 1


def test_srgb_codes_at_the_thresholds(T):
    below = np.nextafter(T, F(-np.inf))
    k = np.arange(1, 256)
    assert np.array_equal(D.srgb_code(T, T), k)
    assert np.array_equal(D.srgb_code(below, T), k - 1)
    assert np.array_equal(D.srgb_code(F([0, -1, 1, 2, np.inf, -np.inf, np.nan]), T), [0, 0, 255, 255, 255, 0, 0])
    # the code is the rounded sRGB encoding: spot values of the standard
    assert D.srgb_code(F([0.5]), T)[0] == 188 and D.srgb_code(F([0.18]), T)[0] == 118 and D.srgb_code(F([0.0031308]), T)[0] == 10


# ---------------------------------------------------------------------------------------------------------------- metering
# the last three collapse (hi <= lo) on every histogram: a high below 2^-53 makes 1.0 - (double)high round to 1.0, and hi = N - N = 0
WINDOWS = ((0.18, 0.5, 0.95), (0.18, 0.0, 1.0), (1.0, 0.25, 0.75), (0.5, 0.5, 0.5000001), (0.18, 0.999, 1.0),
           (1.0, 0.0, 1e-30), (0.18, 0.0, 1e-40), (0.5, 1e-20, 1e-17))
HISTS = {
    "empty": _hist(),
    "only invalid bins": _hist(b0=100, b3=7, b7=1, b2040=9, b2047=2),
    "a single bin": _hist(b1016=64),
    "two bins, the window cuts one": _hist(b1000=100, b1040=100),
    "two bins, uneven": _hist(b8=3, b2039=5),
    "one pixel": _hist(b1016=1),
    "a ramp": np.where((np.arange(D.BINS) >= 900) & (np.arange(D.BINS) < 1100), np.arange(D.BINS) % 13 + 1, 0).astype(np.uint32),
    "large counts": _hist(b0=5, b990=0xFFFFFFFF, b1016=0xFFFFFFFF, b1033=12345),
}


@pytest.mark.parametrize("name", list(HISTS))
def test_exposure_equals_the_model_bit_for_bit(name):
    for key, low, high in WINDOWS:
        got = capi.exposure_from_histogram(HISTS[name], (key, low, high))
        want = D.exposure(HISTS[name], key, low, high)
        assert _bits(got) == _bits(want), (name, key, low, high, got, want)


def test_exposure_closed_forms():
    # nothing valid: exposure 1, whatever the key
    assert capi.exposure_from_histogram(HISTS["empty"], (0.5, 0.0, 1.0)) == 1.0
    assert capi.exposure_from_histogram(HISTS["only invalid bins"], (0.5, 0.0, 1.0)) == 1.0
    # bin 1016 = 8 * 127: [1, 1.125), centre 1.0625, L = 0.5 / 8; E = key * 2^-L by Mitchell = key * (1 + (1 - 1/16)) / 2
    assert capi.exposure_from_histogram(HISTS["a single bin"], (1.0, 0.0, 1.0)) == F(0.96875)
    # 100 pixels at L = -2 + 1/16 and 100 at L = 3 + 1/16; the window [100, 190) lies in the upper bin, [0, 100) in the lower one
    assert capi.exposure_from_histogram(HISTS["two bins, the window cuts one"], (1.0, 0.5, 0.95)) == F(0.96875 / 8)
    assert capi.exposure_from_histogram(HISTS["two bins, the window cuts one"], (1.0, 0.0, 0.5)) == F(0.96875 * 4)
    # [50, 150): half of either, mean L = 1/2 + 1/16, x = -9/16 = -1 + 7/16: E = (1 + 7/16) / 2
    assert capi.exposure_from_histogram(HISTS["two bins, the window cuts one"], (1.0, 0.25, 0.75)) == F(1.4375 / 2)
    # one pixel, low = 0.5: lo = (u64)0.5 = 0, hi = 1 - (u64)0.05 = 1
    assert capi.exposure_from_histogram(HISTS["one pixel"], (1.0, 0.5, 0.95)) == F(0.96875)


def test_a_window_that_collapses_is_the_whole_range():
    """hi <= lo gives 0, N.  Accepted parameters reach it: low < high is tested in f32, but the window is formed in double, where
    1.0 - (double)high is exactly 1.0 for any high below 2^-53 (1e-30, or a denormal); then hi = N - (u64)N = 0 <= lo.  The library is
    held to literals and to the model, bit for bit, on the two-bin histograms."""
    cases = ((1.0, 0.0, 1e-30), (1.0, 0.0, 1e-40), (1.0, 1e-20, 1e-17), (1.0, 0.0, float(np.nextafter(F(0), F(1)))))
    for h in (_hist(b1016=10, b1024=10), HISTS["two bins, the window cuts one"]):
        whole = capi.exposure_from_histogram(h, (1.0, 0.0, 1.0))
        for key, low, high in cases:
            assert D.check_metering(key, low, high) == "ok"
            N = int(h.sum())
            assert N - int((1.0 - float(F(high))) * N) <= int(float(F(low)) * N), "the case is to collapse"
            got = capi.exposure_from_histogram(h, (key, low, high))
            assert _bits(got) == _bits(D.exposure(h, key, low, high)) == _bits(whole), (key, low, high, got)
    # (1/16 + 17/16) / 2 = (-31/16 + 49/16) / 2 = 9/16: x = -1 + 7/16, E = key * (1 + 7/16) / 2
    assert capi.exposure_from_histogram(_hist(b1016=10, b1024=10), (1.0, 0.0, 1e-30)) == F(0.71875)
    assert capi.exposure_from_histogram(HISTS["two bins, the window cuts one"], (1.0, 0.0, 1e-30)) == F(0.71875)
    assert capi.exposure_from_histogram(HISTS["two bins, the window cuts one"], (0.18, 0.0, 1e-40)) == F(float(F(0.18)) * 0.71875)
    # a single-pixel image, where the whole range and any window agree, and an uneven one, where they do not
    u = HISTS["two bins, uneven"]
    assert capi.exposure_from_histogram(u, (1.0, 0.0, 1e-30)) == capi.exposure_from_histogram(u, (1.0, 0.0, 1.0)) != \
        capi.exposure_from_histogram(u, (1.0, 0.0, 0.25))


def test_the_narrowest_ordinary_window():
    """adjacent floats around one half: the window holds one pixel"""
    h = _hist(b1016=10, b1024=10)
    nxt = float(np.nextafter(F(0.5), F(1)))
    # lo = 10, hi = 20 - (u64)9.9999988 = 11: the pixel of rank 10, in bin 1024: L = 1 + 1/16, x = -2 + 15/16
    assert capi.exposure_from_histogram(h, (1.0, 0.5, nxt)) == D.exposure(h, 1.0, 0.5, nxt) == F(1.9375 / 4)


@pytest.mark.parametrize("k", [1, 3, -2, 40])
def test_a_histogram_shifted_by_8k_bins_scales_the_exposure_by_2_to_the_minus_k(k):
    # 64 pixels in the window [32, 64 + 32): M = 64, every part * L a multiple of 1/16: the mean is exact, and so is the shift
    h = _hist(b1000=32, b1003=16, b1011=48, b1030=32)
    m = (0.18, 0.25, 0.75)
    base = capi.exposure_from_histogram(h, m)
    got = capi.exposure_from_histogram(np.roll(h, 8 * k), m)
    assert _bits(got) == _bits(F(np.ldexp(np.float64(base), -k))), (k, base, got)
    assert _bits(got) == _bits(D.exposure(np.roll(h, 8 * k), *m))


def test_exposure_clamps_at_the_ends_of_the_range():
    assert capi.exposure_from_histogram(_hist(b8=1), (1.0, 0.0, 1.0)) == D.exposure(_hist(b8=1), 1.0, 0.0, 1.0) > 1e37
    assert capi.exposure_from_histogram(_hist(b2039=1), (1.0, 0.0, 1.0)) == D.exposure(_hist(b2039=1), 1.0, 0.0, 1.0) < 1e-37


def test_mitchell_level_is_within_0_086_of_log2():
    b = np.arange(8, 2040)
    centre = ((b.astype(np.uint32) << 20) | (1 << 19)).view(F).astype(np.float64)
    L = np.array([D.bin_level(int(x)) for x in b])
    err = np.log2(centre) - L
    print("Mitchell error:", err.min(), err.max())
    assert err.min() >= 0 and err.max() < 0.0861


# ---------------------------------------------------------------------------------------------------------------- refusals
def _exposure_rc(hist, m, out):
    L = capi.load()
    return L.sphip_exposure_from_histogram(hist.ctypes.data if hist is not None else None, C.byref(m) if m is not None else None,
                                           C.byref(out) if out is not None else None)


BAD_METERING = {
    "key zero": (0.0, 0.5, 0.95, 0), "key negative": (-1.0, 0.5, 0.95, 0), "key inf": (np.inf, 0.5, 0.95, 0), "key nan": (np.nan, 0.5, 0.95, 0),
    "low below 0": (0.18, -0.1, 0.95, 0), "high above 1": (0.18, 0.5, 1.5, 0), "low above 1": (0.18, 1.5, 2.0, 0), "low nan": (0.18, np.nan, 0.95, 0),
    "high nan": (0.18, 0.5, np.nan, 0), "low == high": (0.18, 0.5, 0.5, 0), "low > high": (0.18, 0.9, 0.2, 0), "reserved": (0.18, 0.5, 0.95, 1),
}


@pytest.mark.parametrize("name", list(BAD_METERING))
def test_bad_metering_is_refused_and_writes_nothing(name):
    key, low, high, res = BAD_METERING[name]
    assert D.check_metering(key, low, high, res) != "ok"
    out = C.c_float(-7.0)
    assert _exposure_rc(HISTS["a single bin"], capi.Metering(key, low, high, res), out) == -1
    assert out.value == -7.0


def test_null_pointers_are_refused():
    out = C.c_float(-7.0)
    m = capi.Metering.defaults()
    assert _exposure_rc(None, m, out) == -1 and _exposure_rc(HISTS["empty"], None, out) == -1 and _exposure_rc(HISTS["empty"], m, None) == -1
    assert out.value == -7.0
    assert _exposure_rc(HISTS["empty"], m, out) == 0 and out.value == 1.0
    capi.load().sphip_srgb_thresholds(None)          # no output, no crash
    capi.load().sphip_display_defaults(None)
    capi.load().sphip_metering_defaults(None)


def test_defaults_are_the_stated_conventions():
    d, m = capi.Display.defaults(), capi.Metering.defaults()
    assert (d.exposure, d.white, d.curve, d.encode, tuple(d.reserved)) == (1.0, 4.0, capi.CURVE_FILMIC, capi.ENCODE_SRGB, (0, 0))
    assert (_bits(m.key), _bits(m.low), _bits(m.high), m.reserved) == (_bits(0.18), _bits(0.5), _bits(0.95), 0)
    assert D.check_display(d.exposure, d.white, d.curve, d.encode) == "ok" and D.check_metering(m.key, m.low, m.high) == "ok"
    assert (D.CLAMP, D.REINHARD, D.FILMIC, D.LINEAR, D.SRGB) == (capi.CURVE_CLAMP, capi.CURVE_REINHARD, capi.CURVE_FILMIC, capi.ENCODE_LINEAR,
                                                                   capi.ENCODE_SRGB)


# ---------------------------------------------------------------------------------------------------------------- the bins
def test_bins_of_special_values():
    big = np.finfo(F).max
    den = F(5e-39)
    px = F([[0, 0, 0], [-1, -1, -1], [np.nan, 1, 1], [np.inf, 0, 0], [den, den, den], [big, big, big], [1, 1, 1], [-0.0, -0.0, -0.0],
            [0, 1.4e-45, 0]])
    b = D.bins(px)
    # denormals fill the bins 0 .. 7 (the smallest share bin 0 with the pixels that have no luminance: neither is metered)
    assert list(b[:4]) == [0, 0, 0, 2040] and 1 <= b[4] <= 7 and b[7] == 0 and b[8] == 0
    # lum(big) = ((0.2126 + 0.7152) + 0.0722) * big rounds to at most big: the largest finite bin or infinity's, as f32 gives it
    assert b[5] in (2039, 2040)
    assert b[6] == (D.lum(F([[1, 1, 1]])).view(np.uint32)[0] >> 20) and b[6] in (1015, 1016)
    assert D.histogram(px).sum() == len(px)


# ---------------------------------------------------------------------------------------------------------------- the curves
def test_reinhard_maps_the_white_point_to_luminance_one():
    """l = w exactly (a grey pixel g with lum((g, g, g)) = w is searched per w): s = (1 + w / w^2) / (1 + w), l * s = 1 in exact arithmetic.
    In f32, for channels >= 0 (no cancellation anywhere): the input luminance l carries 3 roundings along its longest chain (product,
    sum, sum); s carries 5 (w * w, l / w2, 1 + ., 1 + l, the quotient); the output luminance 4 more (v * s, the product with the
    coefficient, two sums).  l_out = (1 + e_s)(1 + e_out) / (1 + e_in): 12 roundings, |l_out - 1| < 13 u, u = 2^-24."""
    bound = 13 * 2.0 ** -24
    for w in (0.25, 1.0, 4.0, 7.3, 100.0):
        for rgb in ((1, 1, 1), (1, 0.5, 0.25), (0, 1, 0), (0.1, 0.0, 3.0)):
            c = np.asarray(rgb, np.float64)
            c = F(c * (w / float((c * (0.2126, 0.7152, 0.0722)).sum())))[None, :]
            l_in = float(D.lum(c)[0])
            out = D.display_linear(c, 1.0, F(l_in), D.REINHARD)          # the white point: the pixel's own luminance
            # before the clamp: redo without it
            v = F(c * F(1))
            s = F(F(F(1) + F(F(l_in) / F(F(l_in) * F(l_in)))) / F(F(1) + F(l_in)))
            l_out = float(D.lum(F(v * s))[0])
            assert abs(l_out - 1.0) <= bound, (w, rgb, l_out)
            assert np.all(out <= 1) and np.all(out >= 0)


def _sweep():
    """non-negative finite floats, every 2^12-th bit pattern from 2^-40 to 2^40"""
    lo, hi = F(2.0 ** -40).view(np.uint32), F(2.0 ** 40).view(np.uint32)
    return np.concatenate([F([0]), np.arange(lo, hi, 1 << 12, dtype=np.uint32).view(F)])


@pytest.mark.parametrize("curve", [D.CLAMP, D.REINHARD, D.FILMIC])
def test_each_curve_is_monotonic_over_a_sweep_of_bit_patterns(curve, T):
    x = _sweep()
    grey = np.repeat(x[:, None], 3, axis=1)
    for E, white in ((1.0, 4.0), (0.37, 1.5), (8.0, 16.0)):
        v = D.display_linear(grey, E, white, curve)
        assert not np.isnan(v).any()
        assert np.all(np.diff(v, axis=0) >= 0), (curve, E, white)
        assert v[0].tolist() == [0, 0, 0] and np.all(v[-1] == 1)
        for enc in (D.LINEAR, D.SRGB):
            codes = D.encode(v, enc, T)[:, :3].astype(int)
            assert np.all(np.diff(codes, axis=0) >= 0)
            assert codes[0].tolist() == [0, 0, 0] and codes[-1].tolist() == [255, 255, 255]
            assert len(np.unique(codes[:, 0])) == 256          # every code is reached


def test_identity_settings_are_the_renders_resolve():
    """E = 1, CURVE_CLAMP, ENCODE_LINEAR: vec3::clamp and scene::vec3_RGBA (* 255 + 0.5, truncated) of the same floats"""
    rng = np.random.default_rng(5)
    c = np.concatenate([rng.uniform(-0.2, 1.3, (4000, 3)).astype(F), F([[0, 1, 0.5], [1e-9, 0.99999994, 1.0000001], [2, -3, 0.0019607844]])])
    got, v = D.display(c, None, 1.0, 4.0, D.CLAMP, D.LINEAR)
    ref = np.floor(np.clip(c.astype(np.float64), 0, 1).astype(F) * F(255) + F(0.5)).astype(np.uint8)
    assert np.array_equal(got[:, :3], ref) and not got[:, 3].any()
    assert np.array_equal(v, np.clip(c, 0, 1))


def test_filmic_closed_values():
    # f(0) = 0; the fit crosses 1 near x = 7.24 and tends to 2.51 / 2.43
    f = D.filmic(F([0, 0.18, 1.0, 7.0, 7.5, 1e6]))
    assert f[0] == 0 and abs(float(f[1]) - 0.267) < 2e-3 and abs(float(f[2]) - 0.8038) < 1e-3 and f[3] < 1 < f[4] and abs(float(f[5]) - 2.51 / 2.43) < 1e-5
