"""The display transform (include/spath_hip.h "display transform") stated in numpy operation by operation: the
luminance bins by view(np.uint32) >> 20, the exposure of a histogram in float64 in the header's order, the curves in float32 with every
intermediate rounded on its own, the linear code as scene::vec3_RGBA forms it and the sRGB code by np.searchsorted on the table.

Not a test module: tests/test_display_model.py holds it to closed forms and the library's host functions to it, tests/test_hip_display.py
holds the kernels to it."""
import math

import numpy as np

F = np.float32
BINS = 2048
CLAMP, REINHARD, FILMIC = 0, 1, 2
LINEAR, SRGB = 0, 1
DEFAULT_DISPLAY = {"exposure": 1.0, "white": 4.0, "curve": FILMIC, "encode": SRGB}
DEFAULT_METERING = {"key": 0.18, "low": 0.5, "high": 0.95}


def srgb_closed_form():
    """the inverse sRGB transfer function at (k - 0.5) / 255, k = 1 .. 255, in float64"""
    c = (np.arange(1, 256, dtype=np.float64) - 0.5) / 255.0
    return np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4)


def lum(c):
    c = np.asarray(c, F).reshape(-1, 3)
    with np.errstate(all="ignore"):
        return F(F(F(0.2126) * c[:, 0]) + F(F(0.7152) * c[:, 1])) + F(F(0.0722) * c[:, 2])


def bins(c):
    """the histogram bin of every pixel of an (n, 3) f32 image"""
    l = lum(c)
    with np.errstate(invalid="ignore"):
        pos = l > 0
    return np.where(pos, l.view(np.uint32) >> 20, 0).astype(np.int64)


def histogram(c):
    return np.bincount(bins(c), minlength=BINS).astype(np.uint32)


def bin_level(b):
    """L[b]: Mitchell's log2 of the centre of a valid bin (exact in double)"""
    return float((b >> 3) - 127) + (float(b & 7) + 0.5) / 8.0


def check_metering(key, low, high, reserved=0):
    """-> the name of the first field that breaks its rule, or "ok" """
    key, low, high = float(F(key)), float(F(low)), float(F(high))
    if not (math.isfinite(key) and key > 0):
        return "key"
    if not 0.0 <= low <= 1.0:
        return "low"
    if not 0.0 <= high <= 1.0:
        return "high"
    if not low < high:
        return "window"
    return "ok" if int(reserved) == 0 else "reserved"


def check_display(exposure, white, curve, encode, reserved=(0, 0)):
    exposure, white = float(F(exposure)), float(F(white))
    if not (math.isfinite(exposure) and exposure > 0):
        return "exposure"
    if not (math.isfinite(white) and white > 0):
        return "white"
    if curve not in (CLAMP, REINHARD, FILMIC):
        return "curve"
    if encode not in (LINEAR, SRGB):
        return "encode"
    return "ok" if not any(reserved) else "reserved"


def exposure(hist, key=0.18, low=0.5, high=0.95):
    """the exposure a 2048-bin histogram meters: float64, bins in ascending order -> np.float32"""
    hist = np.asarray(hist, np.uint32)
    assert hist.shape == (BINS,)
    key, low, high = float(F(key)), float(F(low)), float(F(high))
    N = int(hist[8:2040].astype(np.uint64).sum())
    if N == 0:
        return F(1.0)
    lo = int(low * float(N))
    hi = N - int((1.0 - high) * float(N))
    if hi <= lo:
        lo, hi = 0, N
    M, S, cum = 0, 0.0, 0
    for b in range(8, 2040):
        first, cum = cum, cum + int(hist[b])
        a, z = max(first, lo), min(cum, hi)
        if z <= a:
            continue
        part = z - a
        M += part
        S += float(part) * bin_level(b)
    mean = S / float(M)
    x = min(max(-mean, -126.0), 126.0)
    f = math.floor(x)
    return F(key * math.ldexp(1.0 + (x - f), int(f)))


def filmic(x):
    x = np.asarray(x, F)
    with np.errstate(all="ignore"):
        num = F(x * F(F(F(2.51) * x) + F(0.03)))
        den = F(F(x * F(F(F(2.43) * x) + F(0.59))) + F(0.14))
        return F(num / den)


def clamp01(x):
    """vec3::clamp: x > 1 ? 1 : (x < 0 ? 0 : x) -- a NaN passes"""
    x = np.asarray(x, F)
    with np.errstate(invalid="ignore"):
        return np.where(x > 1, F(1), np.where(x < 0, F(0), x)).astype(F)


def display_linear(c, E=1.0, white=4.0, curve=FILMIC):
    """exposure, curve and clamp of an (n, 3) f32 image -> the display-linear float output"""
    c = np.asarray(c, F).reshape(-1, 3)
    E = F(E)
    with np.errstate(all="ignore"):
        v = F(c * E)
        if curve == REINHARD:
            l = lum(v)
            w2 = F(F(white) * F(white))
            s = F(F(F(1) + F(l / w2)) / F(F(1) + l))
            v = np.where((l > 0)[:, None], F(v * s[:, None]), v).astype(F)
        elif curve == FILMIC:
            v = filmic(v)
        else:
            assert curve == CLAMP
    return clamp01(v)


def quant8(x):
    """scene::vec3_RGBA of one channel as the device evaluates it: clamp, * 255 + 0.5, truncate; a NaN converts to 0"""
    x = np.asarray(x, F)
    with np.errstate(invalid="ignore"):
        c = F(F(clamp01(x) * F(255)) + F(0.5))
        t = np.where(np.isnan(c), F(0), c)
        return np.where(t < 0, 0, np.where(t > 255, 255, t.astype(np.int64) & 0xFF)).astype(np.uint8)


def srgb_code(x, T):
    """the number of k in 1 .. 255 with x >= T[k] (T: the 255 thresholds); a NaN is 0"""
    x = np.asarray(x, F)
    T = np.asarray(T, F)
    assert T.shape == (255,)
    code = np.searchsorted(T, np.where(np.isnan(x), F(-1), x), side="right")
    return code.astype(np.uint8)


def encode(v, enc, T=None):
    """(n, 3) display-linear floats -> (n, 4) u8, alpha 0"""
    v = np.asarray(v, F).reshape(-1, 3)
    out = np.zeros((v.shape[0], 4), np.uint8)
    out[:, :3] = srgb_code(v, T) if enc == SRGB else quant8(v)
    return out


def display(c, T, E=1.0, white=4.0, curve=FILMIC, enc=SRGB):
    """-> (rgba (n, 4) u8, rgb (n, 3) f32)"""
    v = display_linear(c, E, white, curve)
    return encode(v, enc, T), v
