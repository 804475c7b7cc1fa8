"""What a host-pointer setter of the C ABI checks before it touches a device (spath_amd/csrc/sp_host_tables.h): the row rule of each
per-triangle table and the texel rule of the two images, the index of the first offender, and every message, compared with literals of
the texts that sphip_last_error has always given.  The header runs in the stand-alone program of tests/test_host_plan.py (host compiler,
AddressSanitizer and UBSan linked in, nothing loaded into Python); no GPU is needed."""
import subprocess

import pytest

from test_host_plan import driver  # noqa: F401  (the fixture that builds tests/host_plan_driver.cpp)

N_TRIS, FIRST, SECOND = 64, 40, 60                                   # two bad rows, as the GPU tests' error contracts use: the first is reported
NAN, INF = float("nan"), float("inf")
# a row that every rule accepts, and the message of a refused row with the row's values in %g form
GOOD = {
    "specular": (0.5, 0.25, 0.0, 1.0),
    "vertex_normals": (0.0, 0.0, 1.0, 0.0, -1.0, 0.0, 0.5, 0.5, -0.5),
    "dielectric": (1.0, 0.5, 0.25, 1.5),
    "roughness": (0.25,),
    "uv": (0.0, 0.0, 1.0, 0.0, -0.5, 2.0),
}
MESSAGE = {
    "specular": "specular table: triangle %d has {ks %s %s %s, p %s} (every value finite, ks >= 0, 0 <= p <= 1)",
    "vertex_normals": "vertex normals: triangle %d has {%s %s %s, %s %s %s, %s %s %s} (every value finite)",
    "dielectric": "dielectric table: triangle %d has {kt %s %s %s, ior %s} (every value finite, kt >= 0, ior 0 or >= 1)",
    "roughness": "roughness table: triangle %d has alpha %s (finite, 0 <= alpha <= 1)",
    "uv": "UV table: triangle %d has {%s %s, %s %s, %s %s} (every value finite)",
}
# (table, column, value): every way in which one value breaks its table's rule
REFUSED = (
    [("specular", c, v) for c, v in ((0, -1.0), (1, NAN), (2, INF), (3, -INF), (3, -0.5), (3, NAN), (3, 1.5))] +
    [("dielectric", c, v) for c, v in ((0, -1.0), (1, NAN), (2, INF), (3, -INF), (3, -1.5), (3, NAN), (3, 0.5), (3, 0.999))] +
    [("roughness", 0, v) for v in (-0.5, 1.5, NAN, INF, -INF)] +
    [("uv", c, v) for c, v in ((5, NAN), (0, INF), (3, -INF))] +
    [("vertex_normals", c, v) for c, v in ((8, NAN), (0, INF), (4, -INF))]
)


def g(x):
    """printf's %g of the float32 values used here (all of them exact in binary, so Python's %g of the double agrees)"""
    return "%g" % x


def run(driver, *words):
    out = subprocess.run([driver] + [str(w) for w in words], check=True, capture_output=True, text=True).stdout.split("\n")
    assert out[-1] == "" and len(out) in (2, 3)
    return int(out[0]), (out[1] if len(out) == 3 else None)


def run_table(driver, name, rows):
    return run(driver, "table", name, len(rows), *[g(x) for row in rows for x in row])


@pytest.mark.parametrize("name,col,value", REFUSED, ids=lambda x: x if isinstance(x, str) else g(x))
def test_first_refused_row_and_its_message(driver, name, col, value):
    rows = [list(GOOD[name]) for _ in range(N_TRIS)]
    rows[FIRST][col] = value
    rows[SECOND][col] = value
    rows[SECOND][0] = NAN
    assert run_table(driver, name, rows) == (FIRST, MESSAGE[name] % ((FIRST,) + tuple(g(x) for x in rows[FIRST])))
    rows[FIRST] = list(GOOD[name])                                    # the other one alone is found too
    assert run_table(driver, name, rows) == (SECOND, MESSAGE[name] % ((SECOND,) + tuple(g(x) for x in rows[SECOND])))


@pytest.mark.parametrize("name", sorted(GOOD))
def test_accepted_tables_return_n_tris(driver, name):
    """the edges of every rule: p and alpha 0 and 1, ior 0 (not glass) and exactly 1, ks and kt 0, negative and large UVs and normals"""
    edges = {
        "specular": [(0.0, 0.0, 0.0, 0.0), (1.0, 2.0, 3.0e30, 1.0), (0.5, 0.5, 0.5, 0.5)],
        "vertex_normals": [(0.0,) * 9, (-1.0e30, 1.0e30, 0.0) * 3],
        "dielectric": [(0.0, 0.0, 0.0, 0.0), (1.0, 1.0, 1.0, 1.0), (0.5, 0.5, 0.5, 0.0), (2.0, 0.0, 0.0, 1.0e30)],
        "roughness": [(0.0,), (1.0,), (0.5,)],
        "uv": [(0.0,) * 6, (-3.5, 1.0e30, 2.0, -1.0e30, 0.5, 0.25)],
    }[name]
    rows = [list(GOOD[name]) for _ in range(N_TRIS - len(edges))] + [list(e) for e in edges]
    assert run_table(driver, name, rows) == (N_TRIS, None)
    assert run_table(driver, name, []) == (0, None)


@pytest.mark.parametrize("noun", ["atlas", "environment map"])
@pytest.mark.parametrize("value", [-1.0, -0.5, NAN, INF, -INF], ids=g)
def test_first_refused_texel_and_its_coordinates(driver, noun, value):
    """a 5 x 3 image, texel (i, j) at [(j * 5 + i) * 3]: component 1 of texel (3, 2) is float 40, and a later one is bad as well"""
    w, h = 5, 3
    texels = [0.25 * (k % 7) for k in range(w * h * 3)]
    assert run(driver, "texels", noun, w, h, *[g(x) for x in texels]) == (w * h * 3, None)
    texels[(2 * w + 3) * 3 + 1] = value
    texels[(2 * w + 4) * 3 + 2] = NAN
    assert run(driver, "texels", noun, w, h, *[g(x) for x in texels]) == (
        40, "%s: texel (3, 2) has component 1 = %s (every value finite and >= 0)" % (noun, g(value)))
    texels[(2 * w + 3) * 3 + 1] = 0.0
    assert run(driver, "texels", noun, w, h, *[g(x) for x in texels]) == (
        44, "%s: texel (4, 2) has component 2 = nan (every value finite and >= 0)" % noun)
