"""numpy model of the records and the re-test of stage 2 of the default scan (spath_amd/csrc/sp_cyl_scan.h: CylEdges, cyl_slab_record,
cyl_record, cyl_retest_record, cyl_setup, cyl_x; sp_cylm_scan.h: cylm_retest), with the kernel's roundings: the records in double,
each coefficient rounded once to float32; the ray state and the five-term chain in float32 (FMA emulated through double).

Used by tests/test_retest_margin_model.py and tools/retest_edge_model.py.  No GPU, numpy only.
"""
import numpy as np

F = np.float32
U = 2.0 ** -24
WA_MIN = 0.28867513459481287          # kCylRetestWa: 1 / (2 sqrt(3)), rounded down


def fma(a, b, c):
    """float32 fused multiply-add through float64 (the product of two floats is exact in double)"""
    with np.errstate(all="ignore"):
        return (np.asarray(a, F).astype(np.float64) * np.asarray(b, F).astype(np.float64) + np.asarray(c, F).astype(np.float64)).astype(F)


class Edges:
    """CylEdges: vertices, the three edges (0 = e1, 1 = e2 as the reference rounds them, 2 = c = e2 - e1 in double), squared lengths."""

    def __init__(self, t):
        t = np.asarray(t, F)
        self.n = t.shape[0]
        self.v = t[:, :9].reshape(-1, 3, 3).astype(np.float64)                          # A, B, C
        with np.errstate(all="ignore"):
            e1 = (t[:, 3:6] - t[:, 0:3]).astype(np.float64)
            e2 = (t[:, 6:9] - t[:, 0:3]).astype(np.float64)
            self.e = np.stack([e1, e2, e2 - e1], axis=1)
            self.l = (self.e[:, :, 0] * self.e[:, :, 0] + self.e[:, :, 1] * self.e[:, :, 1]) + self.e[:, :, 2] * self.e[:, :, 2]

    def longest(self):
        l = self.l
        return np.where((l[:, 1] >= l[:, 0]) & (l[:, 1] >= l[:, 2]), 1, np.where(l[:, 0] >= l[:, 2], 0, 2))

    def p0(self, j):            # e1: A, e2: A, c: B
        return self.v[np.arange(self.n), np.where(j == 2, 1, 0)]

    def p1(self, j):            # e1: C, e2: B, c: A
        return self.v[np.arange(self.n), np.where(j == 0, 2, np.where(j == 1, 1, 0))]


def slab_record(E, j, a=None):
    """cyl_slab_record for edge j[n] of every triangle, scaled by 1 / w_a (a = None: the direction's own dominant axis).
    Returns dict(a, beta, gamma, mc [n, 3], H, wa, ok); a record that is not ok is the always-surviving one (zeros, H = +inf)."""
    idx = np.arange(E.n)
    with np.errstate(all="ignore"):
        w3 = E.e[idx, j]
        ln = np.sqrt(E.l[idx, j])
        w = w3 / ln[:, None]
        aw = np.abs(w)
        if a is None:
            a = np.where((aw[:, 0] >= aw[:, 1]) & (aw[:, 0] >= aw[:, 2]), 0, np.where(aw[:, 1] >= aw[:, 2], 1, 2))
        b, c = (a + 1) % 3, (a + 2) % 3
        s = 1.0 / w[idx, a]
        p0, p1 = E.p0(j), E.p1(j)
        pc, ph = 0.5 * (p0 + p1), 0.5 * (p1 - p0)
        cr = lambda x, y: np.stack([x[:, 1] * y[:, 2] - x[:, 2] * y[:, 1], x[:, 2] * y[:, 0] - x[:, 0] * y[:, 2], x[:, 0] * y[:, 1] - x[:, 1] * y[:, 0]], axis=1)
        mcd, hv = cr(w, pc) * s[:, None], cr(w, ph) * s[:, None]
        beta, gamma = (w[idx, b] * s).astype(F), (w[idx, c] * s).astype(F)
        mc = mcd.astype(F)
        H = (np.sqrt((hv[:, 0] * hv[:, 0] + hv[:, 1] * hv[:, 1]) + hv[:, 2] * hv[:, 2]) * (1.0 + 2.0 ** -20)).astype(F)
        chk = ((((beta + gamma) + mc[:, 0]) + mc[:, 1]) + mc[:, 2]) + H
        ok = (chk - chk) == 0
    z = F(0)
    return dict(a=np.where(ok, a, 0), beta=np.where(ok, beta, z), gamma=np.where(ok, gamma, z), mc=np.where(ok[:, None], mc, z),
                H=np.where(ok, H, F(np.inf)), wa=w[idx, a], ok=ok)


def records(t, rule="kernel"):
    """(A, R): cyl_record (the longest edge's cylinder: stage 1's, and the class) and the re-test's record of every triangle.
    rule: "kernel" = cyl_retest_record; "second" / "third" = that edge's cylinder in the edge's own frame (tools/retest_edge_model.py);
    "A" = the longest edge's own record again (the re-test before this change)."""
    E = Edges(t)
    jl = E.longest()
    A = slab_record(E, jl)
    if rule == "A":
        return A, A
    idx = np.arange(E.n)
    j1, j2 = np.where(jl == 0, 1, 0), np.where(jl == 2, 1, 2)
    jb = np.where(E.l[idx, j2] > E.l[idx, j1], j2, j1)
    jc = np.where(jb == j1, j2, j1)
    a = A["a"]
    with np.errstate(all="ignore"):
        second = np.abs(E.e[idx, jb, a]) / np.sqrt(E.l[idx, jb]) >= WA_MIN
    j = {"kernel": np.where(second, jb, jc), "second": jb, "third": jc}[rule]
    if rule != "kernel":                     # that edge's cylinder in its own frame (its direction's dominant axis): the geometry alone
        R = slab_record(E, j)
        a = R["a"]
    else:
        R = slab_record(E, j, a)
    with np.errstate(all="ignore"):
        good = A["ok"] & R["ok"] & (np.abs(R["wa"]) >= 0.28)
    z = F(0)
    R = dict(a=a, beta=np.where(good, R["beta"], z), gamma=np.where(good, R["gamma"], z), mc=np.where(good[:, None], R["mc"], z),
             H=np.where(good, R["H"], F(np.inf)), wa=R["wa"], ok=good, edge=j)
    return A, R


def scene_bound(t):
    """bounds[0] of k_repack: the largest 1-norm of a vertex, in float32"""
    t = np.asarray(t, F)
    with np.errstate(all="ignore"):
        s = [(np.abs(t[:, 3 * k]) + np.abs(t[:, 3 * k + 1])) + np.abs(t[:, 3 * k + 2]) for k in range(3)]
    return F(np.max(np.stack(s)))


def ray_state(rays, rv):
    """cyl_setup for active rays: P (world frame), -dir, D, Dq (+inf: filter off) in float32."""
    r = np.asarray(rays, F)
    o, d = r[:, :3], r[:, 3:6]
    with np.errstate(all="ignore"):
        P = np.stack([o[:, 1] * d[:, 2] - o[:, 2] * d[:, 1], o[:, 2] * d[:, 0] - o[:, 0] * d[:, 2], o[:, 0] * d[:, 1] - o[:, 1] * d[:, 0]], axis=1).astype(F)
        ad, ao = np.abs(d), np.abs(o)
        dn = (ad[:, 0] + ad[:, 1]) + ad[:, 2]
        on = (ao[:, 0] + ao[:, 1]) + ao[:, 2]
        dmax = ad.max(axis=1)
        mag = dn * (on + F(2.0) * F(rv))
        fin = (mag < F(1e37)) & (dmax > F(1e-18)) & (dmax < F(1e18))
        D = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).astype(F) * F(1.0 + 2.0 ** -21)
        dq = np.maximum(((F(2.0 ** -16) * F(1.01)) * mag) * F(1.0 + 2.0 ** -20), F(1e-37))
    z = F(0)
    return dict(P=np.where(fin[:, None], P, z), nd=np.where(fin[:, None], -d, z), D=np.where(fin, D, F(1)).astype(F),
                Dq=np.where(fin, dq, F(np.inf)).astype(F), on=fin)


def cyl_x(rec, ti, ray, ri):
    """x = |gm| - H D of the pairs (triangle ti[k], ray ri[k]): cyl_x with the ray moment rotated to the triangle's class"""
    a = rec["a"][ti]
    b, c = (a + 1) % 3, (a + 2) % 3
    P, nd = ray["P"][ri], ray["nd"][ri]
    k = np.arange(ti.shape[0])
    gm = fma(rec["beta"][ti], P[k, b], P[k, a])
    gm = fma(rec["gamma"][ti], P[k, c], gm)
    for q in range(3):
        gm = fma(nd[:, q], rec["mc"][ti, q], gm)
    return fma(-rec["H"][ti], ray["D"][ri], np.abs(gm))


def survives(rec, ti, ray, ri, margins=1):
    """The kernel's verdict: the sign bit of x - margins * Dq is set, or the difference is a NaN (cylm_retest: margins = 2; the
    per-triangle form of stage 1 in f32: margins = 1)."""
    x = cyl_x(rec, ti, ray, ri)
    Dq = ray["Dq"][ri]
    with np.errstate(all="ignore"):
        m = Dq + Dq if margins == 2 else Dq
        diff = (x - m).astype(F)
    return ~(diff >= 0), x
