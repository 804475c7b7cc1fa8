#!/usr/bin/env python3
"""Which cylinder should stage 2 of the default scan re-test with?  A numpy model, no GPU ("the re-test's cylinder").

Stage 1 keeps a group of four triangles when the ray may hit the cylinder around the LONGEST edge's slab of one of them.  The re-test
then decides which triangles of a listed group go on to the exact test.  Re-testing with the same cylinder (each triangle's own H)
does little more than name the triangle that set the group bit; the cylinder around a SECOND slab of the same triangle is an
independent necessary condition and rejects most of them.  This script counts, on closed_room(N) with bounce-like rays (origins on
random triangles, random directions), the exact-test candidates per list entry for each choice, with the records, the f32 ray state
and the five-term chain of tests/retest_model.py (the kernel's roundings):

    python tools/retest_edge_model.py [--tris 10000] [--rays 1500] [--seed 1]

Groups are quads in the stream's order (class, then ascending H of the longest edge's cylinder); the big class (H >= S / 64, at most
64 triangles: the room itself) is left out, as in the kernel.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import retest_model as M                     # noqa: E402
from spath_amd import scene                  # noqa: E402

F = np.float32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tris", type=int, default=10000)
    ap.add_argument("--rays", type=int, default=1500)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    rng = np.random.default_rng(args.seed)
    t = scene.closed_room(args.tris)[0]
    n = t.shape[0]
    rv = M.scene_bound(t)
    S = 2.0 ** (np.floor(np.log2(float(rv))) + 2)
    A, _ = M.records(t, "A")
    big = np.isfinite(A["H"]) & (A["H"] / F(S) >= F(1.0 / 64))
    assert big.sum() <= 64
    # bounce-like rays: from a random point of a random triangle, in a random direction
    k = rng.integers(0, n, args.rays)
    bc = rng.dirichlet([1, 1, 1], args.rays)
    o = (t[k, :9].reshape(-1, 3, 3).astype(np.float64) * bc[:, :, None]).sum(axis=1)
    d = rng.normal(size=(args.rays, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.concatenate([o, d], axis=1).astype(F)
    ray = M.ray_state(rays, rv)
    # the stream: class, then ascending H (stable), quads
    keep = np.flatnonzero(~big)
    order = keep[np.lexsort((keep, A["H"][keep], A["a"][keep]))]
    groups = []
    for c in range(3):
        oc = order[A["a"][order] == c]
        pad = (-oc.shape[0]) % 4
        groups.append(np.concatenate([oc, np.full(pad, -1)]).reshape(-1, 4))
    grp = np.concatenate(groups)                                   # [group, place] -> triangle index, -1 = padding
    ng = grp.shape[0]
    real = grp >= 0
    gi = np.maximum(grp, 0).reshape(-1)

    def verdicts(rec, margins):
        out = np.zeros((args.rays, ng, 4), dtype=bool)
        for r0 in range(0, args.rays, 64):
            nr = min(64, args.rays - r0)
            ri = np.repeat(np.arange(r0, r0 + nr), gi.shape[0])
            s, _ = M.survives(rec, np.tile(gi, nr), ray, ri, margins)
            out[r0:r0 + nr] = s.reshape(nr, ng, 4) & real[None]
        return out

    s1 = verdicts(A, 1)                                            # stage 1, per triangle with its own H
    listed = s1.any(axis=2)                                        # [ray, group]
    entries = int(listed.sum())
    print(f"closed_room({args.tris}): {n} triangles, {int(big.sum())} in the big class, {ng} groups of four; {args.rays} rays, "
          f"{entries / args.rays:.1f} list entries per scan, {s1.sum() / (args.rays * real.sum()):.4%} of the pairs survive stage 1")
    print("re-test uses                         | margin | exact-test candidates per list entry")
    for name, rule in (("cylinder A, own H (before)", "A"), ("second-longest edge's cylinder", "second"), ("third edge's cylinder", "third"),
                       ("the kernel's rule (cyl_retest_record)", "kernel")):
        _, R = M.records(t, rule)
        for margins in ((1,) if rule == "A" else (1, 2)):
            cand = verdicts(R, margins) & listed[:, :, None]
            print(f"{name:37s}| {'Dq' if margins == 1 else '2 Dq':6s} | {cand.sum() / entries:.3f}")


if __name__ == "__main__":
    main()
