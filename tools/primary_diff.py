"""Per-pixel diff of the primary rays' walk against the oracle: which pixel's ray left the reference, and where.

For one of bench.py's configurations at a small size, takes the GPU's per-ray records of one sample of every pixel
(HipRayCaster.primary_records: the production walk itself, in its recording mode) and traces each pixel's ray alone in the
oracle.  A pixel differs when its ray bits, hit triangle, t, face or any of the five work counters differ, or when the
sizes of its visited leaves' lists do not sum to the oracle's tri_tests.  Prints the count and the first differences with
their visited leaves; exit status 1 when any pixel differs.

    python tools/primary_diff.py --config 3 --size 64 --spp 1 --sample 0
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

COUNTERS = ("box_tests", "tri_tests", "full_tests", "nodes", "leaves")


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--config", type=int, default=3, choices=(3, 4, 5), help="bench.py configuration (3, 4: canonical scene, 5: grid)")
    ap.add_argument("--size", type=int, default=64, help="width = height")
    ap.add_argument("--spp", type=int, default=1, help="samples per pixel of the frame")
    ap.add_argument("--sample", type=int, default=0, help="which sample of every pixel")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--show", type=int, default=5, help="differences to print in full")
    args = ap.parse_args()

    from conftest import build_pair, recipe_canonical, recipe_grid
    from oracle import orc
    from rust_raytrace_amd import raytrace as R

    so, sp = build_pair(recipe_grid() if args.config == 5 else recipe_canonical())
    w = h = args.size
    vp = R.canonical_viewport(w, h, 5, args.spp)
    rec = R.HipRayCaster(seed=args.seed, device=args.device).primary_records(vp, sp, 0, h, args.sample)
    o4, d4 = orc.primary_rays(w, h, orc.canonical_viewport(w, h), args.spp, seed=args.seed)
    o4, d4 = o4[args.sample::args.spp], d4[args.sample::args.spp]
    _, topo, refs = sp.tree()
    u = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)  # noqa: E731
    diffs = []
    for i in range(w * h):
        what = []
        if not (np.array_equal(u(rec.orig[i]), u(o4[i])) and np.array_equal(u(rec.dir[i]), u(d4[i]))):
            what.append(f"ray {rec.orig[i].tolist()} {rec.dir[i].tolist()} vs {o4[i].tolist()} {d4[i].tolist()}")
        tri, t, face, cn = so.trace(o4[i:i + 1], d4[i:i + 1])
        if rec.tri[i] != tri[0] or u(rec.t[i]) != u(t[0]) or rec.face[i] != face[0]:
            what.append(f"hit ({rec.tri[i]}, {rec.t[i]!r}, face {rec.face[i]}) vs ({tri[0]}, {t[0]!r}, face {face[0]})")
        for k in COUNTERS:
            if int(rec.counters[k][i]) != cn[k]:
                what.append(f"{k} {int(rec.counters[k][i])} vs {cn[k]}")
        lv = rec.leaves(i)
        sizes = int(topo[lv, 1].astype(np.int64).sum())
        if sizes != cn["tri_tests"]:
            what.append(f"leaf list sizes sum to {sizes}, oracle tri_tests {cn['tri_tests']}")
        if what:
            diffs.append((i, what))
    print(f"config {args.config} {w}x{h} spp {args.spp} sample {args.sample} seed {args.seed}: "
          f"{len(diffs)} of {w * h} pixels differ from the oracle; {len(rec.leaf_ids)} leaves visited in all")
    for i, what in diffs[:args.show]:
        row, col = (int(x) for x in rec.pixel[i])
        print(f"pixel (row {row}, col {col}):")
        for x in what:
            print("   ", x)
        print("    visited leaves (box index: list size):", ", ".join(f"{b}:{int(topo[b, 1])}" for b in rec.leaves(i)))
    return 1 if diffs else 0


if __name__ == "__main__":
    sys.exit(main())
