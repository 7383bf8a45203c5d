"""-m gpu: every sampling mode on every kernel variant.  Frame (Samp::FRAME), progressive passes (Samp::PASS) and adaptive
passes (Samp::LIST) share every kernel body; rtmi_device.hip picks the variant from tables:
path_variant[slow][mode == PASS][count][fast], path_list_variant[slow][count][fast], trace_oct_variant[count][fast] and the
`count ?` picks of k_trace_linear, k_trace and k_trace_bvh.  A wrong `count` cell still gives a bit-exact image and a wrong
`fast` cell changes no pixel at these sizes, so every row also checks the work counters, and the FAST rows show that their
cell was taken by counting fewer box tests (or nodes) than the exact traversal.

Each row (scene, options, tuning, viewport) renders in a fresh process:
  FRAME  one walk_rays call at S samples (and at every count the adaptive run produced),
  PASS   uneven progressive passes [0,1) [1,3) [3,8) [8,16),
  LIST   adaptive at abs_tol = NaN (every pixel runs to S), and at a tolerance from test_adaptive.pick_tol on the device
         variant, whose count map, accum and sumsq are checked against the float32 replay of the sample colours.
The parent checks: PASS's final out and accum * (1/S) are FRAME's bits; LIST at NaN is FRAME; LIST at the picked tolerance is
the replay and every pixel is FRAME at its own count; the counters summed over the PASS passes, and those of LIST at NaN, are
FRAME's; exact rows (everything but FAST and BVH) are the oracle's image and counters.  FAST rows are compared with the FAST
FRAME only: FAST changes which boxes a ray visits, never how a ray's result or counts depend on its batch, wave or mode.

Row                               path cells [slow][count][fast] (PASS and LIST)   other variants reached in PASS / LIST
octree_counters                   [0][1][0]                                        k_trace_oct<1,0>
octree_fast                       [0][0][1]                                        k_trace_oct<0,1>
octree_fast_counters              [0][1][1]                                        k_trace_oct<1,1>
slow (SLOW_VP12, 8x6)             [1][0][0], [0][0][0]                             k_trace_oct<0,0>
slow_counters                     [1][1][0], [0][1][0]                             k_trace_oct<1,0>
slow_fast                         [1][0][1], [0][0][1]                             k_trace_oct<0,1>
slow_fast_counters                [1][1][1], [0][1][1]                             k_trace_oct<1,1>
slow_off (slow_path_off = 1)      [0][0][0], slow rays traced in the primary kernel; slow_paths == 0
pipeline1_fast_counters           -- (k_gen_list / k_shade_list)                   k_trace_oct<1,1>
generic, generic_counters         --                                               k_trace<0>, k_trace<1>
linear_counters (accel trivial)   --                                               k_trace_linear<1>
bvh_counters                      --                                               k_trace_bvh<1>
analytic_counters                 --                                               k_trace_oct<1,0> + k_trace_spheres
tune_* (six tuning sets)          [0][0][0] with other waves, refills, XCD ranges, streams and batches below a wave
"""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import (OracleApi, ProductApi, assert_bits_equal, recipe_canonical, recipe_circles_analytic)
from test_adaptive import COUNTERS, SLOW_VP12, _ints, _sample_colours, _viewport, pick_tol, replay

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, S, M, P, DEPTH, SEED = 48, 40, 16, 4, 4, 5, 3
PASSES = [(0, 1), (1, 2), (3, 5), (8, 8)]  # (sample0, nsamples): [0,1) [1,3) [3,8) [8,16)
SLOW = dict(w=8, h=6, vp12=SLOW_VP12)
CANON = dict(w=W, h=H, vp12=None)

# name: scene, options (names of R.OPT_*), tuning, viewport, pipeline that must run, whether the frame has slow paths
ROWS = {
    "octree_counters": dict(scene="canonical", opts=("COUNTERS",), view=CANON),
    "octree_fast": dict(scene="canonical", opts=("FAST",), view=CANON),
    "octree_fast_counters": dict(scene="canonical", opts=("FAST", "COUNTERS"), view=CANON),
    "slow": dict(scene="canonical", opts=(), view=SLOW, slow=True),
    "slow_counters": dict(scene="canonical", opts=("COUNTERS",), view=SLOW, slow=True),
    "slow_fast": dict(scene="canonical", opts=("FAST",), view=SLOW, slow=True),
    "slow_fast_counters": dict(scene="canonical", opts=("FAST", "COUNTERS"), view=SLOW, slow=True),
    "slow_off": dict(scene="canonical", opts=("COUNTERS",), tuning={"slow_path_off": 1}, view=SLOW),
    "pipeline1_fast_counters": dict(scene="canonical", opts=("FAST", "COUNTERS"), tuning={"pipeline": 1}, view=CANON, pipeline=1),
    "generic": dict(scene="canonical", opts=("GENERIC",), view=CANON, pipeline=1),
    "generic_counters": dict(scene="canonical", opts=("GENERIC", "COUNTERS"), view=CANON, pipeline=1),
    "linear_counters": dict(scene="trivial", opts=("COUNTERS",), view=CANON, pipeline=1),
    "bvh_counters": dict(scene="canonical", opts=("BVH", "COUNTERS"), view=CANON, pipeline=1),
    "analytic_counters": dict(scene="analytic", opts=("COUNTERS",), view=CANON, pipeline=1),
    "tune_xcd1": dict(scene="canonical", opts=(), tuning={"xcd_aware": 1}, view=CANON),
    "tune_xcd2_one_stream": dict(scene="canonical", opts=(), tuning={"xcd_aware": 2, "streams": 1}, view=CANON),
    "tune_one_wave_per_cu": dict(scene="canonical", opts=(), tuning={"oct_waves_per_cu": 1}, view=CANON),
    "tune_refill_1": dict(scene="canonical", opts=(), tuning={"refill_min0": 1, "refill_min": 1}, view=CANON),
    "tune_refill_64": dict(scene="canonical", opts=(), tuning={"refill_min0": 64, "refill_min": 64}, view=CANON),
    "tune_small_batches": dict(scene="canonical", opts=(), tuning={"streams": 4, "batch_paths": 40, "subtile_min_paths": 1}, view=CANON),
}

_RUN = r"""
import json, os, sys
import numpy as np
root, name, out = sys.argv[1], sys.argv[2], sys.argv[3]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
import test_sampling_matrix as T
arrays, info = T.run_row(name)
np.savez(out + ".npz", **arrays)
with open(out + ".json", "w") as f:
    json.dump(info, f)
"""


def _run(tmp_path, name):
    out = str(tmp_path / name)
    subprocess.run([sys.executable, "-c", _RUN, ROOT, name, out], check=True, timeout=900)
    with open(out + ".json") as f:
        info = json.load(f)
    with np.load(out + ".npz") as z:
        return {k: z[k] for k in z.files}, info


def _recipe(scene):
    return {"canonical": recipe_canonical(), "trivial": recipe_canonical(accel="trivial"), "analytic": recipe_circles_analytic()}[scene]


# ---------------------------------------------------------------- what the child process runs
def run_row(name):
    import torch
    from rust_raytrace_amd import raytrace as R
    row = ROWS[name]
    w, h, vp12 = row["view"]["w"], row["view"]["h"], row["view"]["vp12"]
    sp = _recipe(row["scene"])(ProductApi(R))
    options = 0
    for o in row["opts"]:
        options |= getattr(R, "OPT_" + o)
    c = R.HipRayCaster(seed=SEED, options=options, tuning=row.get("tuning"))
    vp = _viewport(R, w, h, S, vp12, DEPTH)
    arrays, info = {}, {}

    # FRAME
    frame = np.zeros((h, w, 4), np.float32)
    info["frame"] = _ints(c.walk_rays(vp, sp, frame, 1, False).stats)
    arrays["frame"] = frame

    # PASS: accum starts as NaN (sample0 == 0 must not read it); out only from the last pass
    accum = np.full((h, w, 4), np.nan, np.float32)
    out = np.zeros((h, w, 4), np.float32)
    info["passes"] = []
    for i, (k0, n) in enumerate(PASSES):
        last = i == len(PASSES) - 1
        info["passes"].append(_ints(c.walk_samples(vp, sp, 0, h, k0, n, accum, out if last else None).stats))
    arrays.update(pass_out=out, pass_accum=accum)

    # LIST at abs_tol = NaN (host variant)
    img = np.zeros((h, w, 4), np.float32)
    ctx = c.walk_rays_adaptive(vp, sp, img, min_samples=M, pass_samples=P, rel_tol=0.0, abs_tol=float("nan"))
    arrays.update(nan_img=img, nan_counts=ctx.counts)
    info["nan"] = {"stats": _ints(ctx.stats), "passes": ctx.passes, "samples": int(ctx.samples), "unconverged": ctx.unconverged}

    # LIST at a picked tolerance (device variant: accum and sumsq come back too)
    cols = _sample_colours(c, R, sp, w, h, S, vp12, DEPTH)
    rel, ab = pick_tol(cols, M, P)
    dev = torch.device("cuda", 0)
    bufs = {k: torch.full((h, w, 4), float("nan"), dtype=torch.float32, device=dev) for k in ("accum", "sumsq", "out")}
    cnt = torch.zeros((h, w), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    d = c.walk_adaptive_device(vp, sp, (0, h, h, 0), bufs["accum"].data_ptr(), bufs["sumsq"].data_ptr(), cnt.data_ptr(),
                               bufs["out"].data_ptr(), None, M, P, rel, ab)
    torch.cuda.synchronize()
    for k, t in bufs.items():
        arrays["list_" + k] = t.cpu().numpy()
    counts = cnt.cpu().numpy().view(np.uint32)
    arrays.update(list_counts=counts, cols=cols)
    info["list"] = {"stats": _ints(d.stats), "passes": d.passes, "samples": int(d.samples), "unconverged": d.unconverged,
                    "tol": [rel, ab]}

    # FRAME at every count the adaptive run produced
    for n in np.unique(counts).tolist():
        one = np.zeros((h, w, 4), np.float32)
        c.walk_rays(_viewport(R, w, h, n, vp12, DEPTH), sp, one, 1, False)
        arrays[f"frame{n}"] = one
    return arrays, info


# ---------------------------------------------------------------- the checks (parent process)
@functools.lru_cache(maxsize=None)
def _oracle_scene(scene):
    from oracle import orc
    return _recipe(scene)(OracleApi(orc))


@functools.lru_cache(maxsize=None)
def _oracle(scene, view, spp):
    """(image, counters) of the oracle; view: "canonical" (48x40) or "slow" (SLOW_VP12, 8x6)."""
    from oracle import orc
    g = SLOW if view == "slow" else CANON
    vo = orc.canonical_viewport(g["w"], g["h"]) if g["vp12"] is None else np.asarray(g["vp12"], np.float32)
    return _oracle_scene(scene).render(g["w"], g["h"], vo, DEPTH, spp, seed=SEED, threads=8)


def _exact(row):
    return "FAST" not in row["opts"] and "BVH" not in row["opts"]


@pytest.mark.parametrize("name", list(ROWS))
def test_sampling_modes_agree(tmp_path, name):
    row = ROWS[name]
    a, info = _run(tmp_path, name)
    h, w = a["frame"].shape[:2]
    counting = "COUNTERS" in row["opts"]
    frame = info["frame"]
    runs = [("frame", frame), ("nan", info["nan"]["stats"]), ("list", info["list"]["stats"])]
    runs += [(f"pass {k}", p) for k, p in enumerate(info["passes"])]

    # each row ran what it claims: the pipeline, the slow path, the counting kernels
    for what, st in runs:
        assert st["pipeline"] == row.get("pipeline", 3), (what, st["pipeline"])
        if row.get("slow"):
            assert st["slow_paths"] > 0, (what, st["slow_paths"])
        elif "slow_path_off" in row.get("tuning", {}):
            assert st["slow_paths"] == 0, (what, st["slow_paths"])
    # the counting kernels ran exactly when counting (a linear list has no boxes: its work is triangle tests)
    work = "tri_tests" if row["scene"] == "trivial" else "box_tests"
    for what, st in (("frame", frame), ("nan", info["nan"]["stats"]), ("list", info["list"]["stats"])):
        assert (st[work] > 0) == counting, (what, work, st[work])
    assert (sum(p[work] for p in info["passes"]) > 0) == counting

    # PASS: the final preview and the running sums are FRAME's bits; so are the summed counters
    assert_bits_equal(a["pass_out"], a["frame"], "PASS: final out vs FRAME")
    assert_bits_equal(a["pass_accum"] * (np.float32(1) / np.float32(S)), a["frame"], "PASS: accum * (1/S) vs FRAME")
    for k in COUNTERS:
        assert sum(p[k] for p in info["passes"]) == frame[k], ("PASS", k)

    # LIST at NaN: every pixel runs to S in passes and ends in FRAME's bits and counters
    nan = info["nan"]
    assert_bits_equal(a["nan_img"], a["frame"], "LIST at NaN vs FRAME")
    assert (a["nan_counts"] == S).all()
    assert nan["passes"] == 1 + -(-(S - M) // P) and nan["samples"] == S * w * h and nan["unconverged"] == w * h
    for k in COUNTERS:
        assert nan["stats"][k] == frame[k], ("LIST at NaN", k)

    # LIST at the picked tolerance: the float32 replay's count map, sums and schedule; every pixel FRAME at its count
    lst = info["list"]
    rel, ab = lst["tol"]
    counts, acc, sq, passes, unconverged = replay(a["cols"], M, P, rel, ab)
    u = np.unique(counts).tolist()
    assert M in u and S in u and len(u) >= 3, u
    assert np.array_equal(a["list_counts"], counts), f"LIST: {int((a['list_counts'] != counts).sum())} counts differ from the replay"
    assert_bits_equal(a["list_accum"], acc, "LIST: accum vs replay")
    assert_bits_equal(a["list_sumsq"], sq, "LIST: sumsq vs replay")
    assert (lst["passes"], lst["samples"], lst["unconverged"]) == (passes, int(counts.sum()), unconverged)
    for n in u:
        sel = counts == n
        assert_bits_equal(a["list_out"][sel], a[f"frame{n}"][sel], f"LIST: pixels with {n} samples vs FRAME at {n}")

    view = "slow" if row["view"] is SLOW else "canonical"
    if _exact(row):
        # the exact traversals: FRAME (and so every mode above) is the oracle's image and work, at S and every count
        ref, cn = _oracle(row["scene"], view, S)
        assert_bits_equal(a["frame"], ref, "FRAME vs oracle")
        for k in COUNTERS if counting else ("rays",):
            assert frame[k] == cn[k], ("FRAME vs oracle", k, frame[k], cn[k])
        for n in u:
            assert_bits_equal(a[f"frame{n}"], _oracle(row["scene"], view, n)[0], f"FRAME at {n} vs oracle")
    elif "FAST" in row["opts"] and counting:
        # the fast cell was taken: fewer boxes (or nodes) than the exact traversal (the oracle's counts, which the exact
        # rows above show to be the product's)
        cn = _oracle(row["scene"], view, S)[1]
        assert frame["box_tests"] < cn["box_tests"] or frame["nodes"] < cn["nodes"], (frame, cn)
