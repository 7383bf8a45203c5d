"""-m gpu: batches of views (rtmi_render_views / rtmi_render_views_device, HipRayCaster.walk_rays_views).  View k of a batch
must be, bit for bit, what a single-view FRAME render of that viewport and seed gives, and the batch's work counters the sum
of those calls'.  Samp::VIEWS picks its kernels from tables of its own (path_views_variant[slow][count][fast], k_gen_views,
k_shade_views); the rows below reach every pipeline that FRAME reaches.  Exact rows are also compared with the oracle.

At 4 samples per pixel a 64-lane refill of k_path_primary takes 16 pixels; the queue's range cuts (a batch's paths split
into 8 ranges, whose bounds need not fall on a row) and the tuning rows' batch and stream cuts put pixels of two views into
one wave.  The packet cull then loses that wave, never its exactness.
Every case renders in a fresh process (case_* / run_row below); the parent compares."""
import functools
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import OracleApi, ProductApi, assert_bits_equal, recipe_canonical, recipe_circles_analytic

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, S, DEPTH = 48, 40, 4, 5
SEEDS = [3, 11, 1, 977, 42]  # one per orbit view
COUNTERS = ("rays", "box_tests", "tri_tests", "full_tests", "nodes", "leaves")
# a raw viewport whose primary rays all have an exactly-zero x component: their paths go to the slow path
SLOW_VP12 = [2.0, 0.6, 1.0, 2.0, 0.0, 0.0, 0.0, -1.2, 0.0, 0.0, 0.0, 0.5]


def _ints(stats):
    return {k: int(v) for k, v in stats.items() if isinstance(v, (int, np.integer))}


def orbit_vp12(R, w, h, k, n):
    """View k of n cameras on an arc around the canonical teapot (at (0, 0.5, 5)), the canonical field of view: 12 floats."""
    a = math.radians(-30.0 + 60.0 * k / max(n - 1, 1))
    pos = [5.0 * math.sin(a), 0.0, 5.0 - 5.0 * math.cos(a)]
    d = R.unit([0.0 - pos[0], 0.5 - pos[1], 5.0 - pos[2]])
    aspect = np.float32(h) / np.float32(w)
    return R.create_viewport((w, h), (1.0, float(np.float32(1.0) * aspect)), pos, d, 90.0, R.to_radians(0.0), 1, 1).vp12.copy()


_RUN = r"""
import json, os, sys
import numpy as np
root, name, out = sys.argv[1], sys.argv[2], sys.argv[3]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
import test_views as T
arrays, info = (T.run_row(name[4:]) if name.startswith("row_") else getattr(T, "case_" + name)())
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


CANON = dict(w=W, h=H, spp=S, slow=0)
MIXED = dict(w=8, h=6, spp=16, slow=2)  # SLOW_VP12 (every primary ray has an exactly-zero x component) twice among 4 views
ROWS = {
    "octree_counters": dict(scene="canonical", opts=("COUNTERS",), view=CANON),
    "octree_fast": dict(scene="canonical", opts=("FAST",), view=CANON),
    "octree_fast_counters": dict(scene="canonical", opts=("FAST", "COUNTERS"), view=CANON),
    "pipeline1_counters": dict(scene="canonical", opts=("COUNTERS",), tuning={"pipeline": 1}, view=CANON, pipeline=1),
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
    "slow": dict(scene="canonical", opts=("COUNTERS",), view=MIXED),
    "slow_fast": dict(scene="canonical", opts=("FAST",), view=MIXED),
    "slow_off": dict(scene="canonical", opts=("COUNTERS",), tuning={"slow_path_off": 1}, view=MIXED),
}


def _vp12s(R, g):
    """The 12 floats of every view of a row's batch: SLOW_VP12 at views 1 and 3 of the mixed batch, orbit views elsewhere."""
    n = 4 if g["slow"] else len(SEEDS)
    return [np.asarray(SLOW_VP12, np.float32) if g["slow"] and k % 2 == 1 else orbit_vp12(R, g["w"], g["h"], k, n) for k in range(n)]


# ---------------------------------------------------------------- what the child processes run
def _caster(R, row, seed):
    options = 0
    for o in row["opts"]:
        options |= getattr(R, "OPT_" + o)
    return R.HipRayCaster(seed=seed, options=options, tuning=row.get("tuning"))


def run_row(name):
    """One batch of a row's views, then every view alone (walk_rays, a FRAME render) with the same caster settings."""
    from rust_raytrace_amd import raytrace as R
    row = ROWS[name]
    g = row["view"]
    sp = _recipe(row["scene"])(ProductApi(R))
    vps = [R.Viewport(g["w"], g["h"], v, DEPTH, g["spp"]) for v in _vp12s(R, g)]
    seeds = SEEDS[:len(vps)]
    ctx = _caster(R, row, 1).walk_rays_views(vps, sp, seeds=seeds)
    arrays, info = {"batch": ctx.data}, {"batch": _ints(ctx.stats), "singles": []}
    for k, v in enumerate(vps):
        one = np.zeros((g["h"], g["w"], 4), np.float32)
        info["singles"].append(_ints(_caster(R, row, seeds[k]).walk_rays(v, sp, one, 1, False).stats))
        arrays[f"single{k}"] = one
    arrays["vp12s"] = np.stack([v.vp12 for v in vps])
    return arrays, info


def case_seeds():
    """Two identical orbit viewports: equal seeds give equal frames, different seeds different ones."""
    from rust_raytrace_amd import raytrace as R
    sp = _recipe("canonical")(ProductApi(R))
    v = R.Viewport(W, H, orbit_vp12(R, W, H, 1, 3), DEPTH, S)
    c = R.HipRayCaster(seed=5)
    same = c.walk_rays_views([v, v], sp, seeds=[7, 7]).data
    diff = c.walk_rays_views([v, v], sp, seeds=[7, 8]).data
    arrays = {"same": same, "diff": diff}
    for sd in (7, 8):
        one = np.zeros((H, W, 4), np.float32)
        R.HipRayCaster(seed=sd).walk_rays(v, sp, one, 1, False)
        arrays[f"single{sd}"] = one
    return arrays, {}


def case_single_view():
    """K = 1 is rtmi_render: bits and rays.  Also walk_rays_views with its default seeds (the caster's) into a given array."""
    from rust_raytrace_amd import raytrace as R
    sp = _recipe("canonical")(ProductApi(R))
    v = R.canonical_viewport(W, H, DEPTH, S)
    c = R.HipRayCaster(seed=9)
    data = np.full((1, H, W, 4), np.nan, np.float32)
    ctx = c.walk_rays_views([v], sp, data)
    one = np.zeros((H, W, 4), np.float32)
    st = c.walk_rays(v, sp, one, 1, False).stats
    views = [R.Viewport(W, H, orbit_vp12(R, W, H, k, 3), DEPTH, S) for k in range(3)]
    multi = c.walk_rays_views(views, sp).data
    singles = np.zeros((3, H, W, 4), np.float32)
    for k in range(3):
        c.walk_rays(views[k], sp, singles[k], 1, False)
    return ({"batch": data, "same_object": np.array([ctx.data is data]), "single": one, "multi": multi, "multi_singles": singles},
            {"batch": _ints(ctx.stats), "single": _ints(st)})


TILES = [(0, 64, 16, 32), (16, 56, 16, 32)]


def case_device_tile():
    """Two striped tiles of a 3 x 40-row stack on the device variant (stripes 32-47 and 80-95 cross views, the last stripe
    of the second tile is partial), and the host variant's whole stack."""
    import torch
    from rust_raytrace_amd import raytrace as R
    sp = _recipe("canonical")(ProductApi(R))
    views = [R.Viewport(W, H, orbit_vp12(R, W, H, k, 3), DEPTH, S) for k in range(3)]
    seeds = SEEDS[:3]
    c = R.HipRayCaster(seed=1)
    host = c.walk_rays_views(views, sp, seeds=seeds)
    dev = torch.device("cuda", 0)
    arrays, info = {"host": host.data}, {"host": _ints(host.stats), "tiles": []}
    for i, t in enumerate(TILES):
        buf = torch.full((t[1], W, 4), float("nan"), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        st = c.walk_views_device(views, sp, t, buf.data_ptr(), torch.cuda.current_stream().cuda_stream, seeds=seeds)
        torch.cuda.synchronize()
        arrays[f"tile{i}"] = buf.cpu().numpy()
        info["tiles"].append(_ints(st.stats))
    return arrays, info


def case_auto_streams():
    """16 views at 512 x 512 @ 16 = 2^26 paths: the automatic one-stream rule applies to the batch."""
    from rust_raytrace_amd import raytrace as R
    sp = _recipe("canonical")(ProductApi(R))
    n, w = 16, 512
    views = [R.Viewport(w, w, orbit_vp12(R, w, w, k, n), DEPTH, 16) for k in range(n)]
    seeds = list(range(100, 100 + n))
    ctx = R.HipRayCaster().walk_rays_views(views, sp, seeds=seeds)
    bad, rays = [], 0
    for k in range(n):
        one = np.zeros((w, w, 4), np.float32)
        rays += R.HipRayCaster(seed=seeds[k]).walk_rays(views[k], sp, one, 1, False).total_rays
        if not np.array_equal(one.view(np.uint32), ctx.data[k].view(np.uint32)):
            bad.append(k)
    return {}, {"batch": _ints(ctx.stats), "bad_views": bad, "single_rays": int(rays)}


# ---------------------------------------------------------------- the checks (parent process)
@functools.lru_cache(maxsize=None)
def _oracle_scene(scene):
    from oracle import orc
    return _recipe(scene)(OracleApi(orc))


def _oracle(scene, g, vp12, seed):
    return _oracle_scene(scene).render(g["w"], g["h"], np.asarray(vp12, np.float32), DEPTH, g["spp"], seed=seed, threads=8)


def _exact(row):
    return "FAST" not in row["opts"] and "BVH" not in row["opts"]


def _check_row(tmp_path, name):
    row = ROWS[name]
    a, info = _run(tmp_path, name="row_" + name)
    g = row["view"]
    n = a["batch"].shape[0]
    batch, singles = info["batch"], info["singles"]
    counting = "COUNTERS" in row["opts"]
    assert batch["pipeline"] == row.get("pipeline", 3), batch["pipeline"]
    for k in range(n):
        assert_bits_equal(a["batch"][k], a[f"single{k}"], f"{name}: view {k} of the batch vs its single render")
    for key in COUNTERS if counting else ("rays",):
        assert batch[key] == sum(s[key] for s in singles), (name, key, batch[key], [s[key] for s in singles])
    work = "tri_tests" if row["scene"] == "trivial" else "box_tests"
    assert (batch[work] > 0) == counting, (work, batch[work])
    if g["slow"]:
        assert batch["slow_paths"] == sum(s["slow_paths"] for s in singles), (batch["slow_paths"], [s["slow_paths"] for s in singles])
        if "slow_path_off" in row.get("tuning", {}):
            assert batch["slow_paths"] == 0
        else:
            assert batch["slow_paths"] > 0
    if _exact(row):
        for k in range(n):
            ref, cn = _oracle(row["scene"], g, a["vp12s"][k], SEEDS[k])
            assert_bits_equal(a["batch"][k], ref, f"{name}: view {k} vs oracle")
            if counting:
                for key in COUNTERS:
                    assert singles[k][key] == cn[key], (name, k, key, singles[k][key], cn[key])
    return a, info


def test_oracle_parity(tmp_path):
    """Canonical scene, 48 x 40 @ 4, depth 5, 5 orbit views with 5 seeds: every view is the oracle's image, the summed
    counters the oracle's sum."""
    from oracle import orc  # noqa: F401
    a, info = _check_row(tmp_path, "octree_counters")
    row = ROWS["octree_counters"]
    sums = {k: 0 for k in COUNTERS}
    for k in range(a["batch"].shape[0]):
        cn = _oracle(row["scene"], row["view"], a["vp12s"][k], SEEDS[k])[1]
        for key in COUNTERS:
            sums[key] += cn[key]
    for key in COUNTERS:
        assert info["batch"][key] == sums[key], (key, info["batch"][key], sums[key])


@pytest.mark.parametrize("name", [n for n in ROWS if n != "octree_counters" and not n.startswith("slow")])
def test_variant_matrix(tmp_path, name):
    _check_row(tmp_path, name)


@pytest.mark.parametrize("name", ["slow", "slow_fast", "slow_off"])
def test_slow_path_views(tmp_path, name):
    """8 x 6 @ 16: SLOW_VP12 views beside orbit views, with the slow path on and off."""
    _check_row(tmp_path, name)


def test_seeds(tmp_path):
    a, _ = _run(tmp_path, "seeds")
    assert_bits_equal(a["same"][0], a["same"][1], "equal seeds")
    assert not np.array_equal(a["diff"][0].view(np.uint32), a["diff"][1].view(np.uint32)), "different seeds gave equal frames"
    assert_bits_equal(a["diff"][0], a["single7"], "seed 7 vs its single render")
    assert_bits_equal(a["diff"][1], a["single8"], "seed 8 vs its single render")


def test_single_view_is_rtmi_render(tmp_path):
    a, info = _run(tmp_path, "single_view")
    assert_bits_equal(a["batch"][0], a["single"], "K = 1 vs rtmi_render")
    assert info["batch"]["rays"] == info["single"]["rays"]
    assert bool(a["same_object"][0]), "walk_rays_views must fill the array it is given"
    assert_bits_equal(a["multi"], a["multi_singles"], "walk_rays_views (caster's seed) vs walk_rays per view")


def test_device_tiles_interleave_to_the_host_stack(tmp_path):
    a, info = _run(tmp_path, "device_tile")
    stack = a["host"].reshape(3 * H, W, 4)
    got = np.full_like(stack, np.nan)
    for i, (row0, nrows, sr, step) in enumerate(TILES):
        rows = [row0 + (L // sr) * step + L % sr for L in range(nrows)]
        got[rows] = a[f"tile{i}"]
    assert_bits_equal(got, stack, "two device tiles vs the host variant's stack")
    assert sum(t["rays"] for t in info["tiles"]) == info["host"]["rays"]


def test_automatic_stream_rule_applies_to_the_batch(tmp_path):
    _, info = _run(tmp_path, "auto_streams")
    assert info["batch"]["streams"] == 1, info["batch"]["streams"]
    assert info["bad_views"] == [], info["bad_views"]
    assert info["batch"]["rays"] == info["single_rays"]
