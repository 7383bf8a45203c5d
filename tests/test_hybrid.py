"""-m gpu: the hybrid bounce passes (hybrid.hpp; DESIGN.md 4.1 "Hybrid pass"): k_hybrid_bvh proposes, k_oct_verify confirms,
k_trace_oct_list walks the fallback list exactly.  One fresh process per setting (RTMI_HYBRID unset, = 0: read at scene
creation) renders and traces everything below; the tests compare image bits, "Rays", the counting build's counters and the
traced hits between the two and with the oracle, and read the passes' statistics (rth_debug_hybrid_counters)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import assert_bits_equal, recipe_axis_box, recipe_canonical, recipe_grid

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTERS = ("box_tests", "tri_tests", "full_tests", "nodes", "leaves")
CANON = dict(w=64, h=64, spp=4, depth=5, seed=1)
GRID = dict(w=32, h=32, spp=4, depth=5, seed=7, size=(1.0, 1.0), pos=[0.0, 0.0, -2.0], dir=[0.0, 0.0, 1.0], fov=16.0, roll=0.0)
# DCtrl::hyb (hybrid.hpp)
OFFERED, REFUSED, MISSES, TIES, F_ABSENT, F_NOCOLLIDE, F_TMIN, F_NOTRI, FALLBACKS, VIOLATIONS, F_BOUNDS, CONFIRMED = range(12)


def recipe_cluster(extra):
    """24 small triangles inside the cell [0.5, 1]^3 of a root box (centre 0, half 1): octant 7 of the root is an inner box at
    depth 1 over one at depth 2 over leaves (the cluster of test_node_cull.recipe_three_levels); extra(api, s) adds the
    triangles the test is about."""
    def r(api):
        s = api.scene()
        rng = np.random.default_rng(3)
        surfs = [api.matte((200, 120, 40), 0.3), api.reflective(0.01, (220, 220, 230), 0.6)]
        for k in range(24):
            c = rng.uniform(0.6, 0.9, 3)
            tri = (c + rng.uniform(-0.08, 0.08, (3, 3))).clip(0.52, 0.98).astype(np.float32)
            api.add_triangle(s, tri, surfs[k % 2], 0.0)
        extra(api, s)
        s.populate_triangle_numbers()
        s.build_bounding_box([0.0, 0.0, 0.0], 1.0, 3, 2)
        return s
    return r


DUP = np.array([[-0.9, -0.9, -0.5], [0.9, -0.9, -0.5], [0.1, 0.9, -0.45]], np.float32)


def recipe_duplicate():
    """... and the same triangle twice (two records, one geometry) across the front of the root box: every ray that hits it
    ties exactly."""
    def extra(api, s):
        api.add_triangle(s, DUP, api.matte((90, 90, 200), 0.5), 0.0)
        api.add_triangle(s, DUP, api.solid((10, 200, 10)), 0.0)
    return recipe_cluster(extra)


BIG = np.array([[-6.0, -5.0, -0.5], [6.0, -5.5, -0.4], [0.3, 7.0, -0.6]], np.float32)
# corners with x - y constant: the normal is (a, -a, 0) bit for bit, and a direction (u, u, w) has den == 0 exactly
DIAG = np.array([[-0.5, -1.0, -0.75], [0.75, 0.25, -0.75], [0.125, -0.375, 0.5]], np.float32)


def recipe_big():
    """... a large triangle of which the root box (half 1) covers only the middle, and one whose plane holds directions
    without a zero component."""
    def extra(api, s):
        api.add_triangle(s, BIG, api.matte((90, 90, 200), 0.5), 0.0)
        api.add_triangle(s, DIAG, api.matte((200, 90, 90), 0.5), 0.0)
    return recipe_cluster(extra)


def _rays(o, d):
    o4, d4 = np.zeros((len(o), 4), np.float32), np.zeros((len(o), 4), np.float32)
    o4[:, :3], d4[:, :3] = o, d
    return o4, d4


def dup_rays():
    """onto the duplicated triangle (its middle: every one hits both records), none with a zero direction component"""
    rng = np.random.default_rng(17)
    n = 300
    w = rng.dirichlet([2, 2, 2], n)
    p = w @ DUP.astype(np.float64)
    o = p + np.array([0.0, 0.0, -2.0]) + rng.normal(size=(n, 3)) * 0.3
    d = p - o
    return _rays(o, d / np.linalg.norm(d, axis=1, keepdims=True))


def big_rays():
    """onto the large triangle: hit points all over it, most of them outside the root box"""
    rng = np.random.default_rng(18)
    n = 400
    w = rng.dirichlet([1, 1, 1], n)
    p = w @ BIG.astype(np.float64)
    o = p + np.array([0.0, 0.0, -3.0]) + rng.normal(size=(n, 3)) * 0.5
    d = p - o
    return _rays(o, d / np.linalg.norm(d, axis=1, keepdims=True)), p


def refused_rays(parallel=True):
    """Rays the certificate must refuse: the poisoned and zero-component rays of test_gpu_parity.test_trace_edge_case_rays
    (NaN, inf, a zero direction component, a nonzero lane 3) and, with `parallel`, rays without a zero component that are
    exactly parallel to the plane of DIAG (refused in the scene that holds it)."""
    rays = []
    for ox in (-1.0, -0.5, 0.0, 0.25, 1.0):
        for oy in (-1.0, 0.0, 0.25, 0.5):
            for dvec in ((0, 0, 1), (0, 0, -1), (1, 0, 0), (0, 1, 0), (0, -1, 0), (-1, 0, 0), (0.6, 0, 0.8), (0, 0.6, 0.8),
                         (-0.0, 0.0, 1.0), (1e-30, 0, 1)):
                rays.append(((ox, oy, 3.5, 0.0), (*dvec, 0.0)))
                rays.append(((ox, oy, 5.0, 0.0), (*dvec, 0.0)))
                rays.append(((-1.0, oy, 4.0, 0.0), (*dvec, 0.0)))
    rays += [((0, 0, 0, 0), (np.nan, 0, 1, 0)), ((np.nan, 0, 0, 0), (0, 0, 1, 0)), ((0, 0, 0, np.nan), (0, 0, 1, 0)),
             ((0, 0, 0, 0), (0, 0, 1, np.nan)), ((np.inf, 0, 0, 0), (0, 0, 1, 0)), ((0, 0, 0, 0), (0, 0, 0, 0)),
             ((0.1, 0.2, -3.0, 1e-3), (0.1, 0.2, 0.97, 0.0)), ((0.1, 0.2, -3.0, 0.0), (0.1, 0.2, 0.97, 1e-3)),
             ((0.1, 0.2, -3.0, 0.0), (np.inf, 0.2, 0.97, 0.0)), ((0.1, 0.2, -3.0, 0.0), (0.1, -np.inf, 0.97, 0.0))]
    for u, w in ((0.5, 0.70710678), (-0.5, 0.70710678), (0.1, -0.98994949), (0.70710678, 1e-3)) if parallel else ():
        for o in ((0.0, -0.4, -3.0), (0.3, -0.1, -0.5), (-2.0, -2.4, -0.2), (0.0, 0.0, -3.0)):
            rays.append(((*o, 0.0), (u, u, w, 0.0)))
    return np.array([r[0] for r in rays], np.float32), np.array([r[1] for r in rays], np.float32)


def far_rays():
    """Rays aimed at the edges of the 12 recorded triangles of the canonical scene (tests/golden/canonical_triangle_records.npz)
    from 10^0 .. 10^6 away: the reference decides on the rounded hit point, which parts from the line the BVH tests as the origin
    recedes -- beyond the origin bound (hybrid.hpp) the hybrid must refuse the ray."""
    import test_hybrid_cpu as H
    rec = np.load(os.path.join(ROOT, "tests", "golden", "canonical_triangle_records.npz"))["rec"]
    rng = np.random.default_rng(77)
    o, d = [], []
    for r in rec:
        for dist in (1.0, 10.0, 1e2, 1e3, 1e4, 1e5, 1e6):
            a, b = H.edge_rays(r, rng, 400, dist)
            o.append(a); d.append(b)
    return _rays(np.concatenate(o), np.concatenate(d))


_RUN = r"""
import ctypes as C, json, os, sys
import numpy as np
root, out = sys.argv[1], sys.argv[2]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
from rust_raytrace_amd import raytrace as R, _ffi
from conftest import ProductApi, recipe_axis_box, recipe_canonical, recipe_grid
import test_hybrid as T
L = _ffi.lib()
L.rth_debug_hybrid_counters.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
res, arrays = {}, {}

def hyb(sp):
    d, on = (C.c_ulonglong * 12)(), C.c_int(0)
    assert L.rth_debug_hybrid_counters(sp.h, d, C.byref(on)) == 0
    return [int(x) for x in d], int(on.value)

def render(name, sp, vp, w, h, seed, pipe, counting):
    img = np.zeros((h, w, 4), np.float32)
    c = R.HipRayCaster(seed=seed, options=R.OPT_COUNTERS if counting else 0, tuning={"pipeline": pipe})
    ctx = c.walk_rays(vp, sp, img, 1, False)
    key = f"{name}_p{pipe}_c{int(counting)}"
    arrays[key] = img
    r = {"total_rays": int(ctx.total_rays), "stats": {k: int(v) for k, v in ctx.stats.items() if isinstance(v, (int, np.integer))}}
    r["hyb"], r["on"] = hyb(sp)
    res[key] = r

def trace(name, sp, o4, d4, counting=False):
    tri, t, face, st = R.HipRayCaster(options=R.OPT_COUNTERS if counting else 0).trace(sp, o4, d4)
    arrays[name + "_tri"], arrays[name + "_t"], arrays[name + "_face"] = tri, t, face
    r = {"stats": {k: int(v) for k, v in st.items() if isinstance(v, (int, np.integer))}}
    r["hyb"], r["on"] = hyb(sp)
    res[name] = r

sp = recipe_canonical()(ProductApi(R))
k = T.CANON
for pipe in (3, 1):
    for counting in (False, True):
        render("canonical", sp, R.canonical_viewport(k["w"], k["h"], k["depth"], k["spp"]), k["w"], k["h"], k["seed"], pipe, counting)
trace("far", sp, *T.far_rays())
trace("far_counting", sp, *T.far_rays(), True)
trace("axis_refused", recipe_axis_box()(ProductApi(R)), *T.refused_rays(False))
big = T.recipe_big()(ProductApi(R))
trace("big_refused", big, *T.refused_rays())
(bo, bd), _ = T.big_rays()
trace("big", big, bo, bd)
trace("big_counting", big, bo, bd, True)
dup = T.recipe_duplicate()(ProductApi(R))
trace("dup", dup, *T.dup_rays())
trace("dup_counting", dup, *T.dup_rays(), True)
g = T.GRID
vg = R.create_viewport((g["w"], g["h"]), g["size"], g["pos"], R.unit(g["dir"]), g["fov"], g["roll"], g["depth"], g["spp"])
render("grid", recipe_grid()(ProductApi(R)), vg, g["w"], g["h"], g["seed"], 3, False)
np.savez(out + ".npz", **arrays)
json.dump(res, open(out + ".json", "w"))
"""


def _run(tmp, setting):
    env = dict(os.environ)
    for k in ("RTMI_HYBRID", "RTMI_NODE_CULL", "RTMI_BLOCK_CULL", "RTMI_BLOCK_CULL_N"):
        env.pop(k, None)
    if setting is not None:
        env["RTMI_HYBRID"] = setting
    out = str(tmp / f"hyb_{setting}")
    subprocess.run([sys.executable, "-c", _RUN, ROOT, out], env=env, check=True, timeout=300)
    with open(out + ".json") as f:
        return dict(np.load(out + ".npz")), json.load(f)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("hybrid")
    return {"on": _run(tmp, None), "off": _run(tmp, "0")}


@pytest.fixture(scope="module")
def canonical_oracle():
    from oracle import orc
    from conftest import OracleApi
    so = recipe_canonical()(OracleApi(orc))
    k = CANON
    ref, cn = so.render(k["w"], k["h"], orc.canonical_viewport(k["w"], k["h"]), k["depth"], k["spp"], seed=k["seed"], threads=8)
    return so, ref, cn


def _balance(d):
    """every ray offered is refused, missed, tied, confirmed or failed in the descent; the fallbacks are the rest"""
    failed = d[F_ABSENT] + d[F_NOCOLLIDE] + d[F_TMIN] + d[F_NOTRI] + d[F_BOUNDS]
    assert d[OFFERED] == d[REFUSED] + d[MISSES] + d[TIES] + d[CONFIRMED] + failed, d
    assert d[FALLBACKS] == d[REFUSED] + d[TIES] + failed, d
    assert d[F_BOUNDS] == 0, d


@pytest.mark.parametrize("pipe", [3, 1])
def test_frame_parity(runs, canonical_oracle, pipe):
    """Canonical scene, 64 x 64, 4 spp, depth 5: the default frame = the RTMI_HYBRID=0 frame = the oracle's bits, "Rays" equal,
    the counting build's counters the oracle's, no violation, and at most 10 % of the rays offered fall back."""
    _, ref, cn = canonical_oracle
    for counting in (0, 1):
        key = f"canonical_p{pipe}_c{counting}"
        for s in ("on", "off"):
            arrays, res = runs[s]
            assert_bits_equal(ref, arrays[key], f"{key} hybrid {s} vs the oracle")
            assert res[key]["total_rays"] == cn["rays"], (key, s, res[key]["total_rays"], cn["rays"])
            assert res[key]["stats"]["pipeline"] == pipe
            if counting:
                for k in COUNTERS:
                    assert res[key]["stats"][k] == cn[k], (s, k, res[key]["stats"][k], cn[k])
        assert_bits_equal(runs["off"][0][key], runs["on"][0][key], f"{key} hybrid on vs off")
        d, d0 = runs["on"][1][key]["hyb"], runs["off"][1][key]["hyb"]
        print(f"\n{key}: offered {d[OFFERED]}, refused {d[REFUSED]}, BVH misses {d[MISSES]}, ties {d[TIES]}, descents failed "
              f"{d[F_ABSENT]} / {d[F_NOCOLLIDE]} / {d[F_TMIN]}, lists without the hit {d[F_NOTRI]}, confirmed {d[CONFIRMED]}, "
              f"fallbacks {d[FALLBACKS]} ({d[FALLBACKS] / max(d[OFFERED], 1):.4f}), violations {d[VIOLATIONS]}")
        assert runs["on"][1][key]["on"] == 1 and runs["off"][1][key]["on"] == 0
        assert d0 == [0] * 12, "RTMI_HYBRID=0 still runs hybrid passes"
        _balance(d)
        assert d[VIOLATIONS] == 0
        # pipeline 1 offers every ray of the frame, pipeline 3 the bounce rays
        assert d[OFFERED] > 1000 and (pipe == 3 or d[OFFERED] >= 0.99 * cn["rays"])
        assert d[FALLBACKS] <= 0.10 * d[OFFERED], "the hybrid falls back for more than 10 % of its rays"


def _vs_oracle(so, arrays, name, o4, d4):
    tri, t, face, cn = so.trace(o4, d4)
    bad = np.nonzero(arrays[name + "_tri"] != tri)[0]
    assert len(bad) == 0, f"{name}: {len(bad)} hit ids differ, first ray {bad[:5]}: {arrays[name + '_tri'][bad[:5]]} vs {tri[bad[:5]]}"
    hit = tri != 0
    assert_bits_equal(t[hit], arrays[name + "_t"][hit], f"{name}: t")
    assert np.array_equal(face[hit], arrays[name + "_face"][hit]), f"{name}: face"
    return tri, cn


def _oracle(recipe):
    from oracle import orc
    from conftest import OracleApi
    return recipe(OracleApi(orc))


def test_refused_rays_take_the_fallback(runs):
    """NaN, inf, zero components, a nonzero lane 3 and rays exactly parallel to a triangle's plane: every one is refused, walked
    exactly, and equals the oracle -- on the axis-aligned scene of test_trace_edge_case_rays and on the hand-made one."""
    for name, recipe, parallel in (("axis_refused", recipe_axis_box(), False), ("big_refused", recipe_big(), True)):
        o4, d4 = refused_rays(parallel)
        so = _oracle(recipe)
        for s in ("on", "off"):
            _vs_oracle(so, runs[s][0], name, o4, d4)
        r = runs["on"][1][name]
        assert r["on"] == 1, f"{name}: the scene has no hybrid passes"
        d = r["hyb"]
        assert d[OFFERED] == len(o4) and d[REFUSED] == len(o4) and d[FALLBACKS] == len(o4), d
        assert r["stats"]["rays"] == len(o4)


def test_far_origins_are_refused_and_equal_the_oracle(runs, canonical_oracle):
    """rtmi_trace with origins up to 10^6 away from the canonical scene: every ray beyond the origin bound is refused and walked
    exactly, some within it are confirmed, all equal the oracle, and the referee of the counting build sees no violation."""
    import test_hybrid_cpu as H
    so, _, _ = canonical_oracle
    o4, d4 = far_rays()
    raw, _, _ = so.triangles()
    beyond = int((np.abs(o4[:, :3]).sum(axis=1, dtype=np.float32) > H.origin_max(raw[1:])).sum())
    assert 0.3 * len(o4) < beyond < 0.8 * len(o4)
    for name in ("far", "far_counting"):
        for s in ("on", "off"):
            tri, cn = _vs_oracle(so, runs[s][0], name, o4, d4)
        assert (tri != 0).sum() > 0.3 * len(o4)
        d = runs["on"][1][name]["hyb"]
        _balance(d)
        assert d[OFFERED] == len(o4) and d[REFUSED] >= beyond and d[CONFIRMED] > 500, (beyond, d)
        assert d[VIOLATIONS] == 0
    for k in COUNTERS + ("rays",):
        assert runs["on"][1]["far_counting"]["stats"][k] == cn[k], k


def test_ties_fall_back_to_the_octree_walks_choice(runs):
    """A triangle stored twice: the BVH reports a tie for every ray that hits it, and the index returned is the one the oracle's
    octree walk returns."""
    o4, d4 = dup_rays()
    so = _oracle(recipe_duplicate())
    assert so.tree_stats()["maxdepth"] >= 2
    for name in ("dup", "dup_counting"):
        for s in ("on", "off"):
            tri, cn = _vs_oracle(so, runs[s][0], name, o4, d4)
        d = runs["on"][1][name]["hyb"]
        ndup = int(np.isin(tri, [25, 26]).sum())
        assert ndup > 250 and d[TIES] >= ndup, (ndup, d)
        _balance(d)
        assert d[VIOLATIONS] == 0
    for k in COUNTERS + ("rays",):
        assert runs["on"][1]["dup_counting"]["stats"][k] == cn[k], k


def test_hit_points_outside_the_octree(runs):
    """A large triangle over a root box that covers only its middle: where the BVH's hit point lies outside the root box the
    descent fails, the ray falls back, and the result is the oracle's."""
    (o4, d4), p = big_rays()
    so = _oracle(recipe_big())
    outside = (np.abs(p) > 1.0).any(axis=1)
    assert outside.sum() > 200
    for name in ("big", "big_counting"):
        for s in ("on", "off"):
            tri, cn = _vs_oracle(so, runs[s][0], name, o4, d4)
        d = runs["on"][1][name]["hyb"]
        _balance(d)
        assert d[VIOLATIONS] == 0
        assert d[F_ABSENT] + d[F_NOCOLLIDE] + d[F_TMIN] + d[F_NOTRI] > 100, d
        assert d[CONFIRMED] > 0
    for k in COUNTERS + ("rays",):
        assert runs["on"][1]["big_counting"]["stats"][k] == cn[k], k


def test_scene_without_direction_table_keeps_its_path(runs):
    """The 8-teapot grid has more than 8 192 distinct normals, hence no direction table and no certificate: no hybrid pass runs,
    and the frame is the RTMI_HYBRID=0 frame and the oracle's."""
    from oracle import orc
    g = GRID
    so = _oracle(recipe_grid())
    raw, _, _ = so.triangles()
    assert len(np.unique(raw[1:, 3:6], axis=0)) > 8192
    vo = orc.create_viewport(g["w"], g["h"], g["size"], g["pos"], orc.unit(g["dir"]), g["fov"], g["roll"])
    ref, cn = so.render(g["w"], g["h"], vo, g["depth"], g["spp"], seed=g["seed"], threads=8)
    for s in ("on", "off"):
        assert_bits_equal(ref, runs[s][0]["grid_p3_c0"], f"grid, hybrid {s}")
        assert runs[s][1]["grid_p3_c0"]["total_rays"] == cn["rays"]
        assert runs[s][1]["grid_p3_c0"]["on"] == 0 and runs[s][1]["grid_p3_c0"]["hyb"] == [0] * 12
