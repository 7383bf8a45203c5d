"""-m gpu: the node cull of k_path_primary's SELECT step (trace_oct.hpp, the W_PRIMARY part of "Node cull"; DESIGN.md 4.1
"Node cull for primary rays").  One fresh process per setting (RTMI_PRIMARY_NODE_CULL unset, = 0: read at scene creation)
renders every case below with the fast and the counting build; the tests compare image bits, "Rays" and the counting
build's counters between the two and with the oracle."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import assert_bits_equal, recipe_canonical
from test_node_cull import HAND

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTERS = ("rays", "box_tests", "tri_tests", "full_tests", "nodes", "leaves")
NDBG = 52
# dbg[38..44] primary rays, dbg[45..51] mirror reflections traced in place: lanes certified, lanes refused, inner boxes first
# visited, boxes missed, SELECT lane-steps and leaf visits inside missed subtrees, violations
PRIM, REFL = 38, 45
CERT, REFUSED, SEEN, MISSED, SEL_IN, LEAF_IN, VIOL = range(7)
AXIS = dict(size=(1.0, 1.0), pos=[2.0, 0.0, 0.0], dir=[0.0, 0.0, 1.0], fov=90.0, roll=0.0, depth=5)
# name -> (scene, w, h, spp, seed, viewport: None = the canonical one)
CASES = {
    "packets": ("canonical", 32, 32, 64, 1, None),   # whole-wave pixel packets, the mirror disks in view
    "shared": ("canonical", 64, 64, 4, 2, None),     # 16 pixels per wave
    "axis_row": ("canonical", 96, 1, 1, 6, AXIS),    # one row on the camera axis: every primary ray goes to the slow path
    "axis_cross": ("canonical", 33, 33, 1, 6, AXIS),  # its centre row and column do, the other pixels do not
    "hand": ("hand", HAND["w"], HAND["h"], HAND["spp"], HAND["seed"], HAND),  # three levels by hand, the camera outside the root box
}


def recipe_three_levels():
    """test_node_cull.recipe_three_levels without the sliver and the triangle in front: 24 small triangles inside the cell
    [0.5, 1]^3 of a root box (centre 0, half 1), so the root's octant 7 is an inner box at depth 1 over one at depth 2 over
    leaves, and nothing else.  Seen from outside the root box, most rays that cross the cube [0, 1]^3 miss what it holds."""
    def r(api):
        s = api.scene()
        rng = np.random.default_rng(3)
        surfs = [api.matte((200, 120, 40), 0.3), api.reflective(0.01, (220, 220, 230), 0.6)]
        for k in range(24):
            c = rng.uniform(0.6, 0.9, 3)
            tri = (c + rng.uniform(-0.08, 0.08, (3, 3))).clip(0.52, 0.98).astype(np.float32)
            api.add_triangle(s, tri, surfs[k % 2], 0.0)
        s.populate_triangle_numbers()
        s.build_bounding_box([0.0, 0.0, 0.0], 1.0, 3, 2)
        return s
    return r


_RUN = r"""
import ctypes as C, json, os, sys
import numpy as np
root, out = sys.argv[1], sys.argv[2]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
from rust_raytrace_amd import raytrace as R, _ffi
from conftest import ProductApi, recipe_canonical
import test_primary_node_cull as T
L = _ffi.lib()
L.rth_debug_counters_n.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
res, arrays = {}, {}
recipes = {"canonical": recipe_canonical(), "hand": T.recipe_three_levels()}
for name, (scene, w, h, spp, seed, v) in T.CASES.items():
    # a scene of its own per case: the step statistics are summed over the control blocks of every stream, and a stream that
    # a smaller frame does not use keeps those of the frame before
    sp = recipes[scene](ProductApi(R))
    if v is None:
        vp = R.canonical_viewport(w, h, 5, spp)
    else:
        vp = R.create_viewport((w, h), v["size"], v["pos"], R.unit(v["dir"]), v["fov"], R.to_radians(v["roll"]), v["depth"], spp)
    for counting in (False, True):
        img = np.zeros((h, w, 4), np.float32)
        c = R.HipRayCaster(seed=seed, options=R.OPT_COUNTERS if counting else 0)
        ctx = c.walk_rays(vp, sp, img, 1, False)
        key = f"{name}_c{int(counting)}"
        arrays[key] = img
        r = {"total_rays": int(ctx.total_rays), "stats": {k: int(x) for k, x in ctx.stats.items() if isinstance(x, (int, np.integer))}}
        if counting:
            d = (C.c_ulonglong * T.NDBG)()
            L.rth_debug_counters_n(sp.h, d, T.NDBG)
            r["dbg"] = [int(x) for x in d]
        res[key] = r
np.savez(out + ".npz", **arrays)
json.dump(res, open(out + ".json", "w"))
"""


def _run(tmp, setting):
    env = dict(os.environ)
    for k in ("RTMI_PRIMARY_NODE_CULL", "RTMI_NODE_CULL", "RTMI_BLOCK_CULL", "RTMI_BLOCK_CULL_N", "RTMI_PACKET_CULL", "RTMI_MIRROR_INPLACE"):
        env.pop(k, None)
    if setting is not None:
        env["RTMI_PRIMARY_NODE_CULL"] = setting
    out = str(tmp / f"pnc_{setting}")
    subprocess.run([sys.executable, "-c", _RUN, ROOT, out], env=env, check=True, timeout=300)
    with open(out + ".json") as f:
        return dict(np.load(out + ".npz")), json.load(f)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("primary_node_cull")
    return {"on": _run(tmp, None), "off": _run(tmp, "0")}


@pytest.fixture(scope="module")
def oracle():
    """name -> (image, counters) of the oracle, rendered once"""
    from oracle import orc
    from conftest import OracleApi
    scenes = {"canonical": recipe_canonical()(OracleApi(orc)), "hand": recipe_three_levels()(OracleApi(orc))}
    out = {}
    for name, (scene, w, h, spp, seed, v) in CASES.items():
        if v is None:
            vo = orc.canonical_viewport(w, h)
        else:
            vo = orc.create_viewport(w, h, v["size"], v["pos"], orc.unit(v["dir"]), v["fov"], orc.to_radians(v["roll"]))
        out[name] = scenes[scene].render(w, h, vo, 5, spp, seed=seed, threads=8)
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_image_and_rays(runs, oracle, name):
    """Fast build: cull on = cull off = the oracle, image bits and "Rays"."""
    ref, cn = oracle[name]
    key = f"{name}_c0"
    for s in ("on", "off"):
        arrays, res = runs[s]
        assert_bits_equal(ref, arrays[key], f"{key} primary node cull {s} vs the oracle")
        assert res[key]["total_rays"] == cn["rays"], (key, s, res[key]["total_rays"], cn["rays"])
        assert res[key]["stats"]["pipeline"] == 3
    assert_bits_equal(runs["off"][0][key], runs["on"][0][key], f"{key} primary node cull on vs off")


@pytest.mark.parametrize("name", list(CASES))
def test_counting_build(runs, oracle, name):
    """The counting build evaluates certificate and node predicate and culls nothing: image and the six work counters are the
    oracle's, no hit was taken inside a missed subtree, and boxes are missed wherever a lane can hold the certificate (on the
    one-row frame every primary ray has a zero direction component: it leaves for the slow path before any lane takes it, so
    there all fourteen counters are 0).  With RTMI_PRIMARY_NODE_CULL=0 the new counters stay 0 and the rest is unchanged."""
    ref, cn = oracle[name]
    key = f"{name}_c1"
    for s in ("on", "off"):
        assert_bits_equal(ref, runs[s][0][key], f"{key} primary node cull {s} vs the oracle")
        for k in COUNTERS:
            assert runs[s][1][key]["stats"][k] == cn[k], (s, k, runs[s][1][key]["stats"][k], cn[k])
    d, d0 = runs["on"][1][key]["dbg"], runs["off"][1][key]["dbg"]
    p, m = d[PRIM:PRIM + 7], d[REFL:REFL + 7]
    print(f"\n{name}: primary rays certified {p[CERT]}, refused {p[REFUSED]}, boxes seen {p[SEEN]}, missed {p[MISSED]}, inside missed "
          f"subtrees SELECT lane-steps {p[SEL_IN]}, leaf visits {p[LEAF_IN]}, violations {p[VIOL]}; reflections in place {m}; "
          f"all SELECT lane-steps {d[1]}, leaf visits {d[12]}")
    assert p[VIOL] == 0 and m[VIOL] == 0, "a hit was taken inside a subtree whose node record the half-line misses"
    assert d0[PRIM:PRIM + 14] == [0] * 14, "RTMI_PRIMARY_NODE_CULL=0 still evaluates the node cull"
    # (the walk itself is the same: SELECT lane-steps, memo statistics and the bounce passes' culls; wave-step and cycle
    # counts depend on which lanes happen to share a step)
    assert d[1] == d0[1] and d[12:16] == d0[12:16] and d[26:PRIM] == d0[26:PRIM], "the walk's statistics depend on the setting"
    scene, w, h, spp, seed, v = CASES[name]
    slow = runs["on"][1][key]["stats"]["slow_paths"]
    if name == "axis_row":
        assert slow >= w * h and p == [0] * 7 and m[CERT] + m[REFUSED] == 0
        return
    # (every primary ray a lane takes is counted once; those that left for the slow path are not taken)
    assert w * h * spp - slow <= p[CERT] + p[REFUSED] <= w * h * spp
    assert p[MISSED] > 0 and p[SEL_IN] > 0 and p[SEEN] >= p[MISSED]
    if name == "axis_cross":
        assert slow >= w + h - 1, "the centre row and column did not take the slow path"
    if name == "packets":
        assert p[REFUSED] < 0.02 * (p[CERT] + p[REFUSED]), "more than 2 % of the primary lanes refused"
        assert m[CERT] > 0 and m[MISSED] > 0, "no mirror reflection traced in place held the certificate"
