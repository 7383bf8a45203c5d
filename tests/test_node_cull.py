"""-m gpu: the node cull of k_trace_oct's SELECT step (trace_oct.hpp, "Node cull").  One fresh process per
setting (RTMI_NODE_CULL unset, = 0: read at scene creation) renders and traces everything below; the tests compare image
bits, "Rays", the counting build's counters and the traced hits between the two and with the oracle."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import assert_bits_equal, recipe_canonical

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
COUNTERS = ("box_tests", "tri_tests", "full_tests", "nodes", "leaves")
CANON = dict(w=64, h=64, spp=4, depth=5, seed=1)
GRID = dict(w=32, h=32, spp=4, depth=5, seed=7, size=(1.0, 1.0), pos=[0.0, 0.0, -2.0], dir=[0.0, 0.0, 1.0], fov=16.0, roll=0.0)
HAND = dict(w=32, h=32, spp=2, depth=5, seed=3, size=(1.0, 1.0), pos=[0.3, 0.0, -3.0], dir=[0.0, 0.0, 1.0], fov=40.0, roll=0.0)
NDBG = 38
# dbg[33..37]: nodes seen, nodes missed, SELECT lane-steps and leaf visits inside a missed subtree, violations
SEEN, MISSED, SEL_IN, LEAF_IN, VIOL = 33, 34, 35, 36, 37


def recipe_three_levels():
    """Three levels by hand, in the manner of test_leaf_list_cull.recipe_cluster: 24 small triangles inside the cell
    [0.5, 1]^3 of a root box (centre 0, half 1), so the root's octant 7 is an inner box at depth 1 over one at depth 2 over
    leaves; a sliver that starts inside that cell and ends at (-0.1, -0.1, 0.7) makes one list below the depth-1 box reach
    far outside it; a Matte triangle at z = -0.5 in front, whose bounce rays leave towards the camera with the depth-1 box
    behind them."""
    def r(api):
        s = api.scene()
        rng = np.random.default_rng(3)
        surfs = [api.matte((200, 120, 40), 0.3), api.reflective(0.01, (220, 220, 230), 0.6)]
        for k in range(24):
            c = rng.uniform(0.6, 0.9, 3)
            tri = (c + rng.uniform(-0.08, 0.08, (3, 3))).clip(0.52, 0.98).astype(np.float32)
            api.add_triangle(s, tri, surfs[k % 2], 0.0)
        api.add_triangle(s, np.array([[0.6, 0.6, 0.7], [0.66, 0.6, 0.7], [-0.1, -0.1, 0.7]], np.float32), api.matte((40, 200, 90), 0.4), 0.0)
        api.add_triangle(s, np.array([[-0.98, -0.98, -0.5], [0.98, -0.98, -0.5], [0.0, 0.98, -0.5]], np.float32),
                         api.matte((90, 90, 200), 0.5), 0.0)
        s.populate_triangle_numbers()
        s.build_bounding_box([0.0, 0.0, 0.0], 1.0, 3, 2)
        return s
    return r


def trace_rays():
    """test_ray_cert.trace_rays() plus 64 rays: 48 that start at the incenters of the 12 recorded triangles of the canonical
    scene (tests/golden/canonical_triangle_records.npz) and point away from the teapot, and 16 that start beyond the root
    box (centre (0, 0, 20.1), half 20) and point away from it, so that the root itself is culled."""
    import test_ray_cert as T
    o4, d4 = T.trace_rays()
    z = np.load(os.path.join(GOLDEN, "canonical_triangle_records.npz"))
    rec = z["rec"].astype(np.float64)
    rng = np.random.default_rng(43)
    eo, ed = [], []
    for r in rec:
        away = r[0:3] - np.array([0.0, 0.5, 5.0])
        away /= np.linalg.norm(away)
        for k in range(4):
            d = away + rng.normal(size=3) * 0.2
            eo.append(r[0:3]); ed.append(d / np.linalg.norm(d))
    for k in range(16):
        u = rng.normal(size=3)
        u /= np.linalg.norm(u)
        d = u + rng.normal(size=3) * 0.1
        eo.append(np.array([0.0, 0.0, 20.1]) + u * 50.0); ed.append(d / np.linalg.norm(d))
    xo, xd = np.zeros((len(eo), 4), np.float32), np.zeros((len(eo), 4), np.float32)
    xo[:, :3], xd[:, :3] = np.array(eo), np.array(ed)
    return np.concatenate([o4, xo]), np.concatenate([d4, xd])


_RUN = r"""
import ctypes as C, json, os, sys
import numpy as np
import torch
root, out = sys.argv[1], sys.argv[2]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
from rust_raytrace_amd import raytrace as R, _ffi
from conftest import ProductApi, recipe_canonical, recipe_grid
import test_node_cull as T
L = _ffi.lib()
L.rth_debug_counters_n.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
L.rth_debug_node_cull_stats.argtypes = [C.c_void_p, C.c_void_p]
res, arrays = {}, {}

def render(name, sp, vp, w, h, seed, pipe, counting):
    img = np.zeros((h, w, 4), np.float32)
    c = R.HipRayCaster(seed=seed, options=R.OPT_COUNTERS if counting else 0, tuning={"pipeline": pipe})
    ctx = c.walk_rays(vp, sp, img, 1, False)
    key = f"{name}_p{pipe}_c{int(counting)}"
    arrays[key] = img
    r = {"total_rays": int(ctx.total_rays), "stats": {k: int(v) for k, v in ctx.stats.items() if isinstance(v, (int, np.integer))}}
    if counting:
        d = (C.c_ulonglong * T.NDBG)()
        L.rth_debug_counters_n(sp.h, d, T.NDBG)
        r["dbg"] = [int(x) for x in d]
    st = (C.c_ulonglong * 3)()
    L.rth_debug_node_cull_stats(sp.h, st)
    r["node_records"] = int(st[0])
    res[key] = r

sp = recipe_canonical()(ProductApi(R))
k = T.CANON
for pipe in (3, 1):
    for counting in (False, True):
        render("canonical", sp, R.canonical_viewport(k["w"], k["h"], k["depth"], k["spp"]), k["w"], k["h"], k["seed"], pipe, counting)
o4, d4 = T.trace_rays()
n = len(o4)
to, td = torch.from_numpy(o4).cuda(), torch.from_numpy(d4).cuda()
tri, face = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")
t = torch.zeros(n, device="cuda")
R.HipRayCaster().trace_device(sp, to, td, tri, t, face)
torch.cuda.synchronize()
arrays["trace_tri"], arrays["trace_t"], arrays["trace_face"] = tri.cpu().numpy(), t.cpu().numpy(), face.cpu().numpy()
for name, g, sc in (("grid", T.GRID, recipe_grid()(ProductApi(R))), ("hand", T.HAND, T.recipe_three_levels()(ProductApi(R)))):
    vg = R.create_viewport((g["w"], g["h"]), g["size"], g["pos"], R.unit(g["dir"]), g["fov"], g["roll"], g["depth"], g["spp"])
    for counting in (False, True):
        render(name, sc, vg, g["w"], g["h"], g["seed"], 3, counting)
np.savez(out + ".npz", **arrays)
json.dump(res, open(out + ".json", "w"))
"""


def _run(tmp, setting):
    env = dict(os.environ)
    for k in ("RTMI_NODE_CULL", "RTMI_BLOCK_CULL", "RTMI_BLOCK_CULL_N"):
        env.pop(k, None)
    if setting is not None:
        env["RTMI_NODE_CULL"] = setting
    out = str(tmp / f"nc_{setting}")
    subprocess.run([sys.executable, "-c", _RUN, ROOT, out], env=env, check=True, timeout=300)
    with open(out + ".json") as f:
        return dict(np.load(out + ".npz")), json.load(f)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("node_cull")
    return {"on": _run(tmp, None), "off": _run(tmp, "0")}


@pytest.fixture(scope="module")
def canonical_oracle():
    from oracle import orc
    from conftest import OracleApi
    so = recipe_canonical()(OracleApi(orc))
    k = CANON
    ref, cn = so.render(k["w"], k["h"], orc.canonical_viewport(k["w"], k["h"]), k["depth"], k["spp"], seed=k["seed"], threads=8)
    return so, ref, cn


@pytest.mark.parametrize("pipe", [3, 1])
def test_canonical_image_and_rays(runs, canonical_oracle, pipe):
    """Image bits and "Rays": cull on = cull off = the oracle, with the path kernel (3) and one k_trace_oct per pass (1)."""
    _, ref, cn = canonical_oracle
    key = f"canonical_p{pipe}_c0"
    for s in ("on", "off"):
        arrays, res = runs[s]
        assert_bits_equal(ref, arrays[key], f"{key} node cull {s} vs the oracle")
        assert res[key]["total_rays"] == cn["rays"], (key, s, res[key]["total_rays"], cn["rays"])
        assert res[key]["stats"]["pipeline"] == pipe
    assert_bits_equal(runs["off"][0][key], runs["on"][0][key], f"{key} node cull on vs off")
    assert runs["on"][1][key]["node_records"] > 0 and runs["off"][1][key]["node_records"] == 0


@pytest.mark.parametrize("pipe", [3, 1])
def test_canonical_counting_build(runs, canonical_oracle, pipe):
    """The counting build evaluates the node predicate and culls nothing: image and the five counters are the oracle's, no
    hit was taken inside a missed subtree, and some nodes are missed.  With RTMI_NODE_CULL=0 the new counters stay 0."""
    _, ref, cn = canonical_oracle
    key = f"canonical_p{pipe}_c1"
    for s in ("on", "off"):
        assert_bits_equal(ref, runs[s][0][key], f"{key} node cull {s} vs the oracle")
        for k in COUNTERS:
            assert runs[s][1][key]["stats"][k] == cn[k], (s, k, runs[s][1][key]["stats"][k], cn[k])
    d, d0 = runs["on"][1][key]["dbg"], runs["off"][1][key]["dbg"]
    print(f"\npipeline {pipe}: nodes seen {d[SEEN]}, missed {d[MISSED]} ({d[MISSED] / max(d[SEEN], 1):.3f}), inside missed "
          f"subtrees: SELECT lane-steps {d[SEL_IN]} of {d[1]}, leaf visits {d[LEAF_IN]} of {d[12]}; violations {d[VIOL]}")
    assert d[VIOL] == 0, "a hit was taken inside a subtree whose node record the half-line misses"
    assert d[SEEN] > 0 and d[MISSED] > 0 and d[SEL_IN] > 0
    assert d0[33:38] == [0] * 5, "RTMI_NODE_CULL=0 still evaluates the node cull"
    assert d[12:16] == d0[12:16] and d[26:33] == d0[26:33]  # (the walk itself is the same: memo and block-cull statistics)


def test_trace_device_on_equals_off_and_oracle(runs, canonical_oracle):
    """rtmi_trace_device on the explicit ray set: the same hit index, t bits and face, on = off = the oracle; the rays that
    start beyond the root box and point away hit nothing."""
    on, off = runs["on"][0], runs["off"][0]
    assert np.array_equal(on["trace_tri"], off["trace_tri"])
    assert np.array_equal(on["trace_face"], off["trace_face"])
    assert_bits_equal(off["trace_t"], on["trace_t"], "t, node cull on vs off")
    so, _, _ = canonical_oracle
    o4, d4 = trace_rays()
    tri, t, face, _ = so.trace(o4, d4)
    assert np.array_equal(on["trace_tri"].view(np.uint32), tri)
    hit = tri != 0
    assert not hit[-16:].any()
    assert_bits_equal(t[hit], on["trace_t"][hit], "t vs the oracle")
    assert np.array_equal(on["trace_face"].view(np.uint32)[hit], face[hit])


def test_grid_scene_has_no_records_and_on_equals_off(runs):
    """The 8-teapot grid keeps the 32-B block records (no direction table), so it gets no node records: on = off, counters
    and step statistics of the cull included."""
    for counting in (0, 1):
        key = f"grid_p3_c{counting}"
        assert_bits_equal(runs["off"][0][key], runs["on"][0][key], key)
        assert runs["on"][1][key]["total_rays"] == runs["off"][1][key]["total_rays"]
        assert runs["on"][1][key]["node_records"] == 0
    for k in COUNTERS:
        assert runs["on"][1]["grid_p3_c1"]["stats"][k] == runs["off"][1]["grid_p3_c1"]["stats"][k], k
    d, d0 = runs["on"][1]["grid_p3_c1"]["dbg"], runs["off"][1]["grid_p3_c1"]["dbg"]
    assert d[26:38] == d0[26:38] and d[33:38] == [0] * 5


def test_three_level_scene(runs):
    """The hand-made scene at 32 x 32, 2 spp: on = off = the oracle; bounce rays meet missed nodes (that the depth-1 box is
    among them is checked on the host in test_node_cull_cpu.py)."""
    from oracle import orc
    from conftest import OracleApi
    g = HAND
    so = recipe_three_levels()(OracleApi(orc))
    vo = orc.create_viewport(g["w"], g["h"], g["size"], g["pos"], orc.unit(g["dir"]), g["fov"], g["roll"])
    ref, cn = so.render(g["w"], g["h"], vo, g["depth"], g["spp"], seed=g["seed"], threads=8)
    assert cn["rays"] > g["w"] * g["h"] * g["spp"], "no bounce rays in the hand-made scene"
    for s in ("on", "off"):
        for counting in (0, 1):
            key = f"hand_p3_c{counting}"
            assert_bits_equal(ref, runs[s][0][key], f"{key} node cull {s} vs the oracle")
            assert runs[s][1][key]["total_rays"] == cn["rays"]
        for k in COUNTERS:
            assert runs[s][1]["hand_p3_c1"]["stats"][k] == cn[k], (s, k)
    d = runs["on"][1]["hand_p3_c1"]["dbg"]
    assert runs["on"][1]["hand_p3_c1"]["node_records"] == 3
    assert d[VIOL] == 0 and d[MISSED] > 0
    assert runs["off"][1]["hand_p3_c1"]["dbg"][33:38] == [0] * 5
