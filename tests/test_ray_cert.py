"""-m gpu: the per-ray sign certificate and the packed box-only cull records of k_trace_oct (trace_oct.hpp, DESIGN.md 4.1
"Sign certificate per ray").  One fresh process per setting (RTMI_BLOCK_CULL unset, = 0: read at scene creation) renders and
traces everything below; the tests compare image bits, "Rays", the counting build's counters and the traced hits between
the two and with the oracle."""
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
NDBG = 33


def trace_rays():
    """The rays of test_block_cull.trace_rays (random rays and its 96 edge rays: nonzero lane 3, a zero direction component,
    far origins) and, for 12 triangles of the canonical scene (tests/golden/canonical_triangle_records.npz): rays perpendicular
    to the triangle's normal -- as computed in double, and with one component moved by up to 2 ulp -- that pass through the
    triangle's incenter sphere, and rays that start at the incenter, inside the box of every block that lists the triangle."""
    import test_block_cull as T
    o4, d4 = T.trace_rays()
    z = np.load(os.path.join(GOLDEN, "canonical_triangle_records.npz"))
    rec = z["rec"].astype(np.float64)
    rng = np.random.default_rng(41)
    eo, ed = [], []
    for r in rec:
        c, n, rho = r[0:3], r[3:6] / np.linalg.norm(r[3:6]), np.sqrt(r[6])
        for k in range(8):
            d = np.cross(n, rng.normal(size=3))
            d = (d / np.linalg.norm(d)).astype(np.float32)
            j = int(rng.integers(0, 3))
            for _ in range(k % 3):
                d[j] = np.nextafter(d[j], np.float32(np.inf if k & 4 else -np.inf))
            o = c + n * rho * rng.uniform(-0.9, 0.9) - d.astype(np.float64) * rng.uniform(0.5, 4.0)
            eo.append(o); ed.append(d)
        for k in range(4):
            d = rng.normal(size=3)
            eo.append(c); ed.append(d / np.linalg.norm(d))
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
import test_ray_cert as T
L = _ffi.lib()
L.rth_debug_counters_n.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
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
g = T.GRID
sg = recipe_grid()(ProductApi(R))
vg = R.create_viewport((g["w"], g["h"]), g["size"], g["pos"], R.unit(g["dir"]), g["fov"], g["roll"], g["depth"], g["spp"])
for counting in (False, True):
    render("grid", sg, vg, g["w"], g["h"], g["seed"], 3, counting)
np.savez(out + ".npz", **arrays)
json.dump(res, open(out + ".json", "w"))
"""


def _run(tmp, setting):
    env = dict(os.environ)
    env.pop("RTMI_BLOCK_CULL", None)
    env.pop("RTMI_BLOCK_CULL_N", None)
    if setting is not None:
        env["RTMI_BLOCK_CULL"] = setting
    out = str(tmp / f"rc_{setting}")
    subprocess.run([sys.executable, "-c", _RUN, ROOT, out], env=env, check=True, timeout=300)
    with open(out + ".json") as f:
        return dict(np.load(out + ".npz")), json.load(f)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("ray_cert")
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
        assert_bits_equal(ref, arrays[key], f"{key} cull {s} vs the oracle")
        assert res[key]["total_rays"] == cn["rays"], (key, s, res[key]["total_rays"], cn["rays"])
        assert res[key]["stats"]["pipeline"] == pipe
    assert_bits_equal(runs["off"][0][key], runs["on"][0][key], f"{key} cull on vs off")


@pytest.mark.parametrize("pipe", [3, 1])
def test_canonical_counting_build(runs, canonical_oracle, pipe):
    """The counting build evaluates the certificate and the packed predicate and still tests every reference: image and
    counters are the oracle's, no culled block held a passing reference, at least half of the blocks seen are culled and
    the certificate refuses fewer than 5 % of the rays."""
    _, ref, cn = canonical_oracle
    key = f"canonical_p{pipe}_c1"
    for s in ("on", "off"):
        assert_bits_equal(ref, runs[s][0][key], f"{key} cull {s} vs the oracle")
        for k in COUNTERS:
            assert runs[s][1][key]["stats"][k] == cn[k], (s, k, runs[s][1][key]["stats"][k], cn[k])
    d, d0 = runs["on"][1][key]["dbg"], runs["off"][1][key]["dbg"]
    print(f"\npipeline {pipe}: blocks seen {d[26]}, culled {d[28]} ({d[28] / max(d[26], 1):.3f}), lists ended by a culled block "
          f"{d[29]}, violations {d[30]}; rays {d[31]}, refused {d[32]} ({d[32] / max(d[31], 1):.4f})")
    assert d[30] == 0, "a culled block held a reference whose exact test passed"
    assert d[26] > 0 and d[28] >= 0.5 * d[26]
    assert d[31] > 0 and d[32] < 0.05 * d[31]
    assert d0[26:33] == [0] * 7, "RTMI_BLOCK_CULL=0 still evaluates the cull"


def test_grid_scene_on_equals_off(runs):
    """The 8-teapot grid (FN_WIDE boxes; each teapot is rotated, so the scene has eight times the normals and, above
    RTMI_CERT_MAX_NORMALS, keeps the 32-B records): on = off, counters included."""
    for counting in (0, 1):
        key = f"grid_p3_c{counting}"
        assert_bits_equal(runs["off"][0][key], runs["on"][0][key], key)
        assert runs["on"][1][key]["total_rays"] == runs["off"][1][key]["total_rays"]
    for k in COUNTERS:
        assert runs["on"][1]["grid_p3_c1"]["stats"][k] == runs["off"][1]["grid_p3_c1"]["stats"][k], k
    d = runs["on"][1]["grid_p3_c1"]["dbg"]
    assert d[30] == 0 and d[28] > 0


def test_trace_device_on_equals_off_and_oracle(runs, canonical_oracle):
    """rtmi_trace_device on the explicit ray set: the same hit index, t bits and face, on = off = the oracle."""
    on, off = runs["on"][0], runs["off"][0]
    assert np.array_equal(on["trace_tri"], off["trace_tri"])
    assert np.array_equal(on["trace_face"], off["trace_face"])
    assert_bits_equal(off["trace_t"], on["trace_t"], "t, cull on vs off")
    so, _, _ = canonical_oracle
    o4, d4 = trace_rays()
    tri, t, face, _ = so.trace(o4, d4)
    assert np.array_equal(on["trace_tri"].view(np.uint32), tri)
    hit = tri != 0
    assert hit[-144:].sum() > 20, "the perpendicular and inside rays hit nothing"
    assert_bits_equal(t[hit], on["trace_t"][hit], "t vs the oracle")
    assert np.array_equal(on["trace_face"].view(np.uint32)[hit], face[hit])
