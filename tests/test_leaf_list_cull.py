"""-m gpu: the whole-list packet cull of k_path_primary's LEAF step (trace_oct.hpp, DESIGN.md 4.1 "Packet cull").  Every case
renders in fresh processes with the packet cull on and off (RTMI_PACKET_CULL), uncounted and counted, and compares image
bits, "Rays" and the counting build's six work counters with each other and with the oracle."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import assert_bits_equal, recipe_canonical, recipe_grid

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTERS = ("rays", "box_tests", "tri_tests", "full_tests", "nodes", "leaves")


def recipe_cluster(n):
    """n small triangles inside one cell of a depth-2 octree (root centre 0, half 1: the cell [0.5, 1]^3), so that one leaf
    list holds exactly n references, seen head-on by the camera; a Matte triangle at z = -0.5 lies off to the side of the
    camera's view of the cluster (at y = 0.75 it spans |x| <= 0.12) for bounce rays to hit."""
    def r(api):
        s = api.scene()
        rng = np.random.default_rng(n)
        surfs = [api.matte((200, 120, 40), 0.3), api.reflective(0.01, (220, 220, 230), 0.6)]
        for k in range(n):
            c = rng.uniform(0.6, 0.9, 3)
            tri = (c + rng.uniform(-0.08, 0.08, (3, 3))).clip(0.52, 0.98).astype(np.float32)
            api.add_triangle(s, tri, surfs[k % 2], 0.0)
        api.add_triangle(s, np.array([[-0.98, -0.98, -0.5], [0.98, -0.98, -0.5], [0.0, 0.98, -0.5]], np.float32),
                         api.matte((90, 90, 200), 0.5), 0.0)
        s.populate_triangle_numbers()
        s.build_bounding_box([0.0, 0.0, 0.0], 1.0, 2, 1)
        return s
    return r


SCENES = {"canonical": recipe_canonical(), "shallow": recipe_canonical(maxdepth=3, minobjs=19),
          "cluster64": recipe_cluster(64), "cluster65": recipe_cluster(65), "grid": recipe_grid()}

_RENDER = r"""
import ctypes as C, json, os, sys
import numpy as np
root, spec, out = sys.argv[1], json.loads(sys.argv[2]), sys.argv[3]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
from rust_raytrace_amd import raytrace as R, _ffi
from conftest import ProductApi
from test_leaf_list_cull import SCENES
sp = SCENES[spec["scene"]](ProductApi(R))
w, h = spec["w"], spec["h"]
vp = R.create_viewport((w, h), spec["size"], spec["pos"], R.unit(spec["dir"]), spec["fov"], spec["roll"], spec["maxdepth"], spec["spp"])
img = np.zeros((h, w, 4), np.float32)
counting = spec["counting"]
c = R.HipRayCaster(seed=spec["seed"], options=R.OPT_COUNTERS) if counting else R.HipRayCaster(seed=spec["seed"])
ctx = c.walk_rays(vp, sp, img, 1, False)
np.save(out + ".npy", img)
res = {"total_rays": int(ctx.total_rays), "stats": {k: int(v) for k, v in ctx.stats.items() if isinstance(v, (int, np.integer))}}
if counting:
    L = _ffi.lib()
    L.rth_debug_counters_n.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    d = (C.c_ulonglong * 26)()
    L.rth_debug_counters_n(sp.h, d, 26)
    res["dbg"] = [int(x) for x in d]
json.dump(res, open(out + ".json", "w"))
"""


def _render(tmp_path, spec, cull, counting, inplace=None):
    env = dict(os.environ, RTMI_PACKET_CULL="1" if cull else "0")
    env.pop("RTMI_MIRROR_INPLACE", None)
    if inplace is not None:
        env["RTMI_MIRROR_INPLACE"] = str(inplace)
    out = str(tmp_path / f"{spec['scene']}_{spec['w']}_{spec['spp']}_{int(cull)}_{int(counting)}_{inplace}")
    subprocess.run([sys.executable, "-c", _RENDER, ROOT, json.dumps(dict(spec, counting=counting)), out], env=env, check=True,
                   timeout=600)
    with open(out + ".json") as f:
        return np.load(out + ".npy"), json.load(f)


def _oracle(spec):
    from oracle import orc
    so = SCENES[spec["scene"]](__import__("conftest").OracleApi(orc))
    vo = orc.create_viewport(spec["w"], spec["h"], spec["size"], spec["pos"], orc.unit(spec["dir"]), spec["fov"], spec["roll"])
    return so.render(spec["w"], spec["h"], vo, spec["maxdepth"], spec["spp"], seed=spec["seed"], threads=8)


def _check(tmp_path, spec, inplace=None):
    """Cull on / off, uncounted and counted, against the oracle.  Returns the counting build's dbg[] with the cull on."""
    ref, cn = _oracle(spec)
    res = {}
    for cull in (True, False):
        for counting in (False, True):
            img, r = _render(tmp_path, spec, cull, counting, inplace)
            assert_bits_equal(ref, img, f"cull {cull} counting {counting} vs oracle")
            assert r["total_rays"] == cn["rays"], (cull, counting, r["total_rays"], cn["rays"])
            if counting:
                for k in COUNTERS:
                    assert r["stats"][k] == cn[k], (cull, k, r["stats"][k], cn[k])
            res[(cull, counting)] = r
    d = res[(True, True)]["dbg"]
    assert res[(True, False)]["stats"].get("slow_paths") == res[(False, False)]["stats"].get("slow_paths")
    print(f"\n{spec['scene']} {spec['w']}x{spec['h']} spp {spec['spp']} mirror-in-place {inplace}: whole-list culls {d[25]}, "
          f"packet leaf visits {d[24]}, packet block steps {d[16]} of {d[17]}, references culled {d[19]} of {d[18]}, "
          f"violations {d[20]}, slow paths {res[(True, False)]['stats'].get('slow_paths')}")
    assert d[20] == 0, "a reference the list mask culled passed its exact test"
    assert res[(False, True)]["dbg"][25] == 0 and res[(False, True)]["dbg"][24] == 0
    return d


def _spec(**kw):
    # (the packet culls when a pixel's directions spread by at most 1/64: narrow views)
    s = {"scene": "canonical", "w": 48, "h": 48, "size": (1.0, 1.0), "pos": [0.0, 0.5, 0.0], "dir": [0.0, 0.0, 1.0], "fov": 20.0,
         "roll": 0.0, "maxdepth": 5, "spp": 64, "seed": 7}
    s.update(kw)
    return s


@pytest.mark.parametrize("inplace", [None, 0])
def test_canonical(tmp_path, inplace):
    """The canonical scene at the default mirror-in-place threshold and with mirror paths in place off."""
    d = _check(tmp_path, _spec(), inplace)
    assert d[24] > 0 and d[25] >= d[24] and d[19] > 0


def test_shallow_tree_long_lists(tmp_path):
    """A shallow octree: leaf lists longer than 16 blocks, so the whole-list step goes on at block lb0 + 16."""
    d = _check(tmp_path, _spec(scene="shallow"))
    assert d[24] > 0 and d[25] > d[24], "no list continued past 16 blocks"


@pytest.mark.parametrize("n", [64, 65])
def test_list_of_64_and_65_references(tmp_path, n):
    """One leaf list of exactly 64 references (16 full blocks: it ends in range) and of 65 (a 17th block follows)."""
    d = _check(tmp_path, _spec(scene=f"cluster{n}", w=16, h=16, pos=[0.75, 0.75, -3.0], fov=8.0))
    assert d[24] > 0
    if n == 65:
        assert d[25] > d[24]


def test_packet_off_below_64_spp(tmp_path):
    """spp < 64: a wave's lanes hold several pixels, the packet is off and only full LEAF steps run."""
    d = _check(tmp_path, _spec(w=64, h=64, spp=16))
    assert d[25] == 0 and d[16] == 0


def test_slow_path_rays(tmp_path):
    """1 spp in a view so narrow (0.5 degrees over 65 pixels) that the 64 pixels of a wave still make one packet, the camera
    axis through the centre pixel, no roll: the centre column's and row's rays have an exactly-zero direction component
    (129 of them), go to the slow path and leave their lanes idle during the packet steps of their waves."""
    from oracle import orc
    spec = _spec(w=65, h=65, spp=1, fov=0.5)
    vo = orc.create_viewport(65, 65, spec["size"], spec["pos"], orc.unit(spec["dir"]), spec["fov"], spec["roll"])
    _, d4 = orc.primary_rays(65, 65, vo, 1, seed=spec["seed"])
    nzero = int(((d4[:, :3] == 0).any(axis=1)).sum())
    assert nzero > 0
    _img, r = _render(tmp_path, spec, True, False)
    assert r["stats"]["slow_paths"] >= nzero, (r["stats"]["slow_paths"], nzero)
    d = _check(tmp_path, spec)
    assert d[25] > 0


def test_grid_scene_small(tmp_path):
    """The 8-teapot grid of config 5 at a small size."""
    d = _check(tmp_path, _spec(scene="grid", w=32, h=32, pos=[0.0, 0.0, -2.0], fov=16.0))
    assert d[24] > 0
