"""-m gpu: k_path_primary traces the mirror reflections of its primary rays in place (RTMI_MIRROR_INPLACE).
Every case renders in fresh processes with the feature off (RTMI_MIRROR_INPLACE=0), at the default threshold and at other
thresholds, and compares image bits, "Rays" and the counting build's six work counters with each other and with the oracle."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ProductApi, assert_bits_equal, recipe_canonical

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTERS = ("rays", "box_tests", "tri_tests", "full_tests", "nodes", "leaves")


def recipe_mirrors():
    """Two flat mirrors without scattering at 45 degrees to the z axis, with a Matte floor behind them: a camera looking
    along +z sees the first one, its reflections go along +x to the second one, and those reflections go back along -z.
    With a tiny camera roll, primary directions with a tiny but nonzero x component reflect into directions with a
    component that is a rounding-level cancellation of the sums of reflect_ray."""
    def r(api):
        s = api.scene()
        m1 = api.reflective(0.0, (230, 230, 230), 0.7)
        m2 = api.reflective(0.0, (200, 230, 200), 0.6)
        floor = api.matte((200, 200, 200), 0.5)
        quads = [([-2, -3, 3], [3, -3, 8], [3, 3, 8], [-2, 3, 3], m1),      # x = z - 5
                 ([7, -3, 3], [2, -3, 8], [2, 3, 8], [7, 3, 3], m2),        # x = 10 - z
                 ([-3, -3, 0], [8, -3, 0], [8, -3, 9], [-3, -3, 9], floor)]  # y = -3
        for a, b, c, d, surf in quads:
            api.add_triangle(s, np.array([a, b, c], np.float32), surf, 0.0)
            api.add_triangle(s, np.array([a, c, d], np.float32), surf, 0.0)
        s.populate_triangle_numbers()
        s.build_bounding_box([2.5, 0.0, 4.5], 6.0, 4, 1)
        return s
    return r


SCENES = {"canonical": recipe_canonical(), "mirrors": recipe_mirrors()}

_RENDER = r"""
import ctypes as C, json, os, sys
import numpy as np
root, spec, out = sys.argv[1], json.loads(sys.argv[2]), sys.argv[3]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
from rust_raytrace_amd import raytrace as R, _ffi
from conftest import ProductApi
from test_mirror_inplace import SCENES
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
    d = (C.c_ulonglong * 24)()
    L.rth_debug_counters_n(sp.h, d, 24)
    res["dbg"] = [int(x) for x in d]
json.dump(res, open(out + ".json", "w"))
"""


def _render(tmp_path, spec, inplace, counting):
    """One render in a fresh process; inplace None: the library's default threshold."""
    env = dict(os.environ)
    env.pop("RTMI_MIRROR_INPLACE", None)
    if inplace is not None:
        env["RTMI_MIRROR_INPLACE"] = str(inplace)
    out = str(tmp_path / f"{spec['scene']}_{spec['w']}_{spec['maxdepth']}_{spec['spp']}_{inplace}_{int(counting)}")
    subprocess.run([sys.executable, "-c", _RENDER, ROOT, json.dumps(dict(spec, counting=counting)), out], env=env, check=True,
                   timeout=600)
    with open(out + ".json") as f:
        return np.load(out + ".npy"), json.load(f)


def _oracle(spec):
    from oracle import orc
    so = SCENES[spec["scene"]](__import__("conftest").OracleApi(orc))
    vo = orc.create_viewport(spec["w"], spec["h"], spec["size"], spec["pos"], orc.unit(spec["dir"]), spec["fov"], spec["roll"])
    return so.render(spec["w"], spec["h"], vo, spec["maxdepth"], spec["spp"], seed=spec["seed"], threads=8)


def _check(tmp_path, spec, thresholds=(None,)):
    """Off vs each threshold, uncounted and counted, and the oracle.  Returns the counting build's dbg[] of the default."""
    ref, cn = _oracle(spec)
    base, base_c = _render(tmp_path, spec, 0, False)
    assert_bits_equal(ref, base, "feature off vs oracle")
    assert base_c["total_rays"] == cn["rays"]
    off_img, off = _render(tmp_path, spec, 0, True)
    assert_bits_equal(ref, off_img, "counting build, feature off vs oracle")
    for k in COUNTERS:
        assert off["stats"][k] == cn[k], ("off", k, off["stats"][k], cn[k])
    dbg = None
    for th in thresholds:
        img, r = _render(tmp_path, spec, th, False)
        assert_bits_equal(base, img, f"threshold {th} vs off")
        assert r["total_rays"] == base_c["total_rays"], (th, r["total_rays"], base_c["total_rays"])
        img, r = _render(tmp_path, spec, th, True)
        assert_bits_equal(base, img, f"counting build, threshold {th} vs off")
        for k in COUNTERS:
            assert r["stats"][k] == off["stats"][k], (th, k, r["stats"][k], off["stats"][k])
        assert r["stats"].get("slow_paths") == off["stats"].get("slow_paths"), th
        assert r["dbg"][20] == 0, "packet cull violation"
        # the walk of the primary rays is the same with and without the feature: what the counters add is the in-place walks
        assert r["dbg"][21] == off["dbg"][21] and off["dbg"][22] == 0
        if th is None:
            dbg = r["dbg"]
    d = dbg if dbg is not None else off["dbg"]
    print(f"\n{spec['scene']} {spec['w']}x{spec['h']} depth {spec['maxdepth']} spp {spec['spp']}: {d[21]} mirror rays, "
          f"{d[22]} traced in place, {base_c['total_rays']} rays, slow paths {off['stats'].get('slow_paths')}")
    return dbg, off


def _spec(**kw):
    s = {"scene": "canonical", "w": 64, "h": 64, "size": (1.0, 1.0), "pos": [2.0, 0.0, 0.0], "dir": [0.0, 0.0, 1.0], "fov": 90.0,
         "roll": 0.0, "maxdepth": 5, "spp": 4, "seed": 3}
    s.update(kw)
    return s


def test_frame_aimed_at_mirror_disk(tmp_path):
    """A narrow view filled by disk 1: nearly every wave of k_path_primary continues its paths in place."""
    spec = _spec(w=40, h=40, dir=[2.0, 4.0, 7.0], fov=12.0, spp=16)
    dbg, _ = _check(tmp_path, spec, thresholds=(None, 1, 64))
    assert dbg[21] > 0 and dbg[22] >= dbg[21] // 2, dbg[21:23]


@pytest.mark.parametrize("maxdepth", [1, 2, 5])
def test_canonical_view_depths(tmp_path, maxdepth):
    """The canonical camera: disk 1 reflects the teapot (Matte), so the in-place reflections push to the pass-2 queue."""
    dbg, _ = _check(tmp_path, _spec(maxdepth=maxdepth), thresholds=(None, 1))
    if maxdepth > 1:
        assert dbg[22] > 0
    else:
        assert dbg[21] == 0  # depth 1: no path goes on


@pytest.mark.parametrize("spp", [1, 64])
def test_canonical_view_packet_off_and_wide(tmp_path, spp):
    """spp 1: a wave holds 64 pixels (the packet is too wide to cull); spp 64: one pixel per wave."""
    _check(tmp_path, _spec(w=48 if spp == 64 else 96, h=48 if spp == 64 else 96, spp=spp), thresholds=(None, 16))


def test_axis_mirrors_near_zero_component_reflections(tmp_path):
    """Two 45-degree mirrors seen by a camera with a tiny roll: primary directions with a tiny x component reflect into
    directions whose z (then x) component is a rounding-level cancellation, which may come out exactly zero and then leaves
    the in-place path for the slow path (bounce index 1, or 2 after an in-place bounce).  The frame must be right either
    way; the slow paths the counting build saw beyond the primary rays' own are printed."""
    spec = _spec(scene="mirrors", w=65, h=65, pos=[0.0, 0.0, 0.0], fov=30.0, roll=1e-7, spp=1)
    from oracle import orc
    vo = orc.create_viewport(65, 65, (1.0, 1.0), [0.0, 0.0, 0.0], orc.unit([0.0, 0.0, 1.0]), 30.0, 1e-7)
    _, d4 = orc.primary_rays(65, 65, vo, 1, seed=3)
    nzero = int(((d4[:, :3] == 0).any(axis=1)).sum())
    dbg, off = _check(tmp_path, spec, thresholds=(None, 1))
    assert dbg[22] > 0
    assert off["stats"]["slow_paths"] >= nzero
    print(f"slow paths {off['stats']['slow_paths']}, of them zero-component primary rays {nzero}")
