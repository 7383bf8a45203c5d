"""-m gpu: first-hit feature buffers (rtmi_render_features / rtmi_render_features_device, HipRayCaster.walk_rays_features).
Every buffer is compared bit for bit with the NumPy restatement of tests/features_ref.py, whose inputs are the oracle's own
primary rays, closest hits and triangle records: the expected values never come from the code under test.
Every case renders in a fresh process (run_spec / case_* below); the parent computes the expectation and compares."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import (GOLDEN, OracleApi, ProductApi, assert_bits_equal, recipe_axis_box, recipe_canonical, recipe_circles,
                      recipe_circles_analytic)
import features_ref as FR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTERS = ("box_tests", "tri_tests", "full_tests", "nodes", "leaves")
RTMI_OK, RTMI_ERR_UNSUPPORTED = 0, 3
# a raw viewport whose primary rays all have an exactly-zero x component (tests/test_ray_records.py)
SLOW_VP12 = [2.0, 0.6, 1.0, 2.0, 0.0, 0.0, 0.0, -1.2, 0.0, 0.0, 0.0, 0.5]

RECIPES = {
    "canonical": recipe_canonical(),
    "canonical_6": recipe_canonical(maxdepth=6),
    "solid": recipe_canonical(solid_teapot=True),
    "trivial": recipe_canonical(accel="trivial"),
    "circles": recipe_circles(),
    "axis_box": recipe_axis_box(),
    "analytic": recipe_circles_analytic(),
}
# view: "canonical" (canonical_viewport), "axis" (straight down +z through the axis-aligned box: rays parallel to its walls)
# or "slow" (SLOW_VP12).  tile None: the whole frame through the host variant; otherwise the device variant on that tile.
SPECS = {
    "golden": dict(scene="solid", w=64, h=64, spp=1, seed=1),
    "canon_s4": dict(scene="canonical", w=64, h=48, spp=4, seed=1),
    "canon_6_19": dict(scene="canonical_6", w=64, h=48, spp=4, seed=1),
    "range_tile": dict(scene="canonical", w=64, h=48, spp=8, seed=1, sample0=3, nsamples=4, tile=(2, 24, 4, 8)),
    "first_sample": dict(scene="canonical", w=64, h=48, spp=4, seed=1, sample0=0, nsamples=1),
    "last_samples_device": dict(scene="canonical", w=64, h=48, spp=64, seed=2, sample0=0, nsamples=64, tile=(8, 8, 8, 0)),
    "circles": dict(scene="circles", w=64, h=48, spp=4, seed=3),
    "linear": dict(scene="trivial", w=64, h=48, spp=4, seed=1),
    "generic": dict(scene="canonical", w=64, h=48, spp=4, seed=1, opts=("GENERIC",)),
    "axis_box": dict(scene="axis_box", view="axis", w=33, h=33, spp=1, seed=1),
    "axis_box_s2": dict(scene="axis_box", view="axis", w=33, h=33, spp=2, seed=1),
    "slow": dict(scene="circles", view="slow", w=48, h=40, spp=4, seed=3),
    "counters": dict(scene="canonical", w=64, h=48, spp=4, seed=1, opts=("COUNTERS",)),
    "counters_range_tile": dict(scene="canonical", w=64, h=48, spp=8, seed=1, sample0=3, nsamples=4, tile=(2, 24, 4, 8), opts=("COUNTERS",)),
    "counters_linear": dict(scene="trivial", w=64, h=48, spp=4, seed=1, opts=("COUNTERS",)),
    "counters_generic": dict(scene="canonical", w=64, h=48, spp=4, seed=1, opts=("GENERIC", "COUNTERS")),
}
SCALE = dict(scene="canonical", w=256, h=256, spp=16, seed=1)
SCALE_TUNINGS = [dict(batch_paths=150000, streams=k, subtile_min_paths=1) for k in (1, 2, 4)]

_RUN = r"""
import json, os, sys
import numpy as np
root, name, out = sys.argv[1], sys.argv[2], sys.argv[3]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
import test_features as T
arrays, info = (T.run_spec(T.SPECS[name[5:]]) if name.startswith("spec_") else getattr(T, "case_" + name)())
np.savez(out + ".npz", **arrays)
with open(out + ".json", "w") as f:
    json.dump(info, f)
"""


def _run(tmp_path, name):
    out = str(tmp_path / name)
    subprocess.run([sys.executable, "-c", _RUN, ROOT, name, out], check=True, timeout=600)
    with open(out + ".json") as f:
        info = json.load(f)
    with np.load(out + ".npz") as z:
        return {k: z[k] for k in z.files}, info


def _ints(stats):
    return {k: int(v) for k, v in stats.items() if isinstance(v, (int, np.integer))}


def _vp12(m, spec):
    """The 12 viewport floats of a spec; m is the oracle module or the product module (they build the same bits)."""
    view = spec.get("view", "canonical")
    if view == "slow":
        return np.asarray(SLOW_VP12, np.float32)
    if view == "axis":
        if hasattr(m, "Viewport"):
            return m.create_viewport((spec["w"], spec["h"]), (1.0, 1.0), [0.0, 0.0, 0.0], m.unit([0.0, 0.0, 1.0]), 90.0, 0.0, 1, 1).vp12.copy()
        return m.create_viewport(spec["w"], spec["h"], (1.0, 1.0), [0.0, 0.0, 0.0], m.unit([0.0, 0.0, 1.0]), 90.0, 0.0)
    if hasattr(m, "Viewport"):
        return m.canonical_viewport(spec["w"], spec["h"], 1, 1).vp12.copy()
    return m.canonical_viewport(spec["w"], spec["h"])


# ---------------------------------------------------------------- what the child processes run
def _caster(R, spec, tuning=None):
    options = 0
    for o in spec.get("opts", ()):
        options |= getattr(R, "OPT_" + o)
    return R.HipRayCaster(seed=spec["seed"], options=options, tuning=tuning)


def _device_call(R, c, vp, sp, tile, sample0, nsamples, want=(True, True, True)):
    """One rtmi_render_features_device call on torch buffers prefilled with NaN / 0xFFFFFFFF; -> arrays (None where not wanted), ctx"""
    import torch
    dev = torch.device("cuda", 0)
    n, w = tile[1], vp.width
    bufs = [torch.full((n, w, 4), float("nan"), dtype=torch.float32, device=dev) if want[0] else None,
            torch.full((n, w, 4), float("nan"), dtype=torch.float32, device=dev) if want[1] else None,
            torch.full((n, w), -1, dtype=torch.int32, device=dev) if want[2] else None]
    torch.cuda.synchronize()
    ctx = c.walk_features_device(vp, sp, tile, *[b.data_ptr() if b is not None else None for b in bufs], sample0, nsamples,
                                 torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = [b.cpu().numpy() if b is not None else None for b in bufs]
    if out[2] is not None:
        out[2] = out[2].view(np.uint32)
    return out, ctx


def run_spec(spec, tuning=None):
    """The spec's features call: host variant for a whole frame, device variant for a tile."""
    from rust_raytrace_amd import raytrace as R
    sp = RECIPES[spec["scene"]](ProductApi(R))
    vp = R.Viewport(spec["w"], spec["h"], _vp12(R, spec), 7, spec["spp"])
    c = _caster(R, spec, tuning)
    s0, n = spec.get("sample0", 0), spec.get("nsamples")
    if spec.get("tile") is None:
        alb, nrm, ids, ctx = c.walk_rays_features(vp, sp, s0, n)
    else:
        (alb, nrm, ids), ctx = _device_call(R, c, vp, sp, spec["tile"], s0, n)
    return {"albedo": alb, "normal": nrm, "ids": ids}, {"stats": _ints(ctx.stats), "rays": int(ctx.total_rays)}


def case_scale():
    """256 x 256 @ 16 with the default tuning, then in several batches on 1, 2 and 4 streams."""
    a, info = run_spec(SCALE)
    info["same"], info["tuned"] = [], []
    for t in SCALE_TUNINGS:
        b, bi = run_spec(SCALE, t)
        info["same"].append(all(np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in a))
        info["tuned"].append(bi["stats"])
    return a, info


def case_subsets():
    """Every subset of the three outputs on the device variant, each in a call of its own."""
    from rust_raytrace_amd import raytrace as R
    spec = SPECS["canon_s4"]
    sp = RECIPES[spec["scene"]](ProductApi(R))
    vp = R.Viewport(spec["w"], spec["h"], _vp12(R, spec), 5, spec["spp"])
    c = _caster(R, spec)
    tile = (0, spec["h"], spec["h"], 0)
    arrays = {}
    for mask in range(1, 8):
        want = (bool(mask & 1), bool(mask & 2), bool(mask & 4))
        out, _ = _device_call(R, c, vp, sp, tile, 0, None, want)
        for name, a in zip(("albedo", "normal", "ids"), out):
            if a is not None:
                arrays[f"{name}_{mask}"] = a
    return arrays, {}


def case_shared_buffers():
    """rtmi_render before and after a features call on one scene handle, and the host variant against the device variant."""
    from rust_raytrace_amd import raytrace as R
    spec = SPECS["canon_s4"]
    w, h = spec["w"], spec["h"]
    vp = R.Viewport(w, h, _vp12(R, spec), 5, spec["spp"])
    fresh = np.zeros((h, w, 4), np.float32)
    R.HipRayCaster(seed=spec["seed"]).walk_rays(vp, RECIPES[spec["scene"]](ProductApi(R)), fresh, 1, False)
    sp = RECIPES[spec["scene"]](ProductApi(R))
    c = R.HipRayCaster(seed=spec["seed"])
    before, after = np.zeros((h, w, 4), np.float32), np.zeros((h, w, 4), np.float32)
    r0 = c.walk_rays(vp, sp, before, 1, False).total_rays
    alb, nrm, ids, _ = c.walk_rays_features(vp, sp)
    (dalb, dnrm, dids), _ = _device_call(R, c, vp, sp, (0, h, h, 0), 0, None)
    r1 = c.walk_rays(vp, sp, after, 1, False).total_rays
    into = np.full((h, w, 4), np.nan, np.float32)
    got = c.walk_rays_features(vp, sp, albedo=into, normal=False, ids=False)
    return ({"fresh": fresh, "before": before, "after": after, "albedo": alb, "normal": nrm, "ids": ids, "d_albedo": dalb, "d_normal": dnrm,
             "d_ids": dids, "into": into},
            {"rays": [int(r0), int(r1)], "same_object": got[0] is into, "left_out": [got[1] is None, got[2] is None]})


class Sphere(C.Structure):
    _fields_ = [("center", C.c_float * 3), ("radius", C.c_float), ("surface_kind", C.c_uint32), ("color", C.c_float * 3),
                ("alpha", C.c_float), ("scattering", C.c_float)]


def case_analytic():
    """A scene with analytic spheres: the host mirror's message and a render afterwards; the ABI's code on a raw handle."""
    import test_gpu_abi_raw as A
    from oracle import orc
    from rust_raytrace_amd import raytrace as R
    w, h = 32, 24
    vp = R.canonical_viewport(w, h, 5, 2)
    fresh = np.zeros((h, w, 4), np.float32)
    R.HipRayCaster(seed=1).walk_rays(vp, RECIPES["analytic"](ProductApi(R)), fresh, 1, False)
    sp = RECIPES["analytic"](ProductApi(R))
    c = R.HipRayCaster(seed=1)
    try:
        c.walk_rays_features(vp, sp)
        msg = ""
    except RuntimeError as e:
        msg = str(e)
    after = np.zeros((h, w, 4), np.float32)
    rays = c.walk_rays(vp, sp, after, 1, False).total_rays
    # the raw ABI: the canonical scene with one sphere added
    L, ffi = A._lib()
    so = recipe_canonical()(OracleApi(orc))
    tris, geo, topo, refs = A._abi_arrays(so)
    rc, hnd = A._create(L, tris, A._boxes(geo, topo), refs)
    assert rc == RTMI_OK, L.rtmi_last_error()
    sph = Sphere((C.c_float * 3)(0.0, 0.5, 5.0), 0.5, 0, (C.c_float * 3)(1.0, 0.0, 0.0), 0.0, 0.0)
    L.rtmi_scene_set_spheres.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
    assert L.rtmi_scene_set_spheres(hnd, C.byref(sph), 1) == RTMI_OK, L.rtmi_last_error()
    vp12 = orc.canonical_viewport(w, h)
    avp = A.Vp(w, h, (C.c_float * 3)(*vp12[0:3]), (C.c_float * 3)(*vp12[3:6]), (C.c_float * 3)(*vp12[6:9]), (C.c_float * 3)(*vp12[9:12]), 5, 2)
    ids = np.full((h, w), 0xDEADBEEF, np.uint32)
    st = ffi.Stats()
    st.rays = 123
    code = L.rtmi_render_features(hnd, C.byref(avp), 1, 0, h, 0, 2, None, None, ids.ctypes.data_as(C.c_void_p), C.byref(st))
    raw_msg = L.rtmi_last_error().decode()
    _, rst = A._render(L, ffi, hnd, vp12, w, h, 5, 2, 1)
    L.rtmi_scene_destroy(hnd)
    return ({"fresh": fresh, "after": after, "ids": ids},
            {"msg": msg, "rays": int(rays), "code": int(code), "raw_msg": raw_msg, "raw_stats_rays": int(st.rays), "raw_render_rays": int(rst.rays)})


# ---------------------------------------------------------------- the checks (parent process)
@functools.lru_cache(maxsize=None)
def _oracle_scene(scene):
    from oracle import orc
    return RECIPES[scene](OracleApi(orc))


def _expected(spec):
    from oracle import orc
    return FR.features_ref(orc, _oracle_scene(spec["scene"]), spec["w"], spec["h"], _vp12(orc, spec), spec["spp"], spec["seed"],
                           spec.get("sample0", 0), spec.get("nsamples"), spec.get("tile"))


def _check(a, info, spec, what):
    alb, nrm, ids, cn = _expected(spec)
    assert np.array_equal(a["ids"], ids), f"{what}: {(a['ids'] != ids).sum()} of {ids.size} ids differ"
    assert_bits_equal(a["albedo"], alb, f"{what}: albedo")
    assert_bits_equal(a["normal"], nrm, f"{what}: normal")
    st = info["stats"]
    n = spec.get("nsamples") or spec["spp"] - spec.get("sample0", 0)
    assert st["rays"] == ids.size * n == info["rays"] == cn["rays"], (st["rays"], ids.size * n, cn["rays"])
    assert st["pipeline"] == 1 and st["slow_paths"] == 0 and st["trace_launches"] >= 1 and 1 <= st["streams"] <= 4, st
    if "COUNTERS" in spec.get("opts", ()):
        for k in COUNTERS:
            assert st[k] == cn[k], (what, k, st[k], cn[k])
    else:
        assert all(st[k] == 0 for k in COUNTERS), st
    return alb, nrm, ids


def _check_spec(tmp_path, name):
    a, info = _run(tmp_path, "spec_" + name)
    return a, _check(a, info, SPECS[name], name)


def test_first_hit_map_of_the_golden_view(tmp_path):
    """Canonical 64 x 64, S = 1: ids and normal.w against the committed map; coverage is 0 or 1."""
    a, _ = _check_spec(tmp_path, "golden")
    z = np.load(os.path.join(GOLDEN, "canonical_64x64_first_hits.npz"))
    tri, t, face = z["tri"].reshape(64, 64), z["t"].reshape(64, 64), z["face"].reshape(64, 64)
    hit = tri != 0
    assert np.array_equal(a["ids"], np.where(hit, tri | (face << 30), 0).astype(np.uint32))
    assert_bits_equal(a["normal"][..., 3][hit], t[hit], "normal.w vs the map's t")
    assert not a["normal"][~hit].any()
    assert np.array_equal(a["albedo"][..., 3], hit.astype(np.float32))


def test_all_samples_of_the_canonical_view(tmp_path):
    """Canonical 64 x 48, S = 4, octree (10, 19); the case must exercise every row of the table but Solid."""
    a, (alb, nrm, ids) = _check_spec(tmp_path, "canon_s4")
    cov = alb[..., 3]
    assert ((cov > 0) & (cov < 1)).sum() > 50, "partial coverage"
    assert (ids >> 30 == 1).any() and (ids >> 30 >= 2).any() and (ids == 0).any()


def test_the_shallow_octree_of_the_issue(tmp_path):
    """Octree (6, 19), the scene the issue's figures were taken on: 116 pixels with partial coverage."""
    _, (alb, _, _) = _check_spec(tmp_path, "canon_6_19")
    cov = alb[..., 3]
    assert ((cov > 0) & (cov < 1)).sum() == 116


def test_a_sample_range_on_a_striped_tile(tmp_path):
    _check_spec(tmp_path, "range_tile")


def test_one_sample_of_a_larger_frame_is_jittered(tmp_path):
    """S = 4, sample0 = 0, nsamples = 1 is the first sample of the S = 4 rays, not the centred ray of S = 1."""
    a, (alb, nrm, ids) = _check_spec(tmp_path, "first_sample")
    centred = _expected(dict(SPECS["first_sample"], spp=1, nsamples=None))
    assert not np.array_equal(nrm.view(np.uint32), centred[1].view(np.uint32)), "the case does not tell the two rays apart"
    full = _expected(SPECS["canon_s4"])
    assert np.array_equal(ids, full[2]), "ids are the hit of sample sample0 = 0 in both calls"


def test_sixty_four_samples_on_the_device(tmp_path):
    _check_spec(tmp_path, "last_samples_device")


@pytest.mark.parametrize("name", ["circles", "linear", "generic", "axis_box", "axis_box_s2", "slow"])
def test_other_scenes_and_walks(tmp_path, name):
    a, (alb, nrm, ids) = _check_spec(tmp_path, name)
    if name == "circles":
        from oracle import orc
        _, kinds, _ = _oracle_scene("circles").triangles()
        first = kinds[(ids & 0x3FFFFFFF)[(ids != 0) & (ids >> 30 < 2)]]
        assert (first == orc.SOLID).any(), "Solid first hits"
        assert (ids >> 30 >= 2).any(), "wire-frame edges"
    if name == "axis_box":
        assert not np.isfinite(nrm[..., 3]).all(), "the case must hold a non-finite hit time"
    if name == "slow":
        from oracle import orc
        _, d4 = orc.primary_rays(48, 40, np.asarray(SLOW_VP12, np.float32), 4, 3)
        assert (d4[:, 0] == 0).all()


def test_scale_and_tuning(tmp_path):
    """256 x 256 @ 16 (1 M rays): the default tuning against the restatement, then several batches on 1, 2, 4 streams."""
    a, info = _run(tmp_path, "scale")
    _check(a, info, SCALE, "scale")
    assert info["same"] == [True] * len(SCALE_TUNINGS), info["same"]
    for t, st in zip(SCALE_TUNINGS, info["tuned"]):
        assert st["streams"] == t["streams"] and st["rays"] == info["stats"]["rays"], (t, st)
        assert st["trace_launches"] > t["streams"], ("several batches", t, st)


def test_each_subset_of_the_outputs(tmp_path):
    a, _ = _run(tmp_path, "subsets")
    alb, nrm, ids, _ = _expected(SPECS["canon_s4"])
    for mask in range(1, 8):
        for bit, name, ref in ((1, "albedo", alb), (2, "normal", nrm), (4, "ids", ids)):
            key = f"{name}_{mask}"
            assert (key in a) == bool(mask & bit)
            if key in a:
                assert np.array_equal(a[key].view(np.uint32), a[f"{name}_7"].view(np.uint32)), key
        assert_bits_equal(a["albedo_7"], alb, "albedo")
        assert_bits_equal(a["normal_7"], nrm, "normal")
        assert np.array_equal(a["ids_7"], ids)


@pytest.mark.parametrize("name", ["counters", "counters_range_tile", "counters_linear", "counters_generic"])
def test_work_counters_equal_the_oracles(tmp_path, name):
    _check_spec(tmp_path, name)


def test_render_is_unchanged_around_a_features_call(tmp_path):
    a, info = _run(tmp_path, "shared_buffers")
    assert_bits_equal(a["before"], a["fresh"], "render before the features call vs a fresh handle")
    assert_bits_equal(a["after"], a["fresh"], "render after the features call vs a fresh handle")
    assert info["rays"][0] == info["rays"][1]
    alb, nrm, ids, _ = _expected(SPECS["canon_s4"])
    for got in ("", "d_"):
        assert_bits_equal(a[got + "albedo"], alb, got + "albedo")
        assert_bits_equal(a[got + "normal"], nrm, got + "normal")
        assert np.array_equal(a[got + "ids"], ids), got + "ids"
    assert_bits_equal(a["into"], alb, "albedo into the caller's array")
    assert info["same_object"] and info["left_out"] == [True, True]


def test_analytic_spheres_are_unsupported(tmp_path):
    a, info = _run(tmp_path, "analytic")
    assert "analytic spheres" in info["msg"], info["msg"]
    assert_bits_equal(a["after"], a["fresh"], "render after the refused call vs a fresh handle")
    assert info["rays"] > 0
    assert info["code"] == RTMI_ERR_UNSUPPORTED and "analytic spheres" in info["raw_msg"], (info["code"], info["raw_msg"])
    assert info["raw_stats_rays"] == 0 and info["raw_render_rays"] > 0
    assert (a["ids"] == 0xDEADBEEF).all(), "a refused call writes nothing"
