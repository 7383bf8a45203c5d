"""-m gpu: per-ray records of the octree walk (rtmi_trace_records / rtmi_primary_records, HipRayCaster.*_records,
Scene.debug_en).  Every record is checked against the oracle's trace of that single ray: the ray's bits, its hit, its five
work counters and its leaves (their lists' sizes sum to the ray's tri_tests).  Every case runs on the GPU in a fresh
process (case_* below); the parent compares with the oracle on the host."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import OracleApi, ProductApi, assert_bits_equal, recipe_canonical, recipe_circles, recipe_circles_analytic

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTERS = ("box_tests", "tri_tests", "full_tests", "nodes", "leaves")
RTMI_OK, RTMI_ERR_INVALID, RTMI_ERR_UNSUPPORTED = 0, 1, 3
# a raw viewport whose primary rays all have an exactly-zero x component (tests/test_progressive.py)
SLOW_VP12 = [2.0, 0.6, 1.0, 2.0, 0.0, 0.0, 0.0, -1.2, 0.0, 0.0, 0.0, 0.5]

_RUN = r"""
import json, os, sys
import numpy as np
root, name, out = sys.argv[1], sys.argv[2], sys.argv[3]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
import test_ray_records as T
inp = None
if os.path.exists(out + ".in.npz"):
    with np.load(out + ".in.npz") as z:
        inp = {k: z[k] for k in z.files}
arrays, info = getattr(T, "case_" + name)(inp)
np.savez(out + ".npz", **arrays)
with open(out + ".json", "w") as f:
    json.dump(info, f)
"""


def _run(tmp_path, name, inp=None):
    out = str(tmp_path / name)
    if inp is not None:
        np.savez(out + ".in.npz", **inp)
    subprocess.run([sys.executable, "-c", _RUN, ROOT, name, out], check=True, timeout=600)
    with open(out + ".json") as f:
        info = json.load(f)
    with np.load(out + ".npz") as z:
        return {k: z[k] for k in z.files}, info


def _ints(stats):
    return {k: int(v) for k, v in stats.items() if isinstance(v, (int, np.integer))}


# ---------------------------------------------------------------- what the child processes run
def _rec_arrays(rec, prefix=""):
    a = {prefix + k: getattr(rec, k) for k in ("orig", "dir", "tri", "t", "face", "nleaves", "leaf_first", "leaf_ids")}
    for k, v in rec.counters.items():
        a[prefix + "c_" + k] = v
    if rec.pixel is not None:
        a[prefix + "pixel"] = rec.pixel
    return a


def _tree_arrays(sp):
    _, topo, refs = sp.tree()
    return {"topo": topo, "refs": refs}


def _primary_case(recipe, w, h, spp, seed, vp12=None, row0=0, nrows=None, sample=0):
    from rust_raytrace_amd import raytrace as R
    sp = recipe(ProductApi(R))
    vp = R.Viewport(w, h, vp12, 5, spp) if vp12 is not None else R.canonical_viewport(w, h, 5, spp)
    rec = R.HipRayCaster(seed=seed).primary_records(vp, sp, row0, nrows, sample)
    # rtmi_trace with RTMI_OPT_COUNTERS on the same rays: its counters must equal the records' sums
    _, _, _, st = R.HipRayCaster(seed=seed, options=R.OPT_COUNTERS).trace(sp, rec.orig, rec.dir)
    return {**_rec_arrays(rec), **_tree_arrays(sp)}, {"stats": _ints(rec.stats), "trace_stats": _ints(st)}


def case_canonical(inp):
    return _primary_case(recipe_canonical(), 64, 64, 1, 1)


def case_samples(inp):
    return _primary_case(recipe_canonical(), 64, 64, 4, 1, row0=17, nrows=9, sample=2)


def case_circles_slow(inp):
    return _primary_case(recipe_circles(), 48, 40, 1, 3, vp12=SLOW_VP12)


def case_explicit(inp):
    from rust_raytrace_amd import raytrace as R
    sp = recipe_canonical()(ProductApi(R))
    rec = R.HipRayCaster(seed=1).trace_records(sp, inp["o4"], inp["d4"])
    _, _, _, st = R.HipRayCaster(seed=1, options=R.OPT_COUNTERS).trace(sp, inp["o4"], inp["d4"])
    return {**_rec_arrays(rec), **_tree_arrays(sp)}, {"stats": _ints(rec.stats), "trace_stats": _ints(st)}


def case_sizes(inp):
    """Size query vs fill, a too-small leaf_cap, two calls, and a render before / after a record call on one handle."""
    from rust_raytrace_amd import _ffi, raytrace as R
    L = _ffi.lib()
    sp = recipe_canonical()(ProductApi(R))
    w = h = 32
    vp = R.canonical_viewport(w, h, 5, 2)
    c = R.HipRayCaster(seed=5)
    before = np.zeros((h, w, 4), np.float32)
    ctx0 = c.walk_rays(vp, sp, before, 1, False)
    n = w * h

    def call(ids, cap):
        recs = np.zeros(n, R.REC_DTYPE)
        tot, st = C.c_uint64(0), _ffi.Stats()
        rc = L.rth_caster_primary_records(sp.h, w, h, R._p(vp.vp12), vp.maxdepth, vp.samples_per_pixel, 0, h, 1, R._p(recs),
                                          R._p(ids) if ids is not None else None, cap, C.byref(tot), C.byref(st))
        return rc, recs, tot.value, L.rth_last_error().decode()

    rc0, q, total, _ = call(None, 0)
    assert rc0 == 0
    ids1 = np.zeros(total, np.uint32)
    rc1, f1, t1, _ = call(ids1, total)
    small = np.full(total, 0xDEADBEEF, np.uint32)
    rc2, _, t2, msg2 = call(small, total - 1)
    ids3 = np.zeros(total, np.uint32)
    rc3, f3, _, _ = call(ids3, total)
    after = np.zeros((h, w, 4), np.float32)
    ctx1 = c.walk_rays(vp, sp, after, 1, False)
    return ({"query": q, "fill1": f1, "fill3": f3, "ids1": ids1, "ids3": ids3, "small": small, "before": before, "after": after},
            {"rc": [rc0, rc1, rc2, rc3], "totals": [total, t1, t2], "msg2": msg2, "rays": [int(ctx0.total_rays), int(ctx1.total_rays)]})


def _raw_handle(options):
    """rtmi_scene_t of the canonical scene (raw ABI, tests/test_gpu_abi_raw.py's helpers) and its library"""
    import test_gpu_abi_raw as A
    from oracle import orc
    L, ffi = A._lib()
    L.rtmi_primary_records.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                       C.c_uint64, C.c_void_p, C.c_void_p]
    so = recipe_canonical()(OracleApi(orc))
    tris, geo, topo, refs = A._abi_arrays(so)
    rc, hnd = A._create(L, tris, A._boxes(geo, topo), refs)
    assert rc == RTMI_OK, L.rtmi_last_error()
    assert L.rtmi_scene_set_options(hnd, options) == RTMI_OK
    return A, L, ffi, hnd


def case_unsupported(inp):
    """RTMI_ERR_UNSUPPORTED for the modes and scenes k_trace_oct does not run; the handle renders afterwards."""
    from rust_raytrace_amd import raytrace as R
    from oracle import orc
    w = h = 16
    vp12 = orc.canonical_viewport(w, h)
    codes, msgs, renders = {}, {}, {}
    for name, opt in (("generic", R.OPT_GENERIC), ("bvh", R.OPT_BVH), ("fast", R.OPT_FAST)):
        A, L, ffi, hnd = _raw_handle(opt)
        vp = A.Vp(w, h, (C.c_float * 3)(*vp12[0:3]), (C.c_float * 3)(*vp12[3:6]), (C.c_float * 3)(*vp12[6:9]), (C.c_float * 3)(*vp12[9:12]), 5, 1)
        recs = np.zeros(w * h, R.REC_DTYPE)
        tot = C.c_uint64(7)
        codes[name] = L.rtmi_primary_records(hnd, C.byref(vp), 1, 0, h, 0, R._p(recs), None, 0, C.byref(tot), None)
        msgs[name] = L.rtmi_last_error().decode()
        img, st = A._render(L, ffi, hnd, vp12, w, h, 5, 1, 1)
        renders[name] = int(st.rays)
        L.rtmi_scene_destroy(hnd)
    # trivial one-leaf tree and analytic spheres through the host mirror (the C view reports the ABI's message)
    for name, recipe in (("trivial", recipe_canonical(accel="trivial")), ("spheres", recipe_circles_analytic())):
        sp = recipe(ProductApi(R))
        vp = R.canonical_viewport(w, h, 5, 1)
        c = R.HipRayCaster(seed=1)
        try:
            c.primary_records(vp, sp)
            msgs[name] = ""
        except RuntimeError as e:
            msgs[name] = str(e)
        img = np.zeros((h, w, 4), np.float32)
        renders[name] = int(c.walk_rays(vp, sp, img, 1, False).total_rays)
    return {}, {"codes": codes, "msgs": msgs, "renders": renders}


def case_debug_en(inp):
    """walk_rays with Scene.debug_en: the same image, debug_records() == primary_records(sample=0), the CSV; on an
    unsupported scene it raises before rendering."""
    import io
    from rust_raytrace_amd import raytrace as R
    sp = recipe_canonical()(ProductApi(R))
    w, h = 24, 20
    vp = R.canonical_viewport(w, h, 5, 2)
    c = R.HipRayCaster(seed=2)
    off = np.zeros((h, w, 4), np.float32)
    c0 = c.walk_rays(vp, sp, off, 1, False)
    assert sp.debug_records() is None
    sp.debug_en = True
    on = np.zeros((h, w, 4), np.float32)
    c1 = c.walk_rays(vp, sp, on, 1, False)
    dbg = sp.debug_records()
    ref = c.primary_records(vp, sp, 0, None, 0)
    buf = io.StringIO()
    dbg.write_csv(buf, sp)
    st = recipe_canonical(accel="trivial")(ProductApi(R))
    st.debug_en = True
    untouched = np.full((h, w, 4), 7.0, np.float32)
    try:
        c.walk_rays(vp, st, untouched, 1, False)
        raised = ""
    except RuntimeError as e:
        raised = str(e)
    return ({"off": off, "on": on, "untouched": untouched, **_rec_arrays(dbg, "d_"), **_rec_arrays(ref, "r_")},
            {"rays": [int(c0.total_rays), int(c1.total_rays)], "csv": buf.getvalue(), "raised": raised})


# ---------------------------------------------------------------- oracle side
def _oracle_scene(recipe):
    from oracle import orc
    return recipe(OracleApi(orc))


def _check_records(a, info, so, o4, d4):
    """Every record against the oracle's trace of its single ray; the stats against rtmi_trace's counters."""
    n = len(o4)
    assert_bits_equal(a["orig"], o4, "record orig")
    assert_bits_equal(a["dir"], d4, "record dir")
    tri, t, face, _ = so.trace(o4, d4)
    assert np.array_equal(a["tri"], tri), f"hit triangles: {int((a['tri'] != tri).sum())} of {n} differ"
    assert_bits_equal(a["t"], t, "hit t")
    assert np.array_equal(a["face"], face), "faces differ"
    topo, refs, ids = a["topo"], a["refs"], a["leaf_ids"]
    assert len(ids) == int(a["nleaves"].sum())
    assert np.array_equal(a["leaf_first"], np.concatenate([[0], np.cumsum(a["nleaves"].astype(np.uint64))[:-1]]).astype(np.uint64))
    assert (topo[ids, 2] == 1).all(), "a visited id is not a leaf of Scene.tree()"
    bad = []
    for i in range(n):
        _, _, _, cn = so.trace(o4[i:i + 1], d4[i:i + 1])
        mine = {k: int(a["c_" + k][i]) for k in COUNTERS}
        want = {k: cn[k] for k in COUNTERS}
        lv = ids[int(a["leaf_first"][i]):int(a["leaf_first"][i]) + int(a["nleaves"][i])]
        sizes = int(topo[lv, 1].astype(np.int64).sum())
        if mine != want or sizes != want["tri_tests"]:
            bad.append((i, mine, want, sizes))
        elif a["tri"][i] != 0:
            check = np.unique(np.concatenate([refs[topo[b, 0]:topo[b, 0] + topo[b, 1]] for b in lv]))
            if a["tri"][i] not in check:
                bad.append((i, "hit not in check_tris"))
    assert not bad, f"{len(bad)} of {n} records differ from the oracle; first: {bad[:3]}"
    st, ts = info["stats"], info["trace_stats"]
    assert st["rays"] == n
    for k in COUNTERS:
        assert st[k] == int(a["c_" + k].sum()) == ts[k], (k, st[k], ts[k])


def test_canonical_every_pixel(tmp_path):
    from oracle import orc
    a, info = _run(tmp_path, "canonical")
    o4, d4 = orc.primary_rays(64, 64, orc.canonical_viewport(64, 64), 1, seed=1)
    # (no primary ray of this small frame has an exactly-zero component: test_circles_zero_component_rays has only such rays)
    _check_records(a, info, _oracle_scene(recipe_canonical()), o4, d4)
    assert np.array_equal(a["pixel"], np.stack([np.arange(64 * 64) // 64, np.arange(64 * 64) % 64], axis=1))


def test_sample_of_a_row_range(tmp_path):
    from oracle import orc
    a, info = _run(tmp_path, "samples")
    o4, d4 = orc.primary_rays(64, 64, orc.canonical_viewport(64, 64), 4, seed=1, row0=17, nrows=9)
    _check_records(a, info, _oracle_scene(recipe_canonical()), o4[2::4], d4[2::4])
    assert a["pixel"][0].tolist() == [17, 0] and a["pixel"][-1].tolist() == [25, 63]


def test_circles_zero_component_rays(tmp_path):
    from oracle import orc
    a, info = _run(tmp_path, "circles_slow")
    o4, d4 = orc.primary_rays(48, 40, SLOW_VP12, 1, seed=3)
    assert (d4[:, 0] == 0).all()
    _check_records(a, info, _oracle_scene(recipe_circles()), o4, d4)


def test_explicit_rays_inside_the_scene(tmp_path):
    from oracle import orc
    so = _oracle_scene(recipe_canonical())
    po, pd = orc.primary_rays(32, 32, orc.canonical_viewport(32, 32), 1, seed=1)
    tri, t, _, _ = so.trace(po, pd)
    hit = np.nonzero(tri != 0)[0][::3]
    rng = np.random.default_rng(7)
    o4 = np.zeros((len(hit), 4), np.float32)
    o4[:, :3] = po[hit, :3] + t[hit, None] * pd[hit, :3]
    d4 = np.zeros((len(hit), 4), np.float32)
    for j in range(len(hit)):
        d4[j, :3] = orc.unit(rng.normal(size=3).astype(np.float32))
    a, info = _run(tmp_path, "explicit", {"o4": o4, "d4": d4})
    _check_records(a, info, so, o4, d4)


def test_size_query_cap_and_handle_reuse(tmp_path):
    a, info = _run(tmp_path, "sizes")
    rc0, rc1, rc2, rc3 = info["rc"]
    assert rc0 == 0 and rc1 == 0 and rc3 == 0
    total, t1, t2 = info["totals"]
    assert total > 0 and t1 == total and t2 == total
    assert a["query"].tobytes() == a["fill1"].tobytes() == a["fill3"].tobytes()
    assert np.array_equal(a["ids1"], a["ids3"])
    assert rc2 != 0 and str(total) in info["msg2"], info["msg2"]
    assert (a["small"] == 0xDEADBEEF).all(), "a too-small leaf_cap must leave leaf_ids untouched"
    assert_bits_equal(a["before"], a["after"], "render before / after a record call")
    assert info["rays"][0] == info["rays"][1]


def test_unsupported_scenes_and_modes(tmp_path):
    _, info = _run(tmp_path, "unsupported")
    for name in ("generic", "bvh", "fast"):
        assert info["codes"][name] == RTMI_ERR_UNSUPPORTED, (name, info["codes"][name], info["msgs"][name])
        assert info["msgs"][name], name
    assert "single leaf" in info["msgs"]["trivial"], info["msgs"]["trivial"]
    assert "analytic spheres" in info["msgs"]["spheres"], info["msgs"]["spheres"]
    for name, rays in info["renders"].items():
        assert rays > 0, name


def test_walk_rays_with_debug_en(tmp_path):
    a, info = _run(tmp_path, "debug_en")
    assert_bits_equal(a["off"], a["on"], "image with debug_en")
    assert info["rays"][0] == info["rays"][1]
    for k in [k[2:] for k in a if k.startswith("d_")]:
        assert a["d_" + k].tobytes() == a["r_" + k].tobytes(), k
    lines = info["csv"].splitlines()
    assert lines[0] == "Pixel_x;Pixel_y;ray_p;ray_v;tri_hit;hit_t;check_tris"
    assert len(lines) == 1 + 24 * 20
    assert lines[1].startswith("0;0;") and lines[-1].startswith("19;23;")
    assert "single leaf" in info["raised"], info["raised"]
    assert (a["untouched"] == 7.0).all(), "walk_rays rendered before it refused debug_en"
