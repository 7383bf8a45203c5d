"""-m gpu: progressive rendering (rtmi_render_samples / rtmi_render_samples_device, HipRayCaster.walk_rays_progressive).
A frame rendered in sample passes [0,k1) [k1,k2) ... [kn,S) must end in the bits of one render call, and the preview after
k >= 2 samples in the bits of a render at spp = k (oracle).  Every case renders in a fresh process (case_* below); the parent
compares with the oracle and with the same process's single call."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ProductApi, assert_bits_equal, recipe_canonical, recipe_circles_analytic

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTERS = ("rays", "box_tests", "tri_tests", "full_tests", "nodes", "leaves")
W, H, S, DEPTH, SEED = 48, 40, 8, 5, 3
PASSES = [(0, 3), (3, 1), (4, 4)]  # (sample0, nsamples): [0,3) [3,4) [4,8)
# a raw viewport whose primary rays all have an exactly-zero x component: orig - cam, vu and vv have x = 0
SLOW_VP12 = [2.0, 0.6, 1.0, 2.0, 0.0, 0.0, 0.0, -1.2, 0.0, 0.0, 0.0, 0.5]

_RUN = r"""
import json, os, sys
import numpy as np
root, name, out = sys.argv[1], sys.argv[2], sys.argv[3]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
import test_progressive as T
arrays, info = getattr(T, "case_" + name)()
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


# ---------------------------------------------------------------- what the child processes run
def _product(kind):
    from rust_raytrace_amd import raytrace as R
    recipes = {"canonical": recipe_canonical(), "trivial": recipe_canonical(accel="trivial"), "analytic": recipe_circles_analytic()}
    return R, recipes[kind](ProductApi(R))


def _single_and_passes(kind, options=0, tuning=None, w=W, h=H, spp=S, passes=PASSES, vp12=None, depth=DEPTH):
    """One rtmi_render call, then the same frame in host passes (accum starts as NaN: sample0 == 0 must not read it)."""
    R, sp = _product(kind)
    vp = R.Viewport(w, h, vp12, depth, spp) if vp12 is not None else R.canonical_viewport(w, h, depth, spp)
    c = R.HipRayCaster(seed=SEED, options=options, tuning=tuning)
    single = np.zeros((h, w, 4), np.float32)
    ctx = c.walk_rays(vp, sp, single, 1, False)
    accum = np.full((h, w, 4), np.nan, np.float32)
    arrays, stats = {"single": single}, []
    for k0, n in passes:
        prev = np.zeros((h, w, 4), np.float32)
        p = c.walk_samples(vp, sp, 0, h, k0, n, accum, prev)
        arrays[f"prev{k0 + n}"] = prev
        stats.append(_ints(p.stats))
    arrays["accum"] = accum
    return arrays, {"single": _ints(ctx.stats), "passes": stats}


def case_canonical():
    return _single_and_passes("canonical")


def case_counters():
    from rust_raytrace_amd import raytrace as R
    return _single_and_passes("canonical", options=R.OPT_COUNTERS)


def case_pipeline1():
    return _single_and_passes("canonical", tuning={"pipeline": 1})


def case_trivial():
    return _single_and_passes("trivial")


def case_generic():
    from rust_raytrace_amd import raytrace as R
    return _single_and_passes("canonical", options=R.OPT_GENERIC)


def case_bvh():
    from rust_raytrace_amd import raytrace as R
    return _single_and_passes("canonical", options=R.OPT_BVH)


def case_analytic():
    return _single_and_passes("analytic")


def case_slow_path():
    return _single_and_passes("canonical", w=8, h=6, spp=4, passes=[(0, 1), (1, 3)], vp12=SLOW_VP12)


def case_spp1():
    return _single_and_passes("canonical", spp=1, passes=[(0, 1)])


def case_depth0():
    return _single_and_passes("canonical", w=16, h=8, passes=[(0, 5), (5, 3)], depth=0)


def case_device_tile():
    """Device variant on torch buffers and a caller stream: a striped tile over three internal streams with batches of a few
    hundred paths; out only on the last pass."""
    import torch
    R, sp = _product("canonical")
    vp = R.canonical_viewport(W, H, DEPTH, S)
    tile = (1, 16, 4, 8)  # rows 1-4, 9-12, 17-20, 25-28
    c = R.HipRayCaster(seed=SEED, tuning={"streams": 3, "batch_paths": 256, "subtile_min_paths": 1})
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    single = torch.zeros((16, W, 4), dtype=torch.float32, device=dev)
    accum = torch.full((16, W, 4), float("nan"), dtype=torch.float32, device=dev)
    out = torch.zeros((16, W, 4), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    ctx = c.walk_tile_device(vp, sp, tile, single.data_ptr(), stream.cuda_stream)
    stats = []
    for i, (k0, n) in enumerate(PASSES):
        last = i == len(PASSES) - 1
        p = c.walk_samples_device(vp, sp, tile, k0, n, accum.data_ptr(), out.data_ptr() if last else None, stream.cuda_stream)
        stats.append(_ints(p.stats))
    stream.synchronize()
    return ({"single": single.cpu().numpy(), "out": out.cpu().numpy(), "accum": accum.cpu().numpy()},
            {"single": _ints(ctx.stats), "passes": stats})


def case_progressive_api():
    R, sp = _product("canonical")
    vp = R.canonical_viewport(W, H, DEPTH, S)
    c = R.HipRayCaster(seed=SEED)
    ref = np.zeros((H, W, 4), np.float32)
    rc = c.walk_rays(vp, sp, ref, 1, False)
    full = np.zeros((H, W, 4), np.float32)
    seen = []
    ctx = c.walk_rays_progressive(vp, sp, full, pass_samples=3, on_pass=lambda k, cx: seen.append(k))
    stopped = np.zeros((H, W, 4), np.float32)
    ctx2 = c.walk_rays_progressive(vp, sp, stopped, pass_samples=3, on_pass=lambda k, cx: k < 6)
    return ({"ref": ref, "full": full, "stopped": stopped},
            {"ref_rays": int(rc.total_rays), "rays": int(ctx.total_rays), "done": ctx.samples_done, "seen": seen,
             "stopped_done": ctx2.samples_done, "stopped_rays": int(ctx2.total_rays)})


def case_misuse():
    """The raw ABI refuses a bad sample range and a NULL accumulator with a real scene handle, which stays usable."""
    import ctypes as C
    from oracle import orc
    import test_gpu_abi_raw as A
    L, ffi = A._lib()
    so = recipe_canonical()(__import__("conftest").OracleApi(orc))
    tris, geo, topo, refs = A._abi_arrays(so)
    rc, h = A._create(L, tris, A._boxes(geo, topo), refs)
    assert rc == 0, L.rtmi_last_error()
    vp12 = orc.canonical_viewport(16, 8)
    vp = A.Vp(16, 8, (C.c_float * 3)(*vp12[0:3]), (C.c_float * 3)(*vp12[3:6]), (C.c_float * 3)(*vp12[6:9]),
              (C.c_float * 3)(*vp12[9:12]), DEPTH, 4)
    acc = np.zeros((8, 16, 4), np.float32)
    out = np.zeros((8, 16, 4), np.float32)
    pa, po = acc.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    codes = {
        "over": L.rtmi_render_samples(h, C.byref(vp), SEED, 0, 8, 3, 2, pa, po, None),
        "zero": L.rtmi_render_samples(h, C.byref(vp), SEED, 0, 8, 0, 0, pa, po, None),
        "null_accum": L.rtmi_render_samples(h, C.byref(vp), SEED, 0, 8, 0, 4, None, po, None),
    }
    tile = ffi.Tile(0, 8, 8, 0)
    codes["device_null_accum"] = L.rtmi_render_samples_device(h, C.byref(vp), SEED, C.byref(tile), 0, 4, None, None, None, None)
    st = ffi.Stats()
    codes["ok0"] = L.rtmi_render_samples(h, C.byref(vp), SEED, 0, 8, 0, 2, pa, None, C.byref(st))
    codes["ok1"] = L.rtmi_render_samples(h, C.byref(vp), SEED, 0, 8, 2, 2, pa, po, C.byref(st))
    single, _ = A._render(L, ffi, h, vp12, 16, 8, DEPTH, 4, SEED)
    L.rtmi_scene_destroy(h)
    return {"out": out, "single": single}, {"codes": codes}


# ---------------------------------------------------------------- the checks (parent process)
def _oracle(spp, kind="canonical", w=W, h=H, vp12=None, seed=SEED):
    from oracle import orc
    from conftest import OracleApi
    so = {"canonical": recipe_canonical(), "trivial": recipe_canonical(accel="trivial")}[kind](OracleApi(orc))
    vo = orc.canonical_viewport(w, h) if vp12 is None else np.asarray(vp12, np.float32)
    return so.render(w, h, vo, DEPTH, spp, seed=seed, threads=8)


def _check_final(a, info, passes=PASSES):
    end = passes[-1][0] + passes[-1][1]
    assert_bits_equal(a[f"prev{end}"], a["single"], "final pass vs single call")
    assert_bits_equal(a["accum"] * (np.float32(1) / np.float32(end)), a["single"], "accum * (1/S) vs single call")
    assert sum(p["rays"] for p in info["passes"]) == info["single"]["rays"]


def test_canonical_passes_match_oracle_previews_and_rays(tmp_path):
    a, info = _run(tmp_path, "canonical")
    _check_final(a, info)
    cn_prev = {0: 0}
    for k0, n in PASSES:
        ref, cn = _oracle(k0 + n)
        assert_bits_equal(a[f"prev{k0 + n}"], ref, f"preview after {k0 + n} samples vs oracle spp={k0 + n}")
        cn_prev[k0 + n] = cn["rays"]
        assert info["passes"][PASSES.index((k0, n))]["rays"] == cn["rays"] - cn_prev[k0], f"rays of pass [{k0},{k0 + n})"
    assert info["single"]["rays"] == cn_prev[S]


def test_counters_sum_over_passes(tmp_path):
    a, info = _run(tmp_path, "counters")
    _check_final(a, info)
    for k in COUNTERS:
        assert sum(p[k] for p in info["passes"]) == info["single"][k], k
    assert info["single"]["box_tests"] > 0


@pytest.mark.parametrize("case,oracle_kind", [("pipeline1", "canonical"), ("trivial", "trivial"), ("generic", "canonical")])
def test_other_pipelines_match_oracle(tmp_path, case, oracle_kind):
    a, info = _run(tmp_path, case)
    _check_final(a, info)
    assert_bits_equal(a["single"], _oracle(S, oracle_kind)[0], f"{case}: single call vs oracle")
    if case == "pipeline1":
        assert {p["pipeline"] for p in info["passes"]} == {1}


@pytest.mark.parametrize("case", ["bvh", "analytic"])
def test_build_defined_modes_match_their_own_single_call(tmp_path, case):
    a, info = _run(tmp_path, case)
    _check_final(a, info)


def test_slow_path_passes(tmp_path):
    a, info = _run(tmp_path, "slow_path")
    _check_final(a, info, passes=[(0, 1), (1, 3)])
    for p in info["passes"]:
        assert p["slow_paths"] > 0 and p["pipeline"] == 3, p
    assert_bits_equal(a["prev4"], _oracle(4, w=8, h=6, vp12=SLOW_VP12)[0], "slow path: final vs oracle")


def test_one_sample_frame(tmp_path):
    a, info = _run(tmp_path, "spp1")
    _check_final(a, info, passes=[(0, 1)])
    assert_bits_equal(a["single"], _oracle(1)[0], "spp=1 vs oracle")


def test_depth_zero_writes_zeros(tmp_path):
    a, info = _run(tmp_path, "depth0")
    _check_final(a, info, passes=[(0, 5), (5, 3)])
    for k in ("prev5", "prev8", "accum"):
        assert_bits_equal(a[k], np.zeros((8, 16, 4), np.float32), k)
    assert all(p["rays"] == 0 for p in info["passes"])


def test_device_variant_striped_tile_on_a_caller_stream(tmp_path):
    a, info = _run(tmp_path, "device_tile")
    assert_bits_equal(a["out"], a["single"], "device passes vs walk_tile_device")
    assert sum(p["rays"] for p in info["passes"]) == info["single"]["rays"]
    assert info["single"]["streams"] == 3 and all(p["streams"] == 3 for p in info["passes"])
    ref = _oracle(S)[0]
    rows = [r for k in range(4) for r in range(1 + 8 * k, 5 + 8 * k)]
    assert_bits_equal(a["out"], ref[rows], "device passes vs oracle rows")


def test_walk_rays_progressive(tmp_path):
    a, info = _run(tmp_path, "progressive_api")
    assert_bits_equal(a["full"], a["ref"], "walk_rays_progressive vs walk_rays")
    assert info["seen"] == [3, 6, 8] and info["done"] == 8 and info["rays"] == info["ref_rays"]
    assert info["stopped_done"] == 6
    ref6, cn6 = _oracle(6)
    assert_bits_equal(a["stopped"], ref6, "stopped after 6 samples vs oracle spp=6")
    assert info["stopped_rays"] == cn6["rays"]


def test_misuse_is_refused_and_the_scene_stays_usable(tmp_path):
    a, info = _run(tmp_path, "misuse")
    c = info["codes"]
    assert c["over"] == 1 and c["zero"] == 1 and c["null_accum"] == 1 and c["device_null_accum"] == 1, c
    assert c["ok0"] == 0 and c["ok1"] == 0, c
    assert_bits_equal(a["out"], a["single"], "after refused calls")
