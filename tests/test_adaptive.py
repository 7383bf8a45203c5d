"""-m gpu: adaptive sampling (rtmi_render_adaptive / rtmi_render_adaptive_device, HipRayCaster.walk_rays_adaptive).
Every pixel stops at its own sample count and must equal, bit for bit, the pixel of a uniform render at that count
(oracle).  The count map and the sums of squares are checked against a numpy float32 replay of the whole schedule, built
from each sample's exact colour (a one-sample progressive pass on a zero accumulator leaves 0.f + c_k = c_k in it).  Every
case renders in a fresh process (case_* below); the parent compares."""
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
W, H, S, M, P, DEPTH, SEED = 48, 40, 16, 4, 4, 5, 3
# a raw viewport whose primary rays all have an exactly-zero x component (test_progressive.py): the slow path
SLOW_VP12 = [2.0, 0.6, 1.0, 2.0, 0.0, 0.0, 0.0, -1.2, 0.0, 0.0, 0.0, 0.5]
# tolerances the middle cases try in turn; the first whose replayed count map has m, S and a value between is used
TOLS = [(0.05, 0.01), (0.1, 0.01), (0.02, 0.005), (0.2, 0.02), (0.1, 0.05), (0.01, 0.002), (0.3, 0.05), (0.05, 0.1)]

_RUN = r"""
import json, os, sys
import numpy as np
root, name, out = sys.argv[1], sys.argv[2], sys.argv[3]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
import test_adaptive as T
arrays, info = getattr(T, "case_" + name)()
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


def _ints(stats):
    return {k: int(v) for k, v in stats.items() if isinstance(v, (int, np.integer))}


# ---------------------------------------------------------------- the schedule, replayed in numpy float32
def stop_rule(s, q, n, rel_tol, abs_tol):
    """include/rtmi.h's stop rule on (..., 4) float32 sums s and sums of squares q of n samples, in its f32 order."""
    f = np.float32
    with np.errstate(all="ignore"):
        inv = f(1) / f(n)
        m = s[..., :3] * inv
        v = (q[..., :3] - s[..., :3] * m) / f(n - 1)
        mx = lambda a, b: np.where(a < b, b, a)  # noqa: E731
        e = mx(mx(v[..., 0], v[..., 1]), v[..., 2]) / f(n)
        L = mx(mx(m[..., 0], m[..., 1]), m[..., 2])
        t = f(abs_tol) + f(rel_tol) * L
        nan = np.isnan(m).any(-1) | np.isnan(v).any(-1) | np.isnan(e) | np.isnan(t)
        return ~nan & (e <= t * t)


def replay(cols, m, p, rel_tol, abs_tol):
    """cols: (S, h, w, 4) float32, sample k's colour of every pixel.  Returns (counts, accum, sumsq, passes, unconverged):
    unconverged = the pixels still active at S whose stop rule fails there (rtmi_adaptive_t.unconverged)."""
    smax = cols.shape[0]
    acc = np.zeros(cols.shape[1:], np.float32)
    sq = np.zeros(cols.shape[1:], np.float32)
    counts = np.zeros(cols.shape[1:3], np.uint32)
    active = np.ones(cols.shape[1:3], bool)
    n, k, passes, unconverged = 0, m, 0, 0
    while True:
        for j in range(n, n + k):
            c = cols[j]
            acc = np.where(active[..., None], acc + c, acc)
            sq = np.where(active[..., None], sq + c * c, sq)
        n += k
        passes += 1
        counts[active] = n
        if n >= smax:
            unconverged = int((active & ~stop_rule(acc, sq, n, rel_tol, abs_tol)).sum())
            break
        active &= ~stop_rule(acc, sq, n, rel_tol, abs_tol)
        if not active.any():
            break
        k = min(p, smax - n)
    return counts, acc, sq, passes, unconverged


def pick_tol(cols, m, p):
    """The first of TOLS, then of a sweep of absolute tolerances, whose replayed count map has m, S and a value between."""
    for rel, ab in TOLS + [(0.0, float(x)) for x in np.geomspace(1e-4, 0.5, 40)]:
        counts = replay(cols, m, p, rel, ab)[0]
        u = set(np.unique(counts).tolist())
        if m in u and cols.shape[0] in u and len(u) >= 3:
            return rel, ab
    raise AssertionError("no tolerance gives a count map with m, S and a value between")


# ---------------------------------------------------------------- what the child processes run
def _product(kind):
    from rust_raytrace_amd import raytrace as R
    recipes = {"canonical": recipe_canonical(), "trivial": recipe_canonical(accel="trivial"), "analytic": recipe_circles_analytic()}
    return R, recipes[kind](ProductApi(R))


def _viewport(R, w, h, spp, vp12=None, depth=DEPTH):
    return R.Viewport(w, h, vp12, depth, spp) if vp12 is not None else R.canonical_viewport(w, h, depth, spp)


def _sample_colours(c, R, sp, w, h, spp, vp12=None, depth=DEPTH):
    """(spp, h, w, 4): sample k of every pixel, from one-sample progressive passes on a zero accumulator."""
    vp = _viewport(R, w, h, spp, vp12, depth)
    cols = np.zeros((spp, h, w, 4), np.float32)
    for k in range(spp):
        acc = np.zeros((h, w, 4), np.float32)
        c.walk_samples(vp, sp, 0, h, k, 1, acc)
        cols[k] = acc
    return cols


def _adaptive(kind, options=0, tuning=None, w=W, h=H, spp=S, m=M, p=P, rel=None, ab=None, vp12=None, depth=DEPTH,
              pick=False, singles=False):
    """walk_rays_adaptive; pick: the tolerance from TOLS (the sample colours come along); singles: the product's own
    uniform renders at every distinct count."""
    R, sp = _product(kind)
    c = R.HipRayCaster(seed=SEED, options=options, tuning=tuning)
    arrays, info = {}, {}
    if pick:
        cols = _sample_colours(c, R, sp, w, h, spp, vp12, depth)
        rel, ab = pick_tol(cols, m, p)
        arrays["cols"] = cols
    vp = _viewport(R, w, h, spp, vp12, depth)
    img = np.zeros((h, w, 4), np.float32)
    ctx = c.walk_rays_adaptive(vp, sp, img, min_samples=m, pass_samples=p, rel_tol=rel, abs_tol=ab)
    arrays.update(img=img, counts=ctx.counts)
    info.update(stats=_ints(ctx.stats), passes=ctx.passes, samples=int(ctx.samples), unconverged=ctx.unconverged, tol=[rel, ab])
    if singles:
        for n in np.unique(ctx.counts).tolist():
            one = np.zeros((h, w, 4), np.float32)
            c.walk_rays(_viewport(R, w, h, n, vp12, depth), sp, one, 1, False)
            arrays[f"single{n}"] = one
    return arrays, info


def case_nan():
    from rust_raytrace_amd import raytrace as R
    a, info = _adaptive("canonical", options=R.OPT_COUNTERS, ab=float("nan"), rel=0.0)
    R_, sp = _product("canonical")
    c = R.HipRayCaster(seed=SEED, options=R.OPT_COUNTERS)
    single = np.zeros((H, W, 4), np.float32)
    ctx = c.walk_rays(R.canonical_viewport(W, H, DEPTH, S), sp, single, 1, False)
    a["single"] = single
    info["single"] = _ints(ctx.stats)
    return a, info


def case_inf():
    return _adaptive("canonical", ab=float("inf"), rel=0.0)


def case_mid():
    """The picked tolerance through the device variant too: accum, sumsq, counts and out on torch buffers."""
    import torch
    a, info = _adaptive("canonical", pick=True)
    R, sp = _product("canonical")
    c = R.HipRayCaster(seed=SEED)
    dev = torch.device("cuda", 0)
    bufs = {k: torch.full((H, W, 4), float("nan"), dtype=torch.float32, device=dev) for k in ("accum", "sumsq", "out")}
    cnt = torch.zeros((H, W), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    rel, ab = info["tol"]
    d = c.walk_adaptive_device(R.canonical_viewport(W, H, DEPTH, S), sp, (0, H, H, 0), bufs["accum"].data_ptr(),
                               bufs["sumsq"].data_ptr(), cnt.data_ptr(), bufs["out"].data_ptr(), None, M, P, rel, ab)
    torch.cuda.synchronize()
    for k, t in bufs.items():
        a["dev_" + k] = t.cpu().numpy()
    a["dev_counts"] = cnt.cpu().numpy().view(np.uint32)
    info["dev"] = {"passes": d.passes, "samples": int(d.samples), "unconverged": d.unconverged, "rays": int(d.total_rays)}
    return a, info


def case_trivial():
    return _adaptive("trivial", pick=True)


def case_pipeline1():
    return _adaptive("canonical", tuning={"pipeline": 1}, pick=True)


def case_slow_path():
    return _adaptive("canonical", w=8, h=6, spp=6, m=2, p=1, vp12=SLOW_VP12, pick=True)


def case_bvh():
    from rust_raytrace_amd import raytrace as R
    return _adaptive("canonical", options=R.OPT_BVH, rel=0.05, ab=0.01, singles=True)


def case_analytic():
    return _adaptive("analytic", rel=0.05, ab=0.01, singles=True)


def case_depth0():
    return _adaptive("canonical", w=16, h=8, depth=0, rel=0.0, ab=float("nan"))


def case_device_tile():
    """Device variant on a striped tile and a caller stream, with one stream, three streams, and batches of 256 paths."""
    import torch
    R, sp = _product("canonical")
    vp = R.canonical_viewport(W, H, DEPTH, S)
    tile = (1, 16, 4, 8)  # rows 1-4, 9-12, 17-20, 25-28
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    arrays, info = {}, {}
    runs = {"one": {"streams": 1}, "three": {"streams": 3, "subtile_min_paths": 1},
            "small": {"streams": 3, "batch_paths": 256, "subtile_min_paths": 1}}
    for name, tuning in runs.items():
        c = R.HipRayCaster(seed=SEED, tuning=tuning)
        accum = torch.full((16, W, 4), float("nan"), dtype=torch.float32, device=dev)
        sumsq = torch.full((16, W, 4), float("nan"), dtype=torch.float32, device=dev)
        out = torch.zeros((16, W, 4), dtype=torch.float32, device=dev)
        cnt = torch.zeros((16, W), dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        d = c.walk_adaptive_device(vp, sp, tile, accum.data_ptr(), sumsq.data_ptr(), cnt.data_ptr(), out.data_ptr(),
                                   stream.cuda_stream, M, P, 0.05, 0.01)
        stream.synchronize()
        arrays[name + "_out"] = out.cpu().numpy()
        arrays[name + "_counts"] = cnt.cpu().numpy().view(np.uint32)
        arrays[name + "_sumsq"] = sumsq.cpu().numpy()
        info[name] = {"passes": d.passes, "samples": int(d.samples), "rays": int(d.total_rays), "streams": d.stats["streams"]}
    full = np.zeros((H, W, 4), np.float32)
    ctx = R.HipRayCaster(seed=SEED).walk_rays_adaptive(vp, sp, full, min_samples=M, pass_samples=P, rel_tol=0.05, abs_tol=0.01)
    arrays["full"], arrays["full_counts"] = full, ctx.counts
    return arrays, info


def case_misuse():
    """The raw ABI refuses bad adaptive arguments with a real scene handle, which stays usable."""
    import ctypes as C
    from oracle import orc
    import test_gpu_abi_raw as A
    L, ffi = A._lib()
    so = recipe_canonical()(__import__("conftest").OracleApi(orc))
    tris, geo, topo, refs = A._abi_arrays(so)
    rc, h = A._create(L, tris, A._boxes(geo, topo), refs)
    assert rc == 0, L.rtmi_last_error()
    vp12 = orc.canonical_viewport(16, 8)

    def vp(spp):
        return A.Vp(16, 8, (C.c_float * 3)(*vp12[0:3]), (C.c_float * 3)(*vp12[3:6]), (C.c_float * 3)(*vp12[6:9]),
                    (C.c_float * 3)(*vp12[9:12]), DEPTH, spp)
    out = np.zeros((8, 16, 4), np.float32)
    cnt = np.zeros((8, 16), np.uint32)
    po, pc = out.ctypes.data_as(C.c_void_p), cnt.ctypes.data_as(C.c_void_p)
    nan = float("nan")
    codes = {}
    for name, spp, m, p in (("m1", 4, 1, 2), ("m_over", 4, 5, 2), ("p0", 4, 2, 0), ("s1", 1, 1, 1)):
        ad = ffi.Adaptive(m, p, 0.0, nan)
        codes[name] = L.rtmi_render_adaptive(h, C.byref(vp(spp)), SEED, 0, 8, C.byref(ad), po, pc, None)
    ad = ffi.Adaptive(2, 2, 0.0, nan)
    codes["null_out"] = L.rtmi_render_adaptive(h, C.byref(vp(4)), SEED, 0, 8, C.byref(ad), None, pc, None)
    codes["alias"] = L.rtmi_render_adaptive(h, C.byref(vp(4)), SEED, 0, 8, C.byref(ad), po, po, None)
    codes["null_ad"] = L.rtmi_render_adaptive(h, C.byref(vp(4)), SEED, 0, 8, None, po, pc, None)
    tile = ffi.Tile(0, 8, 8, 0)
    b = C.c_void_p(4096)
    codes["device_alias"] = L.rtmi_render_adaptive_device(h, C.byref(vp(4)), SEED, C.byref(tile), C.byref(ad), b, C.c_void_p(8192), b,
                                                          None, None, None)
    st = ffi.Stats()
    codes["ok"] = L.rtmi_render_adaptive(h, C.byref(vp(4)), SEED, 0, 8, C.byref(ad), po, pc, C.byref(st))
    single, _ = A._render(L, ffi, h, vp12, 16, 8, DEPTH, 4, SEED)
    L.rtmi_scene_destroy(h)
    return {"out": out, "counts": cnt, "single": single}, {"codes": codes, "passes": ad.passes}


# ---------------------------------------------------------------- the checks (parent process)
def _oracle(spp, kind="canonical", w=W, h=H, vp12=None, depth=DEPTH):
    from oracle import orc
    from conftest import OracleApi
    so = {"canonical": recipe_canonical(), "trivial": recipe_canonical(accel="trivial")}[kind](OracleApi(orc))
    vo = orc.canonical_viewport(w, h) if vp12 is None else np.asarray(vp12, np.float32)
    return so.render(w, h, vo, depth, spp, seed=SEED, threads=8)


def _check_per_count(img, counts, refs, what):
    """Every pixel equals refs[count] at that pixel."""
    for n in np.unique(counts).tolist():
        sel = counts == n
        assert_bits_equal(img[sel], refs(n)[sel], f"{what}: pixels with {n} samples")


def _check_replay(a, info, m, p):
    rel, ab = info["tol"]
    counts, acc, sq, passes, unconverged = replay(a["cols"], m, p, rel, ab)
    assert np.array_equal(a["counts"], counts), "count map vs the float32 replay"
    assert info["passes"] == passes and info["samples"] == int(counts.sum())
    assert info["unconverged"] == unconverged, (info["unconverged"], unconverged)
    return counts, acc, sq


def test_nan_tolerance_is_the_uniform_render(tmp_path):
    a, info = _run(tmp_path, "nan")
    assert_bits_equal(a["img"], a["single"], "abs_tol = NaN vs rtmi_render")
    assert_bits_equal(a["img"], _oracle(S)[0], "abs_tol = NaN vs oracle")
    assert (a["counts"] == S).all()
    assert info["passes"] == 1 + (S - M) // P and info["samples"] == S * W * H and info["unconverged"] == W * H
    for k in COUNTERS:
        assert info["stats"][k] == info["single"][k], k
    assert info["single"]["box_tests"] > 0


def test_infinite_tolerance_stops_every_pixel_at_min_samples(tmp_path):
    a, info = _run(tmp_path, "inf")
    ref, cn = _oracle(M)
    assert_bits_equal(a["img"], ref, "abs_tol = +inf vs oracle spp = m")
    assert (a["counts"] == M).all() and info["passes"] == 1 and info["unconverged"] == 0
    assert info["stats"]["rays"] == cn["rays"]


def test_middle_tolerance_every_pixel_exact_at_its_count(tmp_path):
    a, info = _run(tmp_path, "mid")
    counts, acc, sq = _check_replay(a, info, M, P)
    u = np.unique(counts).tolist()
    assert M in u and S in u and len(u) >= 3, u
    _check_per_count(a["img"], counts, lambda n: _oracle(n)[0], "host variant vs oracle")
    assert info["unconverged"] == 0 or S in u
    # the device variant: same schedule, and its running sums are the replay's bits
    assert np.array_equal(a["dev_counts"], counts)
    assert_bits_equal(a["dev_out"], a["img"], "device variant vs host variant")
    assert_bits_equal(a["dev_accum"], acc, "accum vs replay")
    assert_bits_equal(a["dev_sumsq"], sq, "sumsq vs replay")
    assert (a["dev_sumsq"][..., 3] == 0).all()
    assert info["dev"]["passes"] == info["passes"] and info["dev"]["samples"] == info["samples"]
    assert info["dev"]["unconverged"] == info["unconverged"]
    assert info["dev"]["rays"] == info["stats"]["rays"]


@pytest.mark.parametrize("case,oracle_kind", [("trivial", "trivial"), ("pipeline1", "canonical")])
def test_other_pipelines_match_oracle_at_their_counts(tmp_path, case, oracle_kind):
    a, info = _run(tmp_path, case)
    counts = _check_replay(a, info, M, P)[0]
    _check_per_count(a["img"], counts, lambda n: _oracle(n, oracle_kind)[0], case)
    if case == "pipeline1":
        assert info["stats"]["pipeline"] == 1


def test_slow_path_adaptive(tmp_path):
    a, info = _run(tmp_path, "slow_path")
    counts = _check_replay(a, info, 2, 1)[0]
    assert info["stats"]["slow_paths"] > 0 and info["stats"]["pipeline"] == 3, info["stats"]
    _check_per_count(a["img"], counts, lambda n: _oracle(n, w=8, h=6, vp12=SLOW_VP12)[0], "slow path")


@pytest.mark.parametrize("case", ["bvh", "analytic"])
def test_build_defined_modes_match_their_own_single_calls(tmp_path, case):
    a, info = _run(tmp_path, case)
    _check_per_count(a["img"], a["counts"], lambda n: a[f"single{n}"], case)
    assert info["samples"] == int(a["counts"].sum())


def test_depth_zero(tmp_path):
    a, info = _run(tmp_path, "depth0")
    assert_bits_equal(a["img"], np.zeros((8, 16, 4), np.float32), "depth 0")
    assert (a["counts"] == M).all() and info["stats"]["rays"] == 0 and info["samples"] == M * 16 * 8


def test_device_variant_streams_and_batches(tmp_path):
    a, info = _run(tmp_path, "device_tile")
    rows = [r for k in range(4) for r in range(1 + 8 * k, 5 + 8 * k)]
    assert info["one"]["streams"] == 1 and info["three"]["streams"] == 3
    for name in ("one", "three", "small"):
        assert_bits_equal(a[name + "_out"], a["full"][rows], f"{name}: tile vs the full-frame host variant")
        assert np.array_equal(a[name + "_counts"], a["full_counts"][rows]), name
        assert_bits_equal(a[name + "_sumsq"], a["one_sumsq"], f"{name}: sumsq")
        assert info[name]["rays"] == info["one"]["rays"] and info[name]["samples"] == info["one"]["samples"], name
    assert len(np.unique(a["one_counts"])) >= 2


def test_misuse_is_refused_and_the_scene_stays_usable(tmp_path):
    a, info = _run(tmp_path, "misuse")
    c = info["codes"]
    for k in ("m1", "m_over", "p0", "s1", "null_out", "alias", "null_ad", "device_alias"):
        assert c[k] == 1, (k, c)
    assert c["ok"] == 0, c
    assert_bits_equal(a["out"], a["single"], "abs_tol = NaN after refused calls vs rtmi_render")
    assert (a["counts"] == 4).all() and info["passes"] == 2
