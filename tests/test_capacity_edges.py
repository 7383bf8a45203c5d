"""-m gpu: the fixed capacities of the wavefront pipeline, reached by legal inputs and compared with the oracle bit for bit
(tests/capacity_cases.py has the inputs, tests/test_capacity_edges_cpu.py their preconditions).

A  The slow-path queue (RTMI_SLOW_CAP = 16 384 entries per stream and batch) at the cap, one past it and 4 096 past it: a
   refused primary ray is traced in place by k_path_primary, a refused bounce ray of k_path_primary goes to its in-place mirror
   packet or to queue 1 / 2, one of k_shade stays in the next pass's queue.  Every sampling mode (FRAME, PASS, LIST, VIEWS),
   two batches, two streams, both sides of the in-place threshold, the slow path off, pipeline 1, RTMI_OPT_FAST, and depth 32.
B  Depth 32 (RTMI_MAX_PASSES) through the path kernels without the slow path: 32 launches per stream in every mode.
C  65 535 distinct surfaces: ids above 255, above 32 767 and the top id through shade_hit's uint16_t stack and k_features.

Each case of A and B renders in a fresh process, without and with RTMI_OPT_COUNTERS; the palette scene of C is built once."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import capacity_cases as CC
from conftest import ProductApi, assert_bits_equal, recipe_axis_box
import shadowed_ref as SR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTERS, SEED, CAP = CC.COUNTERS, CC.SEED, CC.SLOW_CAP
SLOW_VP12 = CC.SLOW_VP12
RECIPES = {"discs": CC.recipe_mirror_discs, "axis_box": recipe_axis_box, "corridor": SR.recipe_corridor}

# name: scene, frame, tuning (streams = 1 unless the case is about streams: the frame is one batch on one stream), environment,
# and what the call's stats must say.  All under SLOW_VP12, seed 3.
FRAME_CASES = {
    "at_cap": dict(w=128, h=128, slow=CAP),
    "cap_plus_one": dict(w=113, h=145, slow=CAP),
    "over": dict(w=160, h=128, slow=CAP),
    "over_axis_box": dict(scene="axis_box", w=160, h=128, slow=CAP),
    "over_batches": dict(w=160, h=128, spp=2, tuning={"streams": 1, "batch_paths": 20480}, slow=2 * CAP),
    "over_streams": dict(w=160, h=256, tuning={"streams": 2, "subtile_min_paths": 1}, slow=2 * CAP, streams=2),
    "over_inplace_on": dict(w=160, h=128, slow=CAP, inplace=1),
    "over_inplace_off": dict(w=160, h=128, slow=CAP, inplace=64),
    "over_off": dict(w=160, h=128, tuning={"streams": 1, "slow_path_off": 1}, slow=0),
    "over_pipeline1": dict(w=160, h=128, tuning={"streams": 1, "pipeline": 1}, slow=0, pipeline=1),
    "over_depth32": dict(w=160, h=128, depth=32, slow=CAP),
}

_RUN = r"""
import json, os, sys
import numpy as np
root, fn, arg, out = sys.argv[1], sys.argv[2], sys.argv[3], sys.argv[4]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
import test_capacity_edges as T
arrays, info = getattr(T, "case_" + fn)(arg)
np.savez(out + ".npz", **arrays)
with open(out + ".json", "w") as f:
    json.dump(info, f)
"""


def _run(tmp_path, fn, arg="", env=None):
    out = str(tmp_path / f"{fn}_{arg}")
    e = dict(os.environ)
    e.pop("RTMI_MIRROR_INPLACE", None)
    e.update(env or {})
    subprocess.run([sys.executable, "-c", _RUN, ROOT, fn, arg, out], check=True, timeout=120, env=e)
    with open(out + ".json") as f:
        info = json.load(f)
    with np.load(out + ".npz") as z:
        return {k: z[k] for k in z.files}, info


def _stats(ctx):
    d = {k: int(v) for k, v in ctx.stats.items() if isinstance(v, (int, np.integer))}
    d["seconds"] = float(ctx.seconds)
    d["kernel_ms"] = float(ctx.stats["kernel_ms"])
    return d


def _full(c):
    return dict(scene=c.get("scene", "discs"), w=c["w"], h=c["h"], spp=c.get("spp", 1), depth=c.get("depth", 5))


# ---------------------------------------------------------------- what the child processes run
def _product(scene):
    from rust_raytrace_amd import raytrace as R
    return R, RECIPES[scene]()(ProductApi(R))


def _caster(R, counting, tuning=None, fast=False, seed=SEED):
    options = (R.OPT_COUNTERS if counting else 0) | (R.OPT_FAST if fast else 0)
    return R.HipRayCaster(seed=seed, options=options, tuning=tuning if tuning is not None else {"streams": 1})


def _dbg(sp):
    import ctypes as C
    from rust_raytrace_amd import _ffi
    L = _ffi.lib()
    L.rth_debug_counters_n.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    d = (C.c_ulonglong * 24)()
    L.rth_debug_counters_n(sp.h, d, 24)
    return [int(x) for x in d]


def case_frame(name):
    """One rtmi_render of the case's frame without and with the counters (the counting build's mirror statistics along)"""
    c = FRAME_CASES[name]
    f = _full(c)
    R, sp = _product(f["scene"])
    vp = R.Viewport(f["w"], f["h"], SLOW_VP12, f["depth"], f["spp"])
    arrays, info = {}, {}
    for counting in (0, 1):
        img = np.zeros((f["h"], f["w"], 4), np.float32)
        ctx = _caster(R, counting, c.get("tuning")).walk_rays(vp, sp, img, 1, False)
        arrays[f"img{counting}"] = img
        info[f"stats{counting}"] = _stats(ctx)
    info["dbg"] = _dbg(sp)
    return arrays, info


def case_modes(counting):
    """`over` in PASS, LIST and VIEWS, each on one stream"""
    counting = int(counting)
    R, sp = _product("discs")
    w, h = CC.OVER_W, CC.OVER_H
    arrays, info = {}, {}
    # PASS: passes [0,1) and [1,2) of a 2-spp frame (accum starts as NaN: sample0 == 0 must not read it)
    c = _caster(R, counting)
    vp = R.Viewport(w, h, SLOW_VP12, 5, 2)
    accum = np.full((h, w, 4), np.nan, np.float32)
    out = np.zeros((h, w, 4), np.float32)
    info["pass"] = [_stats(c.walk_samples(vp, sp, 0, h, k0, 1, accum, out)) for k0 in (0, 1)]
    arrays["pass_out"] = out
    # LIST: one pass of two samples, then one refinement pass that lists every pixel.  abs_tol = NaN is the tolerance at which
    # no pixel ever stops (include/rtmi.h); at rel = abs = 0 a pixel whose two samples agree (all of the sky) has a variance of
    # exactly 0 and stops, and the list of the rest stays below the cap: that run follows, held to the oracle per count.
    img = np.zeros((h, w, 4), np.float32)
    ctx = c.walk_rays_adaptive(R.Viewport(w, h, SLOW_VP12, 5, 3), sp, img, min_samples=2, pass_samples=1, rel_tol=0.0, abs_tol=float("nan"))
    arrays.update(list_img=img, list_counts=ctx.counts)
    info["list"] = dict(_stats(ctx), passes=ctx.passes, samples=int(ctx.samples))
    # ... and at abs_tol = 0: the pixels without variance stop at two samples, the others are listed
    img0 = np.zeros((h, w, 4), np.float32)
    ctx = c.walk_rays_adaptive(R.Viewport(w, h, SLOW_VP12, 5, 3), sp, img0, min_samples=2, pass_samples=1, rel_tol=0.0, abs_tol=0.0)
    arrays.update(list0_img=img0, list0_counts=ctx.counts)
    info["list0"] = dict(_stats(ctx), passes=ctx.passes, samples=int(ctx.samples))
    # VIEWS: two slow views of 160 x 64 (another seed each) and the canonical camera: 20 480 slow paths in the stacked batch
    c = _caster(R, counting)
    views = [R.Viewport(w, h // 2, SLOW_VP12, 5, 1), R.Viewport(w, h // 2, SLOW_VP12, 5, 1), R.canonical_viewport(w, h // 2, 5, 1)]
    ctx = c.walk_rays_views(views, sp, seeds=VIEW_SEEDS)
    arrays["views"] = ctx.data
    info["views"] = _stats(ctx)
    return arrays, info


VIEW_SEEDS = [3, 4, 5]


def case_fast(_):
    """`over` with RTMI_OPT_FAST, without and with the counters: FRAME with the slow path, FRAME without it, and PASS"""
    R, sp = _product("discs")
    w, h = CC.OVER_W, CC.OVER_H
    vp = R.Viewport(w, h, SLOW_VP12, 5, 2)
    arrays, info = {}, {}
    for counting in (0, 1):
        for name, tuning in (("on", {"streams": 1}), ("off", {"streams": 1, "slow_path_off": 1})):
            img = np.zeros((h, w, 4), np.float32)
            info[f"{name}{counting}"] = _stats(_caster(R, counting, tuning, fast=True).walk_rays(vp, sp, img, 1, False))
            arrays[f"{name}{counting}"] = img
        c = _caster(R, counting, fast=True)
        accum = np.full((h, w, 4), np.nan, np.float32)
        out = np.zeros((h, w, 4), np.float32)
        info[f"pass{counting}"] = [_stats(c.walk_samples(vp, sp, 0, h, k0, 1, accum, out)) for k0 in (0, 1)]
        arrays[f"pass_out{counting}"] = out
    return arrays, info


def case_corridor(counting):
    """Depth 32 in the corridor, 16 x 16 @ 2: rtmi_render on pipelines 3 and 1, PASS, LIST (three samples: the third is the
    listed pass), VIEWS (two seeds) and explicit rays"""
    from oracle import orc
    import rays_ref as RR
    counting = int(counting)
    R, sp = _product("corridor")
    g = CC.CORRIDOR
    w, h, spp, depth = g["w"], g["h"], g["spp"], g["maxdepth"]
    vp = R.canonical_viewport(w, h, depth, spp)
    arrays, info = {}, {}
    for pipeline in (3, 1):
        img = np.zeros((h, w, 4), np.float32)
        info[f"frame{pipeline}"] = _stats(_caster(R, counting, {"streams": 1, "pipeline": pipeline}).walk_rays(vp, sp, img, 1, False))
        arrays[f"frame{pipeline}"] = img
    c = _caster(R, counting)
    accum = np.full((h, w, 4), np.nan, np.float32)
    out = np.zeros((h, w, 4), np.float32)
    info["pass"] = [_stats(c.walk_samples(vp, sp, 0, h, k0, 1, accum, out)) for k0 in (0, 1)]
    arrays["pass_out"] = out
    img = np.zeros((h, w, 4), np.float32)
    ctx = c.walk_rays_adaptive(R.canonical_viewport(w, h, depth, 3), sp, img, min_samples=2, pass_samples=1, rel_tol=0.0, abs_tol=float("nan"))
    arrays.update(list_img=img, list_counts=ctx.counts)
    info["list"] = dict(_stats(ctx), passes=ctx.passes)
    ctx = c.walk_rays_views([vp, vp], sp, seeds=VIEW_SEEDS[:2])
    arrays["views"] = ctx.data
    info["views"] = _stats(ctx)
    o4, d4, keys = RR.camera_rays(orc, orc.canonical_viewport(w, h), w, h, spp, SEED)
    got, ctx = c.walk_rays_explicit(sp, o4, d4, depth, group=spp, keys=keys, color=False, mean=True)
    arrays["rays_mean"] = got["mean"].reshape(h, w, 4)
    info["rays"] = _stats(ctx)
    return arrays, info


# ---------------------------------------------------------------- the oracle (parent process)
@functools.lru_cache(maxsize=None)
def _oracle(scene, w, h, spp, depth, seed=SEED, view="slow"):
    from oracle import orc
    vo = np.asarray(SLOW_VP12, np.float32) if view == "slow" else orc.canonical_viewport(w, h)
    return CC.oracle_scene(scene).render(w, h, vo, depth, spp, seed=seed, threads=8)


def _check_exact(what, img, st, ref, cn, counting):
    assert_bits_equal(img, ref, f"{what}: image vs oracle")
    assert st["rays"] == cn["rays"], (what, "rays", st["rays"], cn["rays"])
    for k in COUNTERS if counting else ():
        assert st[k] == cn[k], (what, k, st[k], cn[k])
    if not counting:
        assert st["box_tests"] == 0, what


def _sum(cns):
    return {k: sum(c[k] for c in cns) for k in COUNTERS}


# ---------------------------------------------------------------- A
@pytest.mark.parametrize("name", list(FRAME_CASES))
def test_slow_queue_frames(tmp_path, name):
    """Image bits, "Rays" and (counting) all six work counters are the oracle's whether a zero-component ray was queued for
    k_path_slow or refused and traced where it was; slow_paths is min(attempts, cap) per stream and batch"""
    c = FRAME_CASES[name]
    f = _full(c)
    env = {"RTMI_MIRROR_INPLACE": str(c["inplace"])} if "inplace" in c else None
    a, info = _run(tmp_path, "frame", name, env)
    ref, cn = _oracle(f["scene"], f["w"], f["h"], f["spp"], f["depth"])
    if f["scene"] == "discs" and f["spp"] == 1:
        frame = [v for v in CC.FRAMES.values() if (v["w"], v["h"]) == (f["w"], f["h"])]
        if frame and "rays" in frame[0]:
            assert cn["rays"] == frame[0]["rays"][f["depth"]]
    for counting in (0, 1):
        st = info[f"stats{counting}"]
        _check_exact(f"{name}/{counting}", a[f"img{counting}"], st, ref, cn, counting)
        assert st["slow_paths"] == c["slow"], (name, counting, st["slow_paths"])
        assert st["pipeline"] == c.get("pipeline", 3) and st["streams"] == c.get("streams", 1), st
        if f["depth"] == 32:
            assert st["trace_launches"] == 32 * st["streams"]
        print(f"\n{name} counters={counting}: slow_paths {st['slow_paths']}, rays {st['rays']}, kernel {st['kernel_ms']:.1f} ms, "
              f"wall {st['seconds']:.3f} s")
    dbg = info["dbg"]  # the counting run's: [21] mirror reflections of primary rays that stayed with k_path_primary, [22] in place
    assert dbg[20] == 0, "packet cull violation"
    if name == "over_inplace_on":
        assert dbg[22] == dbg[21] > 0, dbg[21:23]    # threshold 1: every refused reflection is traced in place
    if name == "over_inplace_off":
        # threshold 64: a wave goes in place only when all 64 lanes hold a refused reflection at one exchange step (nm >= minpl,
        # trace_oct.hpp), which a frame may still contain, so [22] == 0 cannot be demanded; what the case needs is that
        # refused reflections exist and that some go to queue 1 and on to k_shade
        assert dbg[21] > 0 and dbg[21] > dbg[22], dbg[21:23]
    if name == "at_cap":
        assert dbg[21] == 0, dbg[21:23]              # every path is k_path_slow's from its first ray on: no bounce push


@pytest.mark.parametrize("counting", [0, 1])
def test_sampling_modes_over_the_cap(tmp_path, counting):
    """`over` through k_path_primary / k_path_slow of PASS, LIST and VIEWS: each batch that overflows reports 16 384 slow paths"""
    a, info = _run(tmp_path, "modes", str(counting))
    w, h = CC.OVER_W, CC.OVER_H
    # PASS
    ref2, cn2 = _oracle("discs", w, h, 2, 5)
    assert_bits_equal(a["pass_out"], ref2, "PASS: final frame vs oracle at 2 spp")
    for p in info["pass"]:
        assert p["slow_paths"] == CAP and p["pipeline"] == 3 and p["streams"] == 1, p
    for k in COUNTERS if counting else ("rays",):
        assert sum(p[k] for p in info["pass"]) == cn2[k], ("PASS", k)
    # LIST at NaN: two batches (the pass of two samples, the listed pass), each over the cap
    ref3, cn3 = _oracle("discs", w, h, 3, 5)
    lst = info["list"]
    assert (a["list_counts"] == 3).all() and lst["passes"] == 2 and lst["samples"] == 3 * w * h
    assert_bits_equal(a["list_img"], ref3, "LIST: every pixel at 3 samples vs oracle")
    assert lst["slow_paths"] == 2 * CAP and lst["pipeline"] == 3, lst
    for k in COUNTERS if counting else ("rays",):
        assert lst[k] == cn3[k], ("LIST", k, lst[k], cn3[k])
    # LIST at 0: every pixel is the oracle's at its own count
    counts = a["list0_counts"]
    assert 3 in counts and ((counts == 2) | (counts == 3)).all() and info["list0"]["samples"] == int(counts.sum())
    for n, ref in ((2, ref2), (3, ref3)):
        sel = counts == n
        assert_bits_equal(a["list0_img"][sel], ref[sel], f"LIST at 0: pixels with {n} samples vs oracle")
    assert info["list0"]["slow_paths"] >= CAP
    # VIEWS
    hv = h // 2
    refs = [_oracle("discs", w, hv, 1, 5, seed=VIEW_SEEDS[0]), _oracle("discs", w, hv, 1, 5, seed=VIEW_SEEDS[1]),
            _oracle("discs", w, hv, 1, 5, seed=VIEW_SEEDS[2], view="canonical")]
    for k, (ref, _) in enumerate(refs):
        assert_bits_equal(a["views"][k], ref, f"VIEWS: view {k} vs its oracle render")
    cnv = _sum([cn for _, cn in refs])
    assert info["views"]["slow_paths"] == CAP and info["views"]["pipeline"] == 3, info["views"]
    for k in COUNTERS if counting else ("rays",):
        assert info["views"][k] == cnv[k], ("VIEWS", k)
    print(f"\nmodes counters={counting}: PASS slow_paths {[p['slow_paths'] for p in info['pass']]}, LIST {lst['slow_paths']} "
          f"({lst['seconds']:.3f} s), LIST at 0 {info['list0']['slow_paths']}, VIEWS {info['views']['slow_paths']} "
          f"({info['views']['seconds']:.3f} s)")


def test_fast_mode_over_the_cap(tmp_path):
    """RTMI_OPT_FAST is compared as test_sampling_matrix.py compares it: with FAST's own frame only, never with the oracle's
    image.  FAST changes which boxes a ray visits, never how a ray's result or counts depend on the kernel that traces it: the
    frame with 16 384 paths queued and 4 096 refused equals the frame with the slow path off, PASS equals FRAME, and the
    uncounted kernels give the counted ones' bits and "Rays".  That the fast cell was taken shows as in that file: strictly
    fewer box tests or nodes than the exact walk (the oracle's counts, which `over` shows to be the product's); the camera
    sits inside the root box, so every ray has boxes wholly behind its origin to skip."""
    a, info = _run(tmp_path, "fast")
    for counting in (0, 1):
        on, off, passes = info[f"on{counting}"], info[f"off{counting}"], info[f"pass{counting}"]
        assert on["slow_paths"] == CAP and off["slow_paths"] == 0 and all(p["slow_paths"] == CAP for p in passes), counting
        assert on["pipeline"] == off["pipeline"] == 3
        assert_bits_equal(a[f"on{counting}"], a[f"off{counting}"], f"FAST/{counting}: slow path on vs off")
        assert_bits_equal(a[f"pass_out{counting}"], a[f"on{counting}"], f"FAST/{counting}: PASS vs FRAME")
        for k in COUNTERS if counting else ("rays",):
            assert on[k] == off[k] == sum(p[k] for p in passes), (counting, k)
        assert (on["box_tests"] > 0) == bool(counting)
    # the uncounted kernels against the counted ones
    for name in ("on", "off", "pass_out"):
        assert_bits_equal(a[name + "0"], a[name + "1"], f"FAST {name}: uncounted vs counted")
    assert info["on0"]["rays"] == info["on1"]["rays"] == info["off0"]["rays"]
    cn = _oracle("discs", CC.OVER_W, CC.OVER_H, 2, 5)[1]
    fast = info["on1"]
    assert fast["box_tests"] < cn["box_tests"] or fast["nodes"] < cn["nodes"], (fast, cn)
    print(f"\nfast: slow_paths {fast['slow_paths']}, rays {fast['rays']}, box tests {fast['box_tests']} (exact {cn['box_tests']}), "
          f"nodes {fast['nodes']} (exact {cn['nodes']}), kernel {info['on0']['kernel_ms']:.1f} ms, wall {info['on0']['seconds']:.3f} s")


# ---------------------------------------------------------------- B
@pytest.mark.parametrize("counting", [0, 1])
def test_depth_32_in_every_mode(tmp_path, counting):
    """The corridor keeps every path alive: 32 launches per stream, ctrl->count[] up to index 32, 64 pass events and a surface
    stack of 32 levels, in k_path_primary + 31 bounce passes (pipeline 3), the per-pass pipeline, PASS, LIST, VIEWS and
    rtmi_render_rays"""
    a, info = _run(tmp_path, "corridor", str(counting))
    g = CC.CORRIDOR
    w, h, spp, depth = g["w"], g["h"], g["spp"], g["maxdepth"]
    ref, cn = _oracle("corridor", w, h, spp, depth, view="canonical")
    assert cn["rays"] == 32 * w * h * spp
    for pipeline in (3, 1):
        st = info[f"frame{pipeline}"]
        _check_exact(f"pipeline {pipeline}", a[f"frame{pipeline}"], st, ref, cn, counting)
        assert st["pipeline"] == pipeline and st["trace_launches"] == 32 * st["streams"] and st["slow_paths"] == 0, st
    assert_bits_equal(a["pass_out"], ref, "PASS: final frame vs oracle")
    for k in COUNTERS if counting else ("rays",):
        assert sum(p[k] for p in info["pass"]) == cn[k], ("PASS", k)
    assert all(p["trace_launches"] == 32 * p["streams"] for p in info["pass"])
    ref3, cn3 = _oracle("corridor", w, h, 3, depth, view="canonical")
    assert (a["list_counts"] == 3).all() and info["list"]["passes"] == 2
    assert_bits_equal(a["list_img"], ref3, "LIST vs oracle at 3 spp")
    for k in COUNTERS if counting else ("rays",):
        assert info["list"][k] == cn3[k], ("LIST", k)
    assert info["list"]["trace_launches"] == 2 * 32 * info["list"]["streams"]
    refs = [_oracle("corridor", w, h, spp, depth, seed=s, view="canonical") for s in VIEW_SEEDS[:2]]
    for k, (r, _) in enumerate(refs):
        assert_bits_equal(a["views"][k], r, f"VIEWS: view {k}")
    cnv = _sum([c for _, c in refs])
    for k in COUNTERS if counting else ("rays",):
        assert info["views"][k] == cnv[k], ("VIEWS", k)
    assert info["views"]["trace_launches"] == 32 * info["views"]["streams"]
    assert_bits_equal(a["rays_mean"], ref, "explicit rays: mean vs oracle")
    for k in COUNTERS if counting else ("rays",):
        assert info["rays"][k] == cn[k], ("explicit rays", k)
    assert info["rays"]["trace_launches"] == 32
    print(f"\ncorridor counters={counting}: rays {cn['rays']}, pipeline 3 {info['frame3']['seconds']:.3f} s, pipeline 1 {info['frame1']['seconds']:.3f} s")


def test_render_refuses_depth_33():
    """rtmi_render reads its scene before it checks the depth, so this needs a live one (the other entry points' refusals
    are pinned without a GPU)"""
    from rust_raytrace_amd import raytrace as R
    sp = recipe_axis_box()(ProductApi(R))
    img = np.zeros((4, 4, 4), np.float32)
    for tuning in ({"pipeline": 3}, {"pipeline": 1}):
        with pytest.raises(RuntimeError, match="maxdepth"):
            R.HipRayCaster(seed=SEED, tuning=tuning).walk_rays(R.canonical_viewport(4, 4, 33, 1), sp, img, 1, False)
    R.HipRayCaster(seed=SEED).walk_rays(R.canonical_viewport(4, 4, 32, 1), sp, img, 1, False)


# ---------------------------------------------------------------- C
@pytest.fixture(scope="module")
def palette():
    """The palette scene on both sides and everything the oracle says about PALETTE_VIEW, built and computed once"""
    from types import SimpleNamespace
    from oracle import orc
    from rust_raytrace_amd import raytrace as R
    import features_ref as FR
    so = CC.oracle_scene("palette")
    sp = CC.recipe_palette()(ProductApi(R))
    ids, distinct = CC.surface_ids(so)
    assert distinct == CC.MAX_SURFACES
    v = CC.PALETTE_VIEW
    vo = CC.palette_viewport(orc)
    vp = R.create_viewport((v["w"], v["h"]), v["size"], v["pos"], R.unit(v["dir"]), v["fov"], v["roll"], v["maxdepth"], v["spp"])
    ref, cn = so.render(v["w"], v["h"], vo, v["maxdepth"], v["spp"], seed=SEED, threads=8)
    alb, nrm, hit, _ = FR.features_ref(orc, so, v["w"], v["h"], vo, v["spp"], SEED)
    o4, d4 = orc.primary_rays(v["w"], v["h"], vo, v["spp"], seed=SEED)
    tri, _, _, _ = so.trace(o4, d4)
    seen = set(ids[tri[tri != 0]].tolist())
    return SimpleNamespace(so=so, sp=sp, ids=ids, vp=vp, ref=ref, cn=cn, albedo=alb, normal=nrm, hit=hit, seen=seen)


@pytest.mark.parametrize("mode", ["pipeline3", "pipeline1", "pipeline3_counters", "generic"])
def test_palette_renders_with_65535_surfaces(palette, mode):
    """The scene is accepted at the limit, and paths whose surface stack holds ids above 32 767 at levels 0, 1 and 2 (a
    signed or truncated 16-bit id would pick another surface's colour and alpha) mix to the oracle's bits"""
    from rust_raytrace_amd import raytrace as R
    p, v = palette, CC.PALETTE_VIEW
    tuning = {"pipeline": 1} if mode == "pipeline1" else {"pipeline": 3} if mode.startswith("pipeline3") else None
    options = (R.OPT_COUNTERS if mode.endswith("counters") else 0) | (R.OPT_GENERIC if mode == "generic" else 0)
    img = np.zeros((v["h"], v["w"], 4), np.float32)
    ctx = R.HipRayCaster(seed=SEED, options=options, tuning=tuning).walk_rays(p.vp, p.sp, img, 1, False)
    assert_bits_equal(img, p.ref, f"{mode}: image vs oracle")
    assert ctx.total_rays == p.cn["rays"]
    assert ctx.stats["pipeline"] == (3 if mode.startswith("pipeline3") else 1)
    if mode.endswith("counters"):
        for k in COUNTERS:
            assert int(ctx.stats[k]) == p.cn[k], k


def test_palette_features_carry_the_high_ids(palette):
    """k_features: albedo (the surface's colour through its id) and the hit ids are features_ref's bits; the surface ids at
    the first hit include one above 255, one above 32 767 and the highest the view can see (65 513, pinned in
    capacity_cases.PALETTE_SEEN), and the product's own hit map names surfaces above 32 767"""
    from rust_raytrace_amd import raytrace as R
    p = palette
    galb, gnrm, gids, ctx = R.HipRayCaster(seed=SEED).walk_rays_features(p.vp, p.sp)
    assert_bits_equal(galb, p.albedo, "albedo")
    assert_bits_equal(gnrm, p.normal, "normal")
    assert np.array_equal(gids, p.hit), f"{int((gids != p.hit).sum())} hit ids differ"
    seen = p.seen
    assert any(255 < i <= 32767 for i in seen) and any(i > 32767 for i in seen)
    assert dict(distinct=len(seen), high=sum(1 for i in seen if i > 32767), lowest=min(seen), top=max(seen)) == CC.PALETTE_SEEN
    got = p.ids[(gids & 0x3FFFFFFF)[gids != 0]]
    assert (got > 32767).any() and got.max() <= CC.PALETTE_SEEN["top"]
