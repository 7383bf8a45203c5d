"""-m gpu: adaptive sampling at scale and at the edges of its schedule, and the three sampling modes on the full config-3 frame.

Compaction of the active list (k_adapt_count / k_adapt_scan / k_adapt_scatter) works in blocks of 256 entries, and
k_adapt_scan turns the block counts into offsets 256 blocks at a time with a carry between chunks.  The carry first matters
above 65 536 active pixels, so the scale case renders 1024 x 512 (2 048 blocks, 8 chunks) at a tolerance whose first
refinement list is longer than that.  At depth 2 only about 56 000 pixels of this view vary between samples (the rest are
sky or see the sky after one bounce), so no tolerance gets there; the case renders at depth 5 instead.

The config-3 case compares frame, progressive passes and adaptive passes at abs_tol = NaN on 2048 x 2048 @ 64 spp, whose
plans differ (a frame of 2^28 paths runs on one stream, a pass of 2^25 on three), exact and with RTMI_OPT_FAST.  FAST changes
some pixels of this frame, which makes its two path-kernel cells without counters visible.

Every case renders in a fresh process (case_* below); the parent compares with the float32 replay of test_adaptive and the
oracle."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import OracleApi, ProductApi, assert_bits_equal, recipe_canonical
from test_adaptive import TOLS, _ints, _sample_colours, pick_tol, replay

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 3
# the scale case
BW, BH, BS, BM, BP, BDEPTH = 1024, 512, 6, 2, 2, 5
BIG_TOLS = [(0.0, 0.002), (0.01, 0.002), (0.0, 0.001), (0.005, 0.001), (0.0, 0.004), (0.02, 0.004)]
ORACLE_ROWS = (0, 160, 256, 320, 450, 511)  # the teapot covers rows 146-497
# the schedule edges, 48 x 40, depth 5: name -> (S, m, p)
EDGES = {"m_is_s": (4, 4, 2), "last_pass_clamped": (7, 2, 3), "s2_m2": (2, 2, 1), "eight_passes": (9, 2, 1)}
EW, EH, EDEPTH = 48, 40, 5

_RUN = r"""
import json, os, sys
import numpy as np
root, name, out = sys.argv[1], sys.argv[2], sys.argv[3]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
import test_adaptive_scale as T
fn, _, arg = name.partition(":")
arrays, info = getattr(T, "case_" + fn)(*([arg] if arg else []))
np.savez(out + ".npz", **arrays)
with open(out + ".json", "w") as f:
    json.dump(info, f)
"""


def _run(tmp_path, name):
    out = str(tmp_path / name.replace(":", "_"))
    subprocess.run([sys.executable, "-c", _RUN, ROOT, name, out], check=True, timeout=900)
    with open(out + ".json") as f:
        info = json.load(f)
    with np.load(out + ".npz") as z:
        return {k: z[k] for k in z.files}, info


def _big_tol_ok(cols, rel, ab):
    """The first refinement list is longer than 256 blocks of 256 entries and pixels stop at every count."""
    counts, passes = replay(cols, BM, BP, rel, ab)[0::3]
    return int((counts > BM).sum()) > 65536 and set(np.unique(counts).tolist()) == {2, 4, 6} and passes == 3


def _one_pass_tol_ok(cols, m, p, rel, ab):
    """A one-pass schedule (m == S): some pixels stop at S and some do not."""
    counts, _, _, _, unconverged = replay(cols, m, p, rel, ab)
    return 0 < unconverged < counts.size


def _device_adaptive(c, vp, sp, w, h, m, p, rel, ab):
    import torch
    dev = torch.device("cuda", 0)
    bufs = {k: torch.full((h, w, 4), float("nan"), dtype=torch.float32, device=dev) for k in ("accum", "sumsq", "out")}
    cnt = torch.zeros((h, w), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    d = c.walk_adaptive_device(vp, sp, (0, h, h, 0), bufs["accum"].data_ptr(), bufs["sumsq"].data_ptr(), cnt.data_ptr(),
                               bufs["out"].data_ptr(), None, m, p, rel, ab)
    torch.cuda.synchronize()
    arrays = {k: t.cpu().numpy() for k, t in bufs.items()}
    arrays["counts"] = cnt.cpu().numpy().view(np.uint32)
    return arrays, {"passes": d.passes, "samples": int(d.samples), "unconverged": d.unconverged, "rays": int(d.total_rays),
                    "streams": d.stats["streams"]}


# ---------------------------------------------------------------- what the child processes run
def case_scale():
    """1024 x 512: the sample colours, the tolerance, the device variant with the default plan and with many small batches
    over three streams, and the frames at 2, 4 and 6 samples."""
    from rust_raytrace_amd import raytrace as R
    sp = recipe_canonical()(ProductApi(R))
    c = R.HipRayCaster(seed=SEED)
    cols = _sample_colours(c, R, sp, BW, BH, BS, None, BDEPTH)
    tol = next((t for t in BIG_TOLS if _big_tol_ok(cols, *t)), None)
    assert tol is not None, "no tolerance in BIG_TOLS puts more than 65536 pixels on the first refinement list"
    vp = R.canonical_viewport(BW, BH, BDEPTH, BS)
    arrays, info = {"cols": cols}, {"tol": list(tol)}
    for name, tuning in (("default", None), ("batches", {"streams": 3, "batch_paths": 4096, "subtile_min_paths": 1})):
        a, i = _device_adaptive(R.HipRayCaster(seed=SEED, tuning=tuning), vp, sp, BW, BH, BM, BP, *tol)
        arrays.update({f"{name}_{k}": v for k, v in a.items()})
        info[name] = i
    for n in (2, 4, 6):
        one = np.zeros((BH, BW, 4), np.float32)
        c.walk_rays(R.canonical_viewport(BW, BH, BDEPTH, n), sp, one, 1, False)
        arrays[f"frame{n}"] = one
    return arrays, info


def case_edge(name):
    from rust_raytrace_amd import raytrace as R
    spp, m, p = EDGES[name]
    sp = recipe_canonical()(ProductApi(R))
    c = R.HipRayCaster(seed=SEED)
    cols = _sample_colours(c, R, sp, EW, EH, spp, None, EDEPTH)
    if m == spp:
        tol = next(t for t in TOLS + [(0.0, float(x)) for x in np.geomspace(1e-4, 0.5, 40)] if _one_pass_tol_ok(cols, m, p, *t))
    else:
        tol = pick_tol(cols, m, p)
    arrays, info = _device_adaptive(c, R.canonical_viewport(EW, EH, EDEPTH, spp), sp, EW, EH, m, p, *tol)
    arrays["cols"] = cols
    info["tol"] = list(tol)
    return arrays, info


def case_config3():
    """2048 x 2048 @ 64 spp, depth 5, seed 1 on device buffers: frame, 8 passes of 8, adaptive at NaN with m = p = 8, exact
    and FAST.  The comparisons run on the device (int32 views); only their results come back."""
    import torch
    from rust_raytrace_amd import raytrace as R
    sp = recipe_canonical()(ProductApi(R))
    n, spp, depth, seed = 2048, 64, 5, 1
    vp = R.canonical_viewport(n, n, depth, spp)
    tile = (0, n, n, 0)
    dev = torch.device("cuda", 0)

    def buf():
        return torch.full((n, n, 4), float("nan"), dtype=torch.float32, device=dev)

    def differ(a, b):  # pixels with any differing bit
        return int((a.view(torch.int32) != b.view(torch.int32)).any(dim=2).sum().item())

    info, frames = {}, {}
    for mode, options in (("exact", 0), ("fast", R.OPT_FAST)):
        c = R.HipRayCaster(seed=seed, options=options)
        frame = buf()
        torch.cuda.synchronize()
        f = c.walk_tile_device(vp, sp, tile, frame.data_ptr())
        torch.cuda.synchronize()
        accum, out = buf(), buf()
        torch.cuda.synchronize()
        passes = []
        for k0 in range(0, spp, 8):
            p = c.walk_samples_device(vp, sp, tile, k0, 8, accum.data_ptr(), out.data_ptr() if k0 + 8 == spp else None)
            passes.append(_ints(p.stats))
        torch.cuda.synchronize()
        r = {"frame_rays": int(f.total_rays), "frame_streams": f.stats["streams"], "frame_pipeline": f.stats["pipeline"],
             "pass_rays": sum(p["rays"] for p in passes), "pass_streams": [p["streams"] for p in passes],
             "pass_vs_frame": differ(out, frame)}
        del accum, out
        acc, sq, aout = buf(), buf(), buf()
        cnt = torch.zeros((n, n), dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        d = c.walk_adaptive_device(vp, sp, tile, acc.data_ptr(), sq.data_ptr(), cnt.data_ptr(), aout.data_ptr(), None, 8, 8,
                                   0.0, float("nan"))
        torch.cuda.synchronize()
        r.update(adaptive_rays=int(d.total_rays), adaptive_passes=d.passes, adaptive_samples=int(d.samples),
                 adaptive_unconverged=d.unconverged, adaptive_counts_ok=bool((cnt == spp).all().item()),
                 adaptive_vs_frame=differ(aout, frame))
        del acc, sq, aout, cnt
        info[mode] = r
        frames[mode] = frame
    info["fast_vs_exact"] = differ(frames["fast"], frames["exact"])
    return {}, info


# ---------------------------------------------------------------- the checks (parent process)
@functools.lru_cache(maxsize=None)
def _oracle_scene():
    from oracle import orc
    return recipe_canonical()(OracleApi(orc))


def _oracle(w, h, depth, spp, row0=0, nrows=None):
    from oracle import orc
    return _oracle_scene().render(w, h, orc.canonical_viewport(w, h), depth, spp, seed=SEED, row0=row0, nrows=nrows, threads=8)


def _check_against_replay(a, info, m, p, prefix=""):
    rel, ab = info["tol"]
    counts, acc, sq, passes, unconverged = replay(a["cols"], m, p, rel, ab)
    assert np.array_equal(a[prefix + "counts"], counts), f"{prefix}: {int((a[prefix + 'counts'] != counts).sum())} counts differ from the replay"
    assert_bits_equal(a[prefix + "accum"], acc, f"{prefix}accum vs replay")
    assert_bits_equal(a[prefix + "sumsq"], sq, f"{prefix}sumsq vs replay")
    run = info[prefix[:-1]] if prefix else info
    assert (run["passes"], run["samples"], run["unconverged"]) == (passes, int(counts.sum()), unconverged), (run, passes, unconverged)
    return counts, passes, unconverged


def test_compaction_across_many_blocks(tmp_path):
    a, info = _run(tmp_path, "scale")
    rel, ab = info["tol"]
    counts, _, _, passes, unconverged = replay(a["cols"], BM, BP, rel, ab)
    # the premise: the first refinement list spans more than 256 compaction blocks, and pixels stop in every pass
    assert int((counts > BM).sum()) > 65536, int((counts > BM).sum())
    assert set(np.unique(counts).tolist()) == {2, 4, 6} and passes == 3
    for run in ("default", "batches"):
        _check_against_replay(a, info, BM, BP, run + "_")
        for n in (2, 4, 6):
            sel = counts == n
            assert_bits_equal(a[run + "_out"][sel], a[f"frame{n}"][sel], f"{run}: pixels with {n} samples vs the frame at {n}")
    assert info["batches"]["rays"] == info["default"]["rays"]
    assert info["batches"]["streams"] == 3
    # the frames themselves, on rows through the sky, the teapot and the disks
    for n in (2, 4, 6):
        for r in ORACLE_ROWS:
            ref, _ = _oracle(BW, BH, BDEPTH, n, row0=r, nrows=1)
            assert_bits_equal(a[f"frame{n}"][r:r + 1], ref, f"frame at {n} samples, row {r}, vs oracle")


@pytest.mark.parametrize("name", list(EDGES))
def test_schedule_edges(tmp_path, name):
    spp, m, p = EDGES[name]
    a, info = _run(tmp_path, "edge:" + name)
    counts, passes, unconverged = _check_against_replay(a, info, m, p)
    want_passes = 1 + -(-(spp - m) // p)
    assert passes == want_passes, (passes, want_passes)  # every pass ran: some pixel went on to S
    if m == spp:
        assert 0 < unconverged < EW * EH and (counts == spp).all()
    else:
        assert m in counts and spp in counts
    if name == "last_pass_clamped":
        assert set(np.unique(counts).tolist()) <= {2, 5, 7} and 5 in counts
    for n in np.unique(counts).tolist():
        sel = counts == n
        assert_bits_equal(a["out"][sel], _oracle(EW, EH, EDEPTH, n)[0][sel], f"pixels with {n} samples vs oracle")


def test_config3_modes_are_one_image(tmp_path):
    _, info = _run(tmp_path, "config3")
    npix = 2048 * 2048
    for mode in ("exact", "fast"):
        r = info[mode]
        # the plans differ: one stream for the frame's 2^28 paths, three for a pass's 2^25
        assert r["frame_streams"] == 1 and r["pass_streams"] == [3] * 8 and r["frame_pipeline"] == 3, (mode, r)
        assert r["pass_vs_frame"] == 0, (mode, "8 passes of 8 vs the frame", r["pass_vs_frame"])
        assert r["adaptive_vs_frame"] == 0, (mode, "adaptive at NaN vs the frame", r["adaptive_vs_frame"])
        assert r["adaptive_counts_ok"] and r["adaptive_passes"] == 8, (mode, r)
        assert r["adaptive_samples"] == 64 * npix and r["adaptive_unconverged"] == npix, (mode, r)
        assert r["frame_rays"] == r["pass_rays"] == r["adaptive_rays"], (mode, r)
    # FAST really differs on this frame (17 pixels when last measured), so the FAST path cells were the ones that ran
    assert info["fast_vs_exact"] >= 1, info["fast_vs_exact"]
