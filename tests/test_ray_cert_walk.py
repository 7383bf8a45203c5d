"""-m gpu: the list walk of the sign certificate on the device (trace_oct.hpp: cert_walk in k_trace_oct's refill and, through
primary_ray_certified, in k_path_primary*_cull; DESIGN.md 4.1 "Sign certificate per ray", the list walk).
One fresh process per case renders a small frame with the fast and with the counting build and traces a fixed ray set; the
tests compare image bits and "Rays" with the oracle and the counting build's certificate counters with the host referee
(the entry-at-a-time loop, rtmi_debug_ray_cert_ref / rtmi_debug_ray_cull) wherever the host can make the same rays."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import assert_bits_equal, recipe_canonical

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NDBG = 52
# name -> (w, h, spp, seed): one pixel per wave -- its lanes walk the same list, mirror reflections are traced in place -- and
# four pixels per wave, whose cells and list lengths differ
CASES = {"packet": (16, 16, 64, 1), "mixed": (33, 33, 16, 2)}
DEPTH = 5
# What the host cannot regenerate -- the mirror reflections traced in place (dbg[45..46]: lanes certified, refused) and the
# bounce rays the frame's passes took (dbg[31..32]: taken with the cull on, refused) -- as the parent commit (17ad78e, the
# entry-at-a-time loop on the device) counted them for these frames: its librtmi.so under this file's _RUN,
#   python -c "$_RUN" <tree of 17ad78e> <this tests directory> out packet      (and mixed)
# and dbg[31], dbg[32], dbg[45], dbg[46] of out.json's "frame_c1".
PARENT = {"packet": {"bounce": (5301, 68), "inplace": (1290, 1)},
          "mixed": {"bounce": (5693, 86), "inplace": (1279, 0)}}


def fixed_rays():
    """4096 bounce-like rays (test_ray_cert_walk_cpu's recipe on the golden triangle records' scene): origins inside the
    scene, directions uniform, a quarter of them nearly perpendicular to a scene normal -> (o4, d4)"""
    z = np.load(os.path.join(ROOT, "tests", "golden", "canonical_triangle_records.npz"))
    rec = z["rec"].astype(np.float64)
    rng = np.random.default_rng(61)
    n = 4096
    d = rng.normal(size=(n, 3))
    k = rng.integers(0, len(rec), n // 4)
    nrm = rec[k, 3:6] / np.linalg.norm(rec[k, 3:6], axis=1, keepdims=True)
    d[:n // 4] = np.cross(nrm, d[:n // 4]) + nrm * rng.uniform(-3e-6, 3e-6, (n // 4, 1))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o4, d4 = np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32)
    o4[:, :3], d4[:, :3] = rng.uniform(-2.0, 2.0, (n, 3)), d
    return o4, d4


_RUN = r"""
import ctypes as C, json, os, sys
import numpy as np
import torch
root, tests, out, name = sys.argv[1], sys.argv[2], sys.argv[3], sys.argv[4]
sys.path.insert(0, root); sys.path.insert(0, tests)
from rust_raytrace_amd import raytrace as R, _ffi
from conftest import ProductApi, recipe_canonical
import test_ray_cert_walk as T
L = _ffi.lib()
L.rth_debug_counters_n.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
res, arrays = {}, {}

def dbg(sp):
    d = (C.c_ulonglong * T.NDBG)()
    L.rth_debug_counters_n(sp.h, d, T.NDBG)
    return [int(x) for x in d]

w, h, spp, seed = T.CASES[name]
for counting in (False, True):
    sp = recipe_canonical()(ProductApi(R))  # (a scene of its own per run: its counters start at 0)
    img = np.zeros((h, w, 4), np.float32)
    c = R.HipRayCaster(seed=seed, options=R.OPT_COUNTERS if counting else 0)
    ctx = c.walk_rays(R.canonical_viewport(w, h, T.DEPTH, spp), sp, img, 1, False)
    key = f"frame_c{int(counting)}"
    arrays[key] = img
    res[key] = {"total_rays": int(ctx.total_rays), "stats": {k: int(v) for k, v in ctx.stats.items() if isinstance(v, (int, np.integer))}}
    if counting:
        res[key]["dbg"] = dbg(sp)
if name == "packet":  # the fixed ray set, once: the counting build of k_trace_oct on caller-supplied rays
    sp = recipe_canonical()(ProductApi(R))
    o4, d4 = T.fixed_rays()
    n = len(o4)
    to, td = torch.from_numpy(o4).cuda(), torch.from_numpy(d4).cuda()
    tri, face = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")
    t = torch.zeros(n, device="cuda")
    R.HipRayCaster(options=R.OPT_COUNTERS).trace_device(sp, to, td, tri, t, face)
    torch.cuda.synchronize()
    res["trace"] = {"dbg": dbg(sp)}
    arrays["trace_tri"] = tri.cpu().numpy()
np.savez(out + ".npz", **arrays)
json.dump(res, open(out + ".json", "w"))
"""


def _run(tmp, name):
    env = dict(os.environ)
    for k in ("RTMI_PRIMARY_NODE_CULL", "RTMI_NODE_CULL", "RTMI_BLOCK_CULL", "RTMI_BLOCK_CULL_N", "RTMI_PACKET_CULL", "RTMI_MIRROR_INPLACE",
              "RTMI_CERT_G", "RTMI_REFILL_MIN", "RTMI_REFILL_MIN0"):
        env.pop(k, None)
    out = str(tmp / f"walk_{name}")
    subprocess.run([sys.executable, "-c", _RUN, ROOT, os.path.join(ROOT, "tests"), out, name], env=env, check=True, timeout=300)
    with open(out + ".json") as f:
        return dict(np.load(out + ".npz")), json.load(f)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("ray_cert_walk")
    return {name: _run(tmp, name) for name in CASES}


@pytest.fixture(scope="module")
def oracle():
    """(scene, name -> (image, counters)) of the oracle, rendered once"""
    from oracle import orc
    from conftest import OracleApi
    so = recipe_canonical()(OracleApi(orc))
    return so, {name: so.render(w, h, orc.canonical_viewport(w, h), DEPTH, spp, seed=seed, threads=8) for name, (w, h, spp, seed) in CASES.items()}


@pytest.fixture(scope="module")
def records(oracle):
    """the scene's plane records in the form the host referees take (record 0 the sentinel)"""
    raw, _, _ = oracle[0].triangles()
    recs = np.zeros((len(raw), 8), np.float32)
    recs[:, 0:3], recs[:, 3], recs[:, 4:7] = raw[:, 0:3], raw[:, 6], raw[:, 3:6]
    return recs


@pytest.mark.parametrize("name", list(CASES))
def test_frame_is_the_oracles(runs, oracle, name):
    """Fast build: image bits and "Rays" are the oracle's."""
    ref, cn = oracle[1][name]
    arrays, res = runs[name]
    assert_bits_equal(ref, arrays["frame_c0"], f"{name} vs the oracle")
    assert res["frame_c0"]["total_rays"] == cn["rays"], (res["frame_c0"]["total_rays"], cn["rays"])
    assert res["frame_c0"]["stats"]["pipeline"] == 3


@pytest.mark.parametrize("name", list(CASES))
def test_counting_build_counts_what_the_host_counts(runs, oracle, records, name):
    """Counting build: the image is the oracle's; the primary lanes certified / refused are the host referee's counts over
    the primary rays the oracle makes for this frame; reflections in place and the bounce passes' rays are what the parent
    commit counted; no hit inside a missed subtree, no culled block with a passing reference."""
    from oracle import orc
    from test_ray_cert_walk_cpu import ray_cert_ref
    w, h, spp, seed = CASES[name]
    ref, cn = oracle[1][name]
    arrays, res = runs[name]
    assert_bits_equal(ref, arrays["frame_c1"], f"{name} counting build vs the oracle")
    r = res["frame_c1"]
    assert r["total_rays"] == cn["rays"]
    d = r["dbg"]
    o4, d4 = orc.primary_rays(w, h, orc.canonical_viewport(w, h), spp, seed=seed)
    cert, _ = ray_cert_ref(records, np.concatenate([o4, d4], axis=1).astype(np.float32), 1024, 0.0)
    print(f"\n{name}: primary lanes certified {d[38]} refused {d[39]} (host {cert.sum()} / {(~cert).sum()}); in place {d[45]} / {d[46]}; "
          f"bounce rays {d[31]} refused {d[32]}; violations {d[30]} {d[37]} {d[44]} {d[51]}")
    assert r["stats"]["slow_paths"] == 0, "a primary ray left for the slow path: the host's count covers rays no lane took"
    assert (d[38], d[39]) == (int(cert.sum()), int((~cert).sum()))
    assert (d[45], d[46]) == PARENT[name]["inplace"]
    assert (d[31], d[32]) == PARENT[name]["bounce"]
    assert d[30] == 0 and d[37] == 0 and d[44] == 0 and d[51] == 0
    if name == "packet":
        assert d[45] > 0, "no mirror reflection was traced in place"


def test_caller_supplied_rays(runs, oracle, records):
    """4096 fixed rays through rtmi_trace_device, counting build: rays taken with the cull on and rays the certificate
    refused are rtmi_debug_ray_cull's counts on those rays; the hits are the oracle's."""
    from test_ray_cert_walk_cpu import table_and_cells
    o4, d4 = fixed_rays()
    arrays, res = runs["packet"]
    d = res["trace"]["dbg"]
    _, _, cert = table_and_cells(records, np.concatenate([o4, d4], axis=1), 1024, 0)
    print(f"\nfixed rays: taken {d[31]}, refused {d[32]} (host {(~cert).sum()})")
    assert 0 < (~cert).sum() < len(cert), "the fixed rays are all certified or all refused"
    assert (d[31], d[32]) == (len(o4), int((~cert).sum()))
    assert d[30] == 0 and d[37] == 0
    tri, _, _, _ = oracle[0].trace(o4, d4)
    assert np.array_equal(arrays["trace_tri"].view(np.uint32), tri)
