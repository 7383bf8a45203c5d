"""-m gpu: the four call families that trace shadow rays inside the bounce loop (rtmi_render_lit*, the same with RTMI_LIT_SURFACES,
rtmi_render_envlight*, rtmi_render_emissive*) on every trace variant launch_trace / launch_occluded can choose for their shadow
queue.  tests/shadow_matrix_cases.py holds the families (each with the scene, lights or lamps, sizes and reference of its own test
file), the rows and the recording hook; tests/test_shadow_matrix_cpu.py asserts every condition on the inputs from the references
alone.  Unless a row says otherwise it asserts: image and accum bit-identical to the reference, stats.rays = plain rays + live shadow
rays, pipeline == 1, the work counters > 0 exactly when counting, and the route it names, read from DCtrl::hyb of the main and of the
shadow workspace (rth_debug_hybrid_counters, rth_debug_shadow_hybrid_counters), so that a row cannot pass on another kernel.

Row                    shadow queue reaches (launch_occluded / launch_trace branch)            what shows it
default_counters       from_hits -> k_trace_oct<1,0>, then the hybrid into scratch +          counters = the oracle's sum over every traced
                       k_hybrid_referee                                                        batch; shadow offered > 0, violations == 0
default_route          from_hits -> the hybrid pass (k_hybrid_bvh, k_oct_verify,               shadow offered == the reference's live shadow
                       k_trace_oct_list)                                                       rays: the silent octree walk was not taken
generic(_counters)     !occluded_anyhit -> k_trace<0> / k_trace<1> + k_ao_occl_from_hits       offered == 0 on both; counters additive
                       (emissive: launch_trace alone)
hybrid_off_counters    RTMI_HYBRID=0: from_hits -> k_trace_oct<1,0>, no referee                offered == 0 on both; counters additive
anyhit                 RTMI_LIT_FROM_HITS=0: k_occluded_oct<0,0> / <1,0> with the lamps'       shadow offered == 0, main > 0; counters between
                       tmax and the nlights-wide queue                                         the plain call's and the closest-hit sum
linear_from_hits       list, RTMI_OCCLUDED_ANYHIT=0: k_trace_linear<1> +                       counters additive (tri_tests > 0, no boxes)
                       k_ao_occl_from_hits (for k_occluded_linear)
tune_* (six sets; lit  the hybrid pass under other waves, refills, XCD ranges, streams and    no bit, no ray changes; offered == live rays
and emissive only)     batches of 8 paths (queues below a wave)                                where a stream ran one batch
depth32                shadow queue index 31, 64 events per workspace, a direct-light stack    bits, rays, trace_launches % 64 == 0
                       of paths * 32
fast                   k_trace_oct<0,1> for paths and shadow rays                              own trace; offered == 0 on both
bvh                    k_trace_bvh<0> for both (emissive refuses RTMI_OPT_BVH)                 own trace; offered == 0 on both
"confirmed + fallbacks == offered" is asserted with the rays the BVH proved to hit nothing counted as confirmed (hyb[2]: an
unoccluded shadow ray is exactly that), which is test_hybrid.py's balance.

Exact rows expect the restatement over the oracle; fast and bvh expect the restatement with trace= pointed at the same handle's
rtmi_trace.  Rows with a creation-time switch run in a fresh child process.  One test runs the families in turn on one handle."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import conftest as CT
from conftest import assert_bits_equal
import emissive_cases as EC
import emissive_ref as EM
import env_ref as ER
import envlight_ref as EL
import lit_ref as LT
import shadow_matrix_cases as SM
import shadowed_ref as SR
from shadow_matrix_cases import CONFIRMED, FALLBACKS, F_BOUNDS, MISSES, OFFERED, VIOLATIONS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = SM.SEED
_SCENES = {}

_RUN = r"""
import json, os, sys
import numpy as np
root, fam, name, out = sys.argv[1:5]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
import shadow_matrix_cases as SM
arrays, info = SM.run_row(fam, name)
np.savez(out + ".npz", **arrays)
with open(out + ".json", "w") as f:
    json.dump(info, f)
"""


def _orc():
    from oracle import orc
    return orc


def _R():
    from rust_raytrace_amd import raytrace as R
    return R


def _child(tmp_path, fam, name):
    env = dict(os.environ)
    for k in ("RTMI_HYBRID", "RTMI_LIT_FROM_HITS", "RTMI_OCCLUDED_ANYHIT"):
        env.pop(k, None)
    env.update(SM.ROWS[name]["env"])
    out = str(tmp_path / f"{fam}_{name}")
    subprocess.run([sys.executable, "-c", _RUN, ROOT, fam, name, out], env=env, check=True, timeout=300)
    with open(out + ".json") as f:
        info = json.load(f)
    with np.load(out + ".npz") as z:
        return {k: z[k] for k in z.files}, info


@pytest.fixture(scope="module", autouse=True)
def _release_scenes():
    yield
    _SCENES.clear()


def _scene(fam, kind):
    """The family's product scene of `kind`, shared by the rows that run in this process"""
    if (fam, kind) not in _SCENES:
        _SCENES[fam, kind] = SM.FAMILIES[fam].product(kind)
    return _SCENES[fam, kind]


def _balance(d):
    """test_hybrid.py's: every ray offered is refused, missed, tied, confirmed or failed in the descent; the fallbacks are the rest"""
    failed = sum(d[SM.F_ABSENT:SM.F_NOTRI + 1]) + d[F_BOUNDS]
    assert d[OFFERED] == d[SM.REFUSED] + d[MISSES] + d[SM.TIES] + d[CONFIRMED] + failed, d
    assert d[FALLBACKS] == d[SM.REFUSED] + d[SM.TIES] + failed, d
    assert d[CONFIRMED] + d[MISSES] + d[FALLBACKS] == d[OFFERED], d
    assert d[VIOLATIONS] == 0 and d[F_BOUNDS] == 0, d


def _frame(what, arrays, key, r, ref, counting, work):
    """What every row asserts of one call: the bytes, the ray count, the pipeline, the counting kernels exactly when counting"""
    st = r["stats"]
    assert_bits_equal(arrays[key + "_image"], ref.image, f"{what}: image")
    assert_bits_equal(arrays[key + "_accum"], ref.accum, f"{what}: accum")
    assert st["rays"] == ref.rays + ref.nlive, f"{what}: rays {st['rays']} vs {ref.rays} + {ref.nlive}"
    assert st["pipeline"] == 1 and st["slow_paths"] == 0
    assert (st[work] > 0) == counting, (what, work, st[work])
    return st


@pytest.mark.parametrize("fam,name", SM.CASES, ids=[f"{f}-{r}" for f, r in SM.CASES])
def test_row(tmp_path, fam, name):
    R = _R()
    f, row = SM.FAMILIES[fam], SM.ROWS[name]
    kind = row.get("kind", "octree")
    k = f.size(kind)
    opts = row.get("opts", ())
    counting = "COUNTERS" in opts
    work = "tri_tests" if kind == "list" else "box_tests"  # a linear list has no boxes: its work is triangle tests
    what = f"{fam}, {name}"
    rec = None
    if row.get("env"):
        arrays, info = _child(tmp_path, fam, name)
        ref, rec = SM.expected(fam, kind)
    else:
        # (both readouts sum over every stream's control block, and a stream the last call did not use keeps its earlier one:
        # the row on four streams gets a scene of its own, so that the shared scene only ever ran on one)
        sp = f.product(kind) if row.get("tuning", {}).get("streams", 1) > 1 else _scene(fam, kind)
        try:
            arrays, info = SM.run_row(fam, name, sp)
            if row.get("own"):  # the restatement on the same handle's closest hits (rtmi_trace under the row's options)
                c = R.HipRayCaster(seed=SEED, options=SM.options_of(row))
                ref = f.render(kind, trace=lambda o4, d4: c.trace(sp, o4, d4)[:3])
            else:
                ref, rec = SM.expected(fam, kind)
        finally:
            if row.get("tuning"):
                R.HipRayCaster().upload(sp)  # back to the library's defaults for the rows that share the scene
    call = info["call"]
    st = _frame(what, arrays, "call", call, ref, counting, work)
    main, shadow, on = call["main"], call["shadow"], call["on"]
    one_batch = st["trace_launches"] == 2 * k["depth"] * st["streams"]  # (a path walk and a shadow walk per level)
    print(f"\n{what}: rays {st['rays']}, streams {st['streams']}, launches {st['trace_launches']}, on {on}, main hyb {main}, shadow hyb {shadow}, "
          + ", ".join(f"{n} {st[n]}" for n in SM.WORK))
    assert st["trace_launches"] % (2 * k["depth"]) == 0 and ref.nlive > 0

    def additive():
        for n in SM.WORK:
            assert st[n] == rec.counters[n], (what, n, st[n], rec.counters[n])

    if name == "default_counters":
        additive()
        assert on == 1 and main[OFFERED] > 0 and shadow[OFFERED] > 0
        _balance(main)
        _balance(shadow)
    elif name == "default_route":
        assert on == 1 and one_batch, st
        assert shadow[OFFERED] == ref.nlive, f"{what}: {shadow[OFFERED]} of {ref.nlive} shadow rays went to the hybrid pass"
        assert main[OFFERED] == ref.rays  # (the per-pass pipeline offers every path ray too)
        _balance(main)
        _balance(shadow)
    elif name in ("generic", "generic_counters", "hybrid_off_counters", "linear_from_hits"):
        if counting:
            additive()
        assert on == 0 and main == [0] * 12 and shadow == [0] * 12, (on, main, shadow)
    elif name == "anyhit":
        assert on == 1 and shadow == [0] * 12 and main[OFFERED] > 0, (on, main, shadow)
        cn = info["counting"]
        cst = _frame(what + ", counting", arrays, "counting", cn, ref, True, work)
        assert cn["shadow"] == [0] * 12 and cn["main"][OFFERED] > 0
        pst = info["plain"]["stats"]
        assert pst["rays"] == ref.rays and pst["pipeline"] == 1
        for n in SM.WORK:  # an any-hit walk stops early: no more work than the closest-hit walks, no less than the paths alone
            print(f"  {n}: plain {pst[n]} <= any-hit {cst[n]} <= closest-hit {rec.counters[n]}")
            assert pst[n] <= cst[n] <= rec.counters[n], (what, n, pst[n], cst[n], rec.counters[n])
    elif name.startswith("tune_"):
        assert on == 1
        _balance(main)
        _balance(shadow)
        assert st["streams"] == row["tuning"].get("streams", 1)
        if one_batch:
            assert shadow[OFFERED] == ref.nlive and main[OFFERED] > 0
        if name == "tune_small_batches":
            assert st["trace_launches"] >= 2 * k["depth"] * (k["w"] * k["h"] * k["spp"] // SM.batch_paths_of(SM.SMALL, k))
    elif name == "depth32":
        assert k["depth"] == 32 and st["trace_launches"] % 64 == 0
        assert on == 1 and one_batch and shadow[OFFERED] == ref.nlive and main[OFFERED] == ref.rays, (on, main, shadow)
        _balance(main)
        _balance(shadow)
    elif name in ("fast", "bvh"):
        assert on == 0 and main == [0] * 12 and shadow == [0] * 12, (on, main, shadow)
    else:
        raise AssertionError(f"row {name} has no checks")


def test_emissive_refuses_bvh_and_takes_fast():
    """RTMI_OPT_BVH is refused (tests/test_emissive.py holds the refusal's bytes); RTMI_OPT_FAST is taken: the row above passes,
    because path rays and shadow rays take the same trace and "the first hit is the lamp" is decided on the same hits"""
    R = _R()
    assert ("emissive", "fast") in SM.CASES and ("emissive", "bvh") not in SM.CASES
    sp = _scene("emissive", "octree")
    with pytest.raises(RuntimeError, match="RTMI_OPT_BVH"):
        R.HipRayCaster(seed=SEED, options=R.OPT_BVH).walk_rays_emissive(R.canonical_viewport(16, 16, 4, 1), sp)


def test_the_families_in_turn_on_one_handle():
    """ShadowBuf is shared by every family and rtmi_render_shadowed*, its buffers only grow, the fallback list is sized from the hit
    records at the time of the call, and setting or clearing the environment drops cached samplers: ten calls of changing family,
    size and depth on one scene, each bit-identical to its own reference"""
    R, orc = _R(), _orc()
    so, sp = CT.build_pair(EC.recipe_teapot_lamp())
    lamps = EC.TEAPOT_LAMPS
    sp.set_emitters(np.array(lamps))
    c = R.HipRayCaster(seed=SEED)
    AB = (LT.A, LT.B)
    sky = dict(table=ER.sky_table(16, SM.SUN), frame=None)
    from types import SimpleNamespace
    env = SimpleNamespace(**sky)

    def check(what, got, ref):
        img, ctx = got
        assert_bits_equal(img, ref.image, f"{what}: image")
        assert_bits_equal(ctx.accum, ref.accum, f"{what}: accum")
        assert ctx.stats["rays"] == ref.rays + ref.nlive and ctx.stats["pipeline"] == 1, (what, ctx.stats["rays"], ref.rays, ref.nlive)
        assert ref.nlive > 0
        return img.copy()

    def lit(w, h, spp, e=None):
        ref = LT.render(orc, so, orc.canonical_viewport(w, h), w, h, spp, SEED, 4, AB, env=e)
        return check(f"lit {w} x {h}", c.walk_rays_lit(R.canonical_viewport(w, h, 4, spp), sp, c.lit_params(AB)), ref)

    def emissive(w, h, depth, e=None):
        ref = EM.render(orc, so, orc.canonical_viewport(w, h), w, h, 4, SEED, depth, lamps, env=e)
        return check(f"emissive {w} x {h}", c.walk_rays_emissive(R.canonical_viewport(w, h, depth, 4), sp), ref)

    first = lit(32, 32, 4)
    emissive(48, 48, 3)
    ref = SR.shadowed_ref(orc, so, 40, 40, orc.canonical_viewport(40, 40), 4, 4, SEED, LT.A["orig"], 0.5)
    check("shadowed 40 x 40", c.walk_rays_shadowed(R.canonical_viewport(40, 40, 4, 4), sp, orig=LT.A["orig"], len2=0.5), ref)
    sp.set_sky(16, **SM.SUN)
    ref = EL.render(orc, so, orc.canonical_viewport(16, 16), 16, 16, 4, SEED, 4, env)
    check("envlight 16 x 16", c.walk_rays_envlight(R.canonical_viewport(16, 16, 4, 4), sp), ref)
    lit(33, 31, 3, env)
    emissive(32, 32, 4, env)
    sp.clear_environment()
    again = lit(32, 32, 4)
    assert_bits_equal(again, first, "the last lit frame against the first")
    img = np.zeros((32, 32, 4), np.float32)
    ctx = c.walk_rays(R.canonical_viewport(32, 32, 4, 4), sp, img, 1, False)
    want, cn = so.render(32, 32, orc.canonical_viewport(32, 32), 4, 4, seed=SEED)
    assert_bits_equal(img, want, "the plain frame against the oracle")
    assert ctx.total_rays == cn["rays"]
