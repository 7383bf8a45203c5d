"""-m "not gpu": the conditions tests/test_shadow_matrix.py relies on, from the references alone (tests/shadow_matrix_cases.py): the
recording hook changes no bit, its sums are the oracle's own frame counters, every family has live shadow rays of both outcomes
whose walks cost box and triangle tests, the depth-32 scene keeps paths and shadow rays alive to the last level, and the small-batch
tuning puts fewer rays than a wave into a shadow queue.  A failing condition here means the inputs were chosen wrongly, not that a
kernel is wrong.  Every figure is printed (pytest -s shows them)."""
import numpy as np
import pytest

from conftest import assert_bits_equal
import shadow_matrix_cases as SM

FAMS = list(SM.FAMILIES)


def _orc():
    from oracle import orc
    return orc


def _shadow_work(fam, kind):
    """The recorded work of the shadow rays alone: the hooked reference's sums less those of the same paths without shadow rays"""
    f = SM.FAMILIES[fam]
    ref, rec = SM.expected(fam, kind)
    plain_rec = SM.Recorder(f.oracle(kind)[0])
    plain = f.render(kind, trace=plain_rec, plain=True)
    assert plain.rays == ref.rays == plain_rec.rays, "the shadow rays changed the paths"
    return {k: rec.counters[k] - plain_rec.counters[k] for k in SM.WORK}, rec.rays - plain_rec.rays


@pytest.mark.parametrize("fam", FAMS)
def test_the_hook_changes_no_bit(fam):
    f = SM.FAMILIES[fam]
    bare = f.render("octree")
    ref, rec = SM.expected(fam, "octree")
    assert_bits_equal(ref.image, bare.image, f"{fam}: image with the hook")
    assert_bits_equal(ref.accum, bare.accum, f"{fam}: accum with the hook")
    assert (ref.rays, ref.nlive) == (bare.rays, bare.nlive)
    # the hook saw every path ray and every live shadow ray, and nothing else: stats.rays of the call
    assert rec.rays == rec.oracle_rays == ref.rays + ref.nlive, (rec.rays, rec.oracle_rays, ref.rays, ref.nlive)
    print(f"\n{fam}: {rec.batches} traced batches, {rec.rays} rays = {ref.rays} path + {ref.nlive} shadow")


def test_the_hooks_sums_are_the_oracles_frame_counters():
    """lit without lights is the plain frame: the sum over the traced batches equals Scene.render's counters of the same frame,
    which anchors "sum over traced batches" to the oracle's own frame total"""
    orc = _orc()
    f, k = SM.FAMILIES["lit"], SM.DEFAULT
    so = f.oracle("octree")[0]
    rec = SM.Recorder(so)
    ref = f.render("octree", trace=rec, plain=True)
    img, cn = so.render(k["w"], k["h"], orc.canonical_viewport(k["w"], k["h"]), k["depth"], k["spp"], seed=SM.SEED)
    assert_bits_equal(ref.image, img, "lit without lights against Scene.render")
    assert rec.rays == cn["rays"] == ref.rays
    for name in SM.WORK:
        assert rec.counters[name] == cn[name], (name, rec.counters[name], cn[name])
    print(f"\nanchor: rays {cn['rays']}, " + ", ".join(f"{n} {cn[n]}" for n in SM.WORK))


@pytest.mark.parametrize("fam", FAMS)
def test_live_shadow_rays_of_both_outcomes_that_cost_work(fam):
    f = SM.FAMILIES[fam]
    ref, rec = SM.expected(fam, "octree")
    live, blocked = f.levels(ref)
    work, nrays = _shadow_work(fam, "octree")
    print(f"\n{fam} (octree, default size): live {sum(live)} per level {live}, occluded {sum(blocked)}, unoccluded {sum(live) - sum(blocked)}; "
          f"shadow rays' work " + ", ".join(f"{k} {v}" for k, v in work.items()))
    assert sum(live) == ref.nlive == nrays > 100
    assert sum(blocked) > 0 and sum(live) - sum(blocked) > 0
    assert work["box_tests"] > 0 and work["tri_tests"] > 0, work
    assert live[-1] == 0, "the exhausted level gets no sample"


@pytest.mark.parametrize("fam", ["lit", "lit_surf", "envlight"])
def test_linear_list_scenes_have_live_shadow_rays(fam):
    f = SM.FAMILIES[fam]
    ref, rec = SM.expected(fam, "list")
    live, blocked = f.levels(ref)
    work, nrays = _shadow_work(fam, "list")
    print(f"\n{fam} (linear list): live {sum(live)}, occluded {sum(blocked)}; shadow rays' work " + ", ".join(f"{k} {v}" for k, v in work.items()))
    assert sum(live) == nrays > 50 and sum(blocked) > 0
    assert work["tri_tests"] > 0, work  # (a list has no boxes: its work is triangle tests)


@pytest.mark.parametrize("fam", FAMS)
def test_depth_32_scene_is_alive_to_the_last_level(fam):
    f, k = SM.FAMILIES[fam], SM.DEEP
    assert (k["w"], k["h"], k["spp"], k["depth"]) == (16, 16, 1, 32)
    ref, rec = SM.expected(fam, "deep")
    live, _ = f.levels(ref)
    print(f"\n{fam} (matte corridor, depth 32): paths in pass 31: {ref.passes[31]} of {ref.passes[0]}; live shadow rays at level 30: {live[30]}, "
          f"in all {sum(live)}; rays {ref.rays}")
    assert len(ref.passes) == 32 and ref.passes[31] > 0
    assert live[30] > 0 and live[31] == 0
    assert all(x > 0 for x in live[:31]), live


@pytest.mark.parametrize("fam", SM.TUNED)
def test_small_batch_tuning_leaves_a_shadow_queue_below_a_wave(fam):
    """plan_tile's split restated: under streams=4, batch_paths=40 a batch holds two pixels.  The batches of stream 1 (rows 1, 5,
    ...) are traced one by one on their own primary rays until one shows a level whose shadow queue holds between 1 and 63 rays;
    the per-level sums over every batch of one image row are the row's own."""
    f, k = SM.FAMILIES[fam], SM.DEFAULT
    bp = SM.batch_paths_of(SM.SMALL, k)
    ref, _ = SM.expected(fam, "octree")
    live, _ = f.levels(ref)
    nbatches = -(-k["w"] * k["h"] * k["spp"] // bp)
    assert bp == 8 and 1 <= bp * f.per_path <= 63 and nbatches > 4 * SM.SMALL["streams"]
    per_row = k["w"] * k["spp"] // bp
    shown, row_sum = None, np.zeros(k["depth"], np.int64)
    for b in range(3 * per_row, 4 * per_row):  # stream 1's fourth row, image row 13: across the teapot
        lv, npaths = SM.batch_levels(fam, "octree", SM.SMALL, 1, b)
        assert npaths == bp
        row_sum += np.array(lv)
        if shown is None and any(1 <= x <= 63 for x in lv):
            shown = (b, lv)
    assert shown is not None, "no batch of that row has a shadow queue of 1 .. 63 rays"
    # the same row as one tile of the family's reference: the batches' queues add up to it
    pix = np.concatenate([SM.batch_pixels(SM.SMALL, k, 1, b) for b in range(3 * per_row, 4 * per_row)])
    assert sorted(pix.tolist()) == list(range(13 * k["w"], 14 * k["w"]))
    whole = f.levels(f._paths(_orc(), *f.oracle("octree"), ref, np.isin(ref.pixel, pix), k["depth"]))[0]
    assert row_sum.tolist() == list(whole), (row_sum, whole)
    print(f"\n{fam}: {bp} paths per batch, {nbatches} batches; stream 1 batch {shown[0]} (pixels {SM.batch_pixels(SM.SMALL, k, 1, shown[0])}) queues "
          f"{shown[1]} shadow rays per level; image row 13 in all {whole}; frame {live}")
    # ... and at the library's defaults the frame is one batch on one stream, where the readout of the last batch is the call's
    assert SM.batch_paths_of(dict(streams=3, batch_paths=256 << 20, subtile_min_paths=32768), k) == k["w"] * k["h"] * k["spp"]


def test_rows_and_families():
    assert len(SM.CASES) == len(set(SM.CASES)) == 4 * 7 + 2 * 6 + 2 + 3 + 3
    assert [n for n in SM.ROWS if n.startswith("tune_")] == ["tune_xcd1", "tune_xcd2_one_stream", "tune_one_wave_per_cu", "tune_refill_1",
                                                              "tune_refill_64", "tune_small_batches"]
    assert np.dtype(SM.F32) == np.float32
