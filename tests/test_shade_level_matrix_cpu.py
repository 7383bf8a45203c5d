"""The conditions on the inputs of tests/test_shade_level_matrix.py, on the CPU restatement alone (tests/shade_level_cases.py): a row
of that matrix passes vacuously if its adaptive run has no sparse list, if its level never acts, if a tuning leaves a pass in one
batch, if the views show the same image or if the ray permutation leaves a batch in place.  Every row is checked for all of it here,
and the count maps, list shapes and ray counts the matrix was laid out for are pinned, so that a change to a restatement or a scene
shows up in this file first."""
import numpy as np
import pytest

from conftest import assert_bits_equal
import nmap_ref as NR
import shade_level_cases as K

F32 = np.float32
# pixels at count 2, 4, 6, 8 and the rays of the (pixel, sample) pairs below each pixel's count, at tolerance (0.05, 0.01)
PINNED = {"glass": ((862, 11, 9, 142), 5546), "env": ((796, 82, 13, 133), 4897), "smooth": ((905, 44, 5, 70), 4398),
          "tex": ((740, 51, 16, 217), 6299), "nmap": ((740, 54, 18, 212), 6242), "all": ((667, 23, 33, 301), 9148)}


@pytest.mark.parametrize("name", K.ROWS)
def test_the_count_map_is_sparse_and_pinned(name):
    e = K.expect(name)
    u = np.unique(e.counts).tolist()
    assert K.M in u and K.S in u and len(u) >= 3, u
    assert e.tol == (0.05, 0.01) and e.passes == 1 + (K.S - K.M) // K.P
    hist, rays = PINNED[name]
    assert tuple(int((e.counts == n).sum()) for n in (2, 4, 6, 8)) == hist
    assert e.rays == rays and e.samples == int(e.counts.sum()) and 0 < e.unconverged <= hist[3]
    # a sample's colour does not depend on how many samples its pixel ends with: the subset's colours are the full render's rows
    assert_bits_equal(e.subset_color, e.ref.color[e.subset], "path_trace over sample < count vs the render at S")
    assert int(e.subset.sum()) == e.samples


@pytest.mark.parametrize("name", K.ROWS)
def test_every_refinement_list_is_sparse_and_spans_batches(name):
    for e, npix in ((K.expect(name), K.W * K.H), (K.expect_tile(name), 16 * K.W)):
        assert len(e.lists) == e.passes - 1 == 3
        for lst in e.lists:
            assert 0 < len(lst) < npix and not np.array_equal(lst, np.arange(len(lst))), "a prefix of the tile"
            assert (np.diff(lst) > 0).all()
    e = K.expect(name)
    for lst in e.lists:
        assert K.runs(lst) >= 20, K.runs(lst)
        plan = K.plan_batches(len(lst), K.P, K.SMALL, refinement=True)
        assert len(plan) == 4 and all(len(b) >= 2 for b in plan), plan  # four streams, each with two batches and more
        assert sum(n for b in plan for _, n in b) == len(lst)
    # the first pass under the other tuning: one stream, five batches; the `all` row's refinement passes take two
    assert [len(b) for b in K.plan_batches(K.W * K.H, K.M, K.ONE_STREAM)] == [5]
    if name == "all":
        assert all([len(b) for b in K.plan_batches(len(lst), K.P, K.ONE_STREAM, refinement=True)] == [2] for lst in e.lists)
    # the tile's count map differs from the frame's rows only through nothing: the stop rule is per pixel
    t = K.expect_tile(name)
    assert np.array_equal(t.counts, e.counts[t.rows]) and len(np.unique(t.counts)) >= 3
    assert_bits_equal(t.accum, e.accum[t.rows], "the tile's sums are the frame's rows")


@pytest.mark.parametrize("name", K.ROWS)
def test_a_list_position_taken_for_a_pixel_changes_the_colours(name):
    """What the sparse list is for: the rays of the first refinement pass, keyed by their pixel's place in the list instead of the
    pixel, come out in other colours wherever a path draws a random number"""
    e = K.expect(name)
    lst = e.lists[0]
    place = np.zeros(K.W * K.H, np.int64)
    place[lst] = np.arange(len(lst))
    sel = np.isin(e.ref.pixel, lst) & (e.ref.sample >= K.M) & (e.ref.sample < K.M + K.P)
    wrong = K.path_trace(name, e.ref.o4[sel], e.ref.d4[sel], place[e.ref.pixel[sel]], e.ref.sample[sel])
    assert (wrong.color != e.ref.color[sel]).any(axis=1).sum() >= 50


def test_plan_batches_restates_the_equal_batch_rule():
    # a budget a little below the sub-tile: one batch (within 9 / 8); well below: equal batches, not a full one and a sliver
    assert K.plan_batches(1024, 2, {"streams": 1, "batch_paths": 1900}, nrows=32) == [[(0, 1024)]]
    assert K.plan_batches(1024, 2, {"streams": 1, "batch_paths": 1500}, nrows=32) == [[(0, 512), (512, 512)]]
    # three views of 1024 pixels at 4 samples in batches of 600 paths: a batch straddles each view border
    (b,) = K.plan_batches(3 * K.W * K.H, K.VIEW_SPP, {"batch_paths": K.VIEW_BATCH}, nrows=3 * K.H)
    for border in (K.W * K.H, 2 * K.W * K.H):
        assert any(p0 < border < p0 + n for p0, n in b), b
    # the default tuning leaves the three views in one batch: two view borders inside it
    assert K.plan_batches(3 * K.W * K.H, K.VIEW_SPP, {}, nrows=3 * K.H) == [[(0, 3 * K.W * K.H)]]
    # the small tuning on a progressive pass of the full tile: four streams, rows dealt out in turn
    plan = K.plan_batches(K.W * K.H, 5, K.SMALL, nrows=K.H)
    assert len(plan) == 4 and all(sum(n for _, n in b) == 8 * K.W and len(b) >= 2 for b in plan)


@pytest.mark.parametrize("name", K.ROWS)
def test_the_level_is_live(name):
    r, e = K.row(name), K.expect(name)
    pt = e.ref.pt
    if "env" in r.kw:
        assert (pt.hits0[0] == 0).sum() >= 50  # escaping paths read the map
    if "normals" in r.kw:
        hn = NR.hit_normals(r.so, r.normals, None, None, e.ref.o4, e.ref.d4)
        assert (hn.ok & (hn.norm != hn.ng).any(axis=1)).sum() >= 500  # hits shade with a normal other than the geometric one
    if "tex" in r.kw:
        assert sum(pt.tex[k] for k in ("solid", "matte", "reflective", "glass")) >= 500, pt.tex
    if "nm" in r.kw:
        assert pt.nmap["usem"] >= 500, pt.nmap
    if name in K.GLASSY:
        assert min(pt.total["refract_in"], pt.total["tir"], pt.total["schlick"]) > 0, pt.total
    # without the keyword of its own level the row renders another image: a kernel of the level below would not pass
    if name in K.LEVEL_KEY:
        kw = {k: v for k, v in r.kw.items() if k != K.LEVEL_KEY[name]}
        lower = NR.render(K._orc(), r.so, r.vo, K.W, K.H, K.S, K.SEED, K.DEPTH, **kw)
        assert (lower.image != e.ref.image).any(axis=2).sum() >= 50


@pytest.mark.parametrize("name", sorted(K.BELOW))
def test_rows_differ_from_the_row_below(name):
    assert (K.expect(name).ref.image != K.expect(K.BELOW[name]).ref.image).any(axis=2).sum() >= 50


@pytest.mark.parametrize("name", K.ROWS)
def test_progressive_passes_end_in_the_frame(name):
    for tile, rows in ((None, slice(None)), (K.STRIPED, K.expect_tile(name).rows)):
        refs = K.pass_refs(name, tile)
        full = K.expect(name).ref
        assert_bits_equal(refs[-1].image, full.image[rows], "passes [0,1) [1,3) [3,8) end in the render at S")
        assert sum(p.rays for p in refs) == (full.rays if tile is None else K.expect_tile(name).ref.rays)


@pytest.mark.parametrize("name", K.ROWS)
def test_the_three_views_differ_pairwise_and_see_the_scene(name):
    refs = K.view_refs(name)
    for a in range(3):
        assert (refs[a].pt.hits0[0] != 0).sum() >= 200, a
        for b in range(a + 1, 3):
            assert (refs[a].image != refs[b].image).any(axis=2).sum() >= 200, (a, b)


@pytest.mark.parametrize("name", K.ROWS)
def test_the_permutation_moves_every_batch(name):
    c = K.rays_case(name)
    n = len(c.perm)
    assert n == K.W * K.H * K.S and np.array_equal(np.sort(c.perm), np.arange(n))
    for b0 in range(0, n, K.RAYS_BATCH):  # nine in ten rays of every batch come from another batch
        src = c.perm[b0:b0 + K.RAYS_BATCH]
        assert ((src < b0) | (src >= b0 + K.RAYS_BATCH)).mean() >= 0.9
    # keyed by (pixel, sample) a ray keeps its colour wherever it stands; keyed by its place it does not
    assert_bits_equal(c.color, K.expect(name).ref.color[c.perm], "the permuted colours")
    assert (c.group_color != c.color).any(axis=1).mean() > 0.05
    assert c.mean.shape == (n // K.G, 4) and c.ids.shape == (n // K.G,)
