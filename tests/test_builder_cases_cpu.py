"""CPU: the adversarial builder cases of builder_cases.py.  The host mirror's box_contains_polygon and make_triangle against
the oracle's on every case, and the conditions that make the cases what they claim to be, from the oracle alone."""
import numpy as np
import pytest

import builder_cases as bc
from conftest import assert_bits_equal


def _R():
    from rust_raytrace_amd import raytrace as R
    return R


def _host_scene(corners, edge=0.0):
    """The host mirror's scene of the given (oracle-accepted) corners, behind the dummy triangle."""
    R = _R()
    s = R.Scene(True)
    surf = R.SurfaceKind.Solid(R.make_color(10, 20, 30))
    for t in corners:
        s.push_triangle(t, surf, edge)
    return s


@pytest.mark.parametrize("name", bc.FAMILIES)
def test_host_overlap_test_equals_oracle(name):
    r = bc.realise(name)
    host = _host_scene(r.rec[1:, 20:29].reshape(-1, 3, 3))
    assert_bits_equal(host.triangles()[0], r.rec, f"family {name}: triangle records")
    got = np.array([host.box_contains_polygon(r.boxes[b, :3], float(r.boxes[b, 3]), int(t)) for b, t in zip(r.box, r.tri)], bool)
    bad = np.flatnonzero(got != r.answer)
    assert len(bad) == 0, (f"family {name}: {len(bad)} of {len(got)} pairs differ; first: pair {bad[0]} ({r.tag[bad[0]]}), box "
                           f"{r.boxes[r.box[bad[0]]]!r}, triangle {r.rec[r.tri[bad[0]], 20:29]!r}: host {got[bad[0]]}, oracle {r.answer[bad[0]]}")


@pytest.mark.parametrize("name", bc.FAMILIES)
def test_family_has_both_answers_for_both_kinds_of_box(name):
    r = bc.realise(name)
    assert len(r.tri) >= 2000, "a few thousand pairs per family"
    for kind in (0, 1):
        a = r.answer[r.box_kind[r.box] == kind]
        assert a.any() and (~a).any(), f"family {name}, box kind {kind}: {a.sum()} True of {len(a)}"


def test_family_A_covers_every_size_ratio():
    r = bc.realise("A")
    for ratio in ("ratio0.015625", "ratio0.25", "ratio1", "ratio4", "ratio64"):
        a = r.answer[r.tag == ratio]
        assert a.any() and (~a).any(), ratio


def test_family_B_face_plane_placements_give_both_answers():
    r = bc.realise("B")
    on = np.char.startswith(r.tag, "on/")
    assert on.sum() > 500
    # (the True ones are builder boxes whose f32 |p - c| rounds below L; on round boxes every term is exact, the parallel
    # faces divide by 1 - nn*nn = 0 and the perpendicular ones multiply 0 by inf, and the oracle answers False throughout)
    a = r.answer[on]
    assert a.any() and (~a).any(), f"{a.sum()} True of {len(a)}"
    for place in ("in/", "out/"):
        assert np.char.startswith(r.tag, place).sum() > 500
    # and the triangles are what the family says: one coordinate constant, which for `on` is c_k +- L in f32
    c = r.rec[r.tri, 20:29].reshape(-1, 3, 3)
    const = (c == c[:, :1, :]).all(1)
    assert (const.sum(1) == 1).all()
    k = const.argmax(1)
    w = c[np.arange(len(c)), 0, k]
    bx = r.boxes[r.box]
    ck, L = bx[np.arange(len(c)), k], bx[:, 3]
    assert (((w == ck + L) | (w == ck - L))[on]).all()


def test_family_C_is_found_by_the_face_test_alone():
    r = bc.realise("C")
    pts = np.concatenate([r.rec[r.tri, 0:3][:, None, :], r.rec[r.tri, 20:29].reshape(-1, 3, 3)], 1)   # incenter + corners
    inside = np.array([bc.points_inside(r.boxes[b], p).any() for b, p in zip(r.box, pts)])
    assert (r.answer & ~inside).sum() >= 100
    for tag in ("pierce", "graze_in", "graze_out", "par_in", "par_out"):
        assert (r.tag == tag).sum() >= 100, tag
    for tag in ("graze_in", "graze_out"):
        a = r.answer[r.tag == tag]
        assert a.any() and (~a).any(), tag
    # much larger than the box: the shortest edge is above 8 half edges
    c = r.rec[r.tri, 20:29].reshape(-1, 3, 3).astype(np.float64)
    edge = np.linalg.norm(c - np.roll(c, 1, axis=1), axis=2).min(1)
    assert (edge > 8.0 * r.boxes[r.box, 3]).all()


def test_family_D_points_sit_on_the_boundary():
    r = bc.realise("D")
    bx = r.boxes[r.box]
    on = np.char.endswith(r.tag, "/on")
    corner = np.char.startswith(r.tag, "corner")
    c = r.rec[r.tri, 20:29].reshape(-1, 3, 3)
    dc = np.abs(c - bx[:, None, :3])                         # f32, as box_contains_point subtracts
    hit_corner = (dc == bx[:, None, 3:4]).any((1, 2))
    di = np.abs(r.rec[r.tri, 0:3] - bx[:, :3])
    hit_inc = (di == bx[:, 3:4]).any(1)
    for kind in (0, 1):
        m = r.box_kind[r.box] == kind
        assert hit_corner[on & corner & m].mean() > 0.9, kind
        assert hit_inc[on & ~corner & m].sum() >= 20, kind
    # `on`: no point strictly inside, so the answer is the face test's; all three placements give both answers
    for place in ("on", "in", "out"):
        a = r.answer[np.char.endswith(r.tag, "/" + place)]
        assert a.any() and (~a).any(), place
    pts = np.concatenate([r.rec[r.tri, 0:3][:, None, :], c], 1)
    inside = np.array([bc.points_inside(r.boxes[b], p).any() for b, p in zip(r.box, pts)])
    assert not inside[on & corner & hit_corner & (np.char.find(r.tag, "corner3") >= 0)].any()


def test_family_E_reaches_tmin_zero():
    r = bc.realise("E")
    for tag in ("edge_in_face", "edge_on_box_edge", "plane_has_box_edge", "tmin0"):
        a = r.answer[r.tag == tag]
        assert a.any() and (~a).any(), tag
    m = r.tag == "tmin0"
    zeros = 0
    for b in np.unique(r.box[m]):
        mm = m & (r.box == b)
        for axis in range(6):
            zeros += int((bc.face_first_pass_tmin(r.boxes[b], axis, r.rec[r.tri[mm], 3:6], r.rec[r.tri[mm], 0:3]) == 0).sum())
    assert zeros >= 10, "face lines that start exactly on a slab plane (first-pass tmin == 0)"


def test_family_F_aspect_ratio():
    fam = bc.pair_family("F")
    r = bc.realise("F")
    assert r.accepted.sum() >= 1000 and (~r.accepted).sum() >= 1000      # make_triangle accepts some and rejects some
    assert (bc.aspect_ratio(fam["tris"]) >= 1e3).all()


# ---------------------------------------------------------------- make_triangle
def test_median_solve_restatement_equals_oracle():
    """The NumPy restatement the generators and the checks below rely on: same accept/reject set and incenter bits."""
    pts, _ = bc.all_corners()
    acc, rec = bc.oracle_make_triangles()
    m = bc.median_solve_f32(pts)
    assert np.array_equal(m["ok"], acc)
    assert_bits_equal(m["incenter"][acc], rec[:, 0:3], "incenter")


def test_host_make_triangle_equals_oracle():
    R = _R()
    pts, names = bc.all_corners()
    acc, rec = bc.oracle_make_triangles(0.05)
    s = R.Scene(False)
    surf = R.SurfaceKind.Solid(R.make_color(10, 20, 30))
    got = np.zeros(len(pts), bool)
    for i, t in enumerate(pts):
        try:
            s.push_triangle(t, surf, 0.05)
            got[i] = True
        except RuntimeError as e:
            assert "degenerate" in str(e)
    bad = np.flatnonzero(got != acc)
    assert len(bad) == 0, f"{len(bad)} triangles accepted by one side only; first {bad[0]} ({names[bad[0]]}): host {got[bad[0]]}, {pts[bad[0]]!r}"
    assert_bits_equal(s.triangles()[0], rec, "all 29 record floats")


def test_corner_sets_straddle_the_thresholds():
    pts, names = bc.all_corners()
    acc, rec = bc.oracle_make_triangles()
    m = bc.median_solve_f32(pts)
    det01 = np.abs(m["det"][:, 0])
    for n in sorted(set(names)):
        print(n, (names == n).sum(), "accepted", acc[names == n].sum())
    assert acc[names == "soup"].mean() > 0.9
    assert not acc[names == "degenerate"][:7].any() and acc[names == "degenerate"][7]
    # determinant threshold 1e-4: needles whose determinants (all three pairs) are just below, and just above
    nd = names == "needle_det"
    allbelow = (np.abs(m["det"]) < np.float32(1e-4)).all(1)
    assert (nd & allbelow & ~acc).sum() >= 50 and (nd & ~allbelow & acc).sum() >= 50
    top = np.abs(m["det"]).max(1)
    assert ((top[nd] > 0.5e-4) & (top[nd] < 1e-4)).sum() >= 20 and ((top[nd] >= 1e-4) & (top[nd] < 2e-4)).sum() >= 20
    # reject threshold 0.01 on |p2 - p1|^2
    nr = names == "near_reject"
    d2 = m["dist2"]
    assert (nr & acc & (d2 > 0.005)).sum() >= 10 and (nr & ~acc & (d2 >= 0.01) & (d2 < 0.02)).sum() >= 10
    # the later coordinate pairs run: accepted triangles whose first-pair determinant is below 1e-4
    assert (acc & (det01 < 1e-4) & (m["pair"] == 1)).sum() >= 100
    assert (acc & (det01 < 1e-4) & (m["pair"] == 2)).sum() >= 100
    ax = names == "axis"
    assert acc[ax].all()
    assert set(m["pair"][ax]) == {0, 1, 2}
    k = np.flatnonzero(ax)
    assert (m["pair"][k[:120]] == 2).all() and (m["pair"][k[120:240]] == 1).all()      # x = const: (1,2); y = const: (0,2)
