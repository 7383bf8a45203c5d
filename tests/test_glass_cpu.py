"""No GPU: the restatement of the dielectric surface kind (tests/glass_ref.py) is pinned before tests/test_glass.py trusts it, and the
interface that carries the kind is checked where no device is needed.
 1. Without glass the restatement is Scene.render, bit for bit (the canonical pair).
 2. Its refraction and Fresnel arithmetic agree with an independent float64 textbook evaluation, t = eta d + (eta cos_i - sqrt(k)) n
    with Schlick's approximation, over a fixed sample of directions and normals.  The margins are measured, not guessed: DIR_MEASURED
    and R_MEASURED are the largest deviations of the float32 listing from the float64 evaluation on the machine the test was written
    on and the test asserts 8 x that -- headroom for another libm or NumPy, not for another formula.  Cases within
    K_NEAR of the critical angle are left out (sqrt(k) amplifies rounding there); they must stay under 1 % of the sample.
 3. The reflect-or-refract decision draws word 3 of the bounce block: its share of reflections matches R within a two-sided binomial
    bound at draw_ref's false-alarm level, and it is uncorrelated with the Lambert lobe drawn from words 0-2 of the same block.
 4. The slab's view shows every event (entering, leaving, Schlick, total internal reflection) by the restatement alone, and its side
    view holds paths for 32 bounces.
 5. The interface: SurfaceKind.Dielectric, flattening, the raw ABI's surface check."""
import numpy as np
import pytest

import capacity_cases as CC
import draw_ref as DR
import glass_cases as GC
import glass_ref as GR
from conftest import OracleApi, assert_bits_equal
from rays_ref import vunit

F32 = np.float32
IORS = (1.0, 1.33, 1.5, 2.4)
NSAMPLE = 4000            # directions and normals per (ior, face)
K_NEAR = 1e-4             # |k| below this (float64) is "near the critical angle"
DIR_MEASURED = 5.618e-6   # largest |td_f32 - t_f64| (a component) over the kept cases, as measured
R_MEASURED = 2.095e-5     # largest |R_f32 - R_f64| over the kept cases, as measured


def _orc():
    from oracle import orc
    return orc


def _R():
    from rust_raytrace_amd import raytrace as R
    return R


# ---------------------------------------------------------------- 1
def test_without_glass_the_restatement_is_the_oracle(canonical_pair):
    orc = _orc()
    so, _ = canonical_pair
    w, h, spp, seed, maxdepth = 24, 20, 3, 5, 6
    vo = orc.canonical_viewport(w, h)
    want, cn = so.render(w, h, vo, maxdepth, spp, seed=seed, threads=4)
    got = GR.render(orc, so, vo, w, h, spp, seed, maxdepth)
    assert_bits_equal(got.image, want, "glass_ref.render against Scene.render")
    assert got.rays == cn["rays"] and got.pt.total == dict.fromkeys(GR.EVENTS, 0)
    assert got.passes[-1] > 0 and len(np.unique(want)) > 100


# ---------------------------------------------------------------- 2
def _sample():
    rng = np.random.default_rng(20240611)
    d = np.zeros((NSAMPLE, 4), F32)
    n = np.zeros((NSAMPLE, 4), F32)
    d[:, :3] = rng.normal(size=(NSAMPLE, 3))
    n[:, :3] = rng.normal(size=(NSAMPLE, 3))
    d, n = vunit(d), vunit(n)
    against = (d.astype(np.float64) * n.astype(np.float64)).sum(axis=1) > 0
    n[against] = -n[against]  # shade_hit's norm faces the ray on either face
    return d, n


def _float64(d, n, ior, back):
    """The textbook evaluation in float64: t = eta d + (eta cos_i - sqrt(k)) n, Schlick with the cosine on the thin side"""
    d, n = d[:, :3].astype(np.float64), n[:, :3].astype(np.float64)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    eta = ior if back else 1.0 / ior
    cos_i = -(d * n).sum(axis=1)
    k = 1.0 - eta * eta * (1.0 - cos_i * cos_i)
    with np.errstate(invalid="ignore"):
        cos_t = np.sqrt(k)
        t = eta * d + (eta * cos_i - cos_t)[:, None] * n
        t /= np.linalg.norm(t, axis=1, keepdims=True)
    r0 = ((1.0 - ior) / (1.0 + ior)) ** 2
    R = r0 + (1.0 - r0) * (1.0 - (cos_t if back else cos_i)) ** 5
    return t, k, R


def test_refraction_and_schlick_against_float64():
    d, n = _sample()
    zeros = np.zeros((NSAMPLE, 4), F32)
    dev_dir = dev_R = 0.0
    near = total = 0
    for ior in IORS:
        for back in (False, True):
            g = GR.dielectric_ray(zeros, n, d, np.full(NSAMPLE, ior, F32), np.full(NSAMPLE, back), zeros, np.ones(NSAMPLE, F32))
            t64, k64, R64 = _float64(d, n, float(F32(ior)), back)
            keep = np.abs(k64) >= K_NEAR
            near += int((~keep).sum())
            total += NSAMPLE
            assert np.array_equal(g.tir[keep], k64[keep] < 0), f"ior {ior}, back {back}: total internal reflection"
            assert g.reflect[keep & ~(k64 < 0)].sum() == 0 and g.reflect[keep & (k64 < 0)].all()  # u = 1: only tir reflects
            ok = keep & (k64 >= 0)
            if back and ior > 1.0:  # leaving the denser medium: a good share is beyond the critical angle
                assert (k64 < 0).sum() > NSAMPLE // 10
            else:
                assert not (k64 < 0).any()
            assert (g.td[ok, 3] == 0).all()
            dev_dir = max(dev_dir, float(np.abs(g.td[ok, :3].astype(np.float64) - t64[ok]).max()))
            dev_R = max(dev_R, float(np.abs(g.R[ok].astype(np.float64) - R64[ok]).max()))
            # the ray as make_ray stores it: the origin moved 0.001 along the unit direction
            assert np.abs(np.linalg.norm(g.d[ok, :3].astype(np.float64), axis=1) - 1).max() < 1e-6
            assert np.abs(g.o[ok, :3] / F32(0.001) - g.td[ok, :3]).max() < 1e-3
    print(f"float32 listing against float64: direction {dev_dir:.3e}, R {dev_R:.3e}, near the critical angle {near} of {total}")
    assert near <= total // 100, f"{near} of {total} cases within {K_NEAR} of the critical angle"
    assert dev_dir <= 8 * DIR_MEASURED, dev_dir
    assert dev_R <= 8 * R_MEASURED, dev_R


def test_ior_one_goes_straight_on():
    d, n = _sample()
    zeros = np.zeros((NSAMPLE, 4), F32)
    for back in (False, True):
        g = GR.dielectric_ray(zeros, n, d, np.ones(NSAMPLE, F32), np.full(NSAMPLE, back), zeros, np.ones(NSAMPLE, F32))
        # k = 1 - (1 - ci^2) carries up to 2 ulp(1) = 2.4e-7 of rounding (ci^2, s2 and k each round below 1), so ct = sqrt(k) is
        # off by at most 2.4e-7 / (2 ci) = 1.2e-6 at ci >= 0.1; the two normalisations add a few ulp: 2e-6 in all.  No clamp
        # repairs the grazing rays, where the same error is divided by a smaller ci: they only have to stay finite.
        steep = g.ci >= 0.1
        assert steep.sum() > NSAMPLE // 2 and np.abs(g.td - d)[steep].max() < 2e-6
        assert not g.tir[steep].any() and np.isfinite(g.td[g.ci > 1e-3]).all()


# ---------------------------------------------------------------- 3
def test_reflection_share_matches_R_and_is_independent_of_the_lobe():
    orc = _orc()
    n, seed = 4096, 9
    pixel, sample = np.arange(n), np.zeros(n, np.int64)
    rv, u = GR.random_vec_u(orc, seed, pixel, sample, 1)
    nrm = np.tile(np.array([0, 0, -1, 0], F32), (n, 1))
    rd = np.tile(vunit(np.array([[np.sin(np.pi / 3), 0, np.cos(np.pi / 3), 0]], F32)), (n, 1))  # entering at 60 degrees
    g = GR.dielectric_ray(np.zeros((n, 4), F32), nrm, rd, np.full(n, 1.5, F32), np.zeros(n, bool), rv, u)
    R = float(g.R[0])
    assert (g.R == g.R[0]).all() and not g.tir.any() and abs(R - (0.04 + 0.96 * 0.5 ** 5)) < 1e-6
    k = int(g.reflect.sum())
    bound = DR.Z_TWO_SIDED * np.sqrt(n * R * (1 - R))
    print(f"reflections {k} of {n}, expected {n * R:.1f} +- {bound:.1f}")
    assert abs(k - n * R) <= bound
    # the reflected rays are reflect_ray's with scattering 0: one direction for all; the refracted ones likewise
    assert len(np.unique(g.d[g.reflect], axis=0)) == 1 and len(np.unique(g.d[~g.reflect], axis=0)) == 1
    assert g.d[g.reflect][0, 2] < 0 < g.d[~g.reflect][0, 2]
    c = DR.contingency_chi2(g.reflect.astype(np.int64), (rv[:, 0] > 0).astype(np.int64), 2, 2)
    print(f"reflected against sign(rv.x): chi2 {c['chi2']:.2f}, threshold {c['threshold']:.2f}")
    assert c["ok"], c
    # and word 3 is not one of the lobe's words
    w = np.array([orc.rng_block(seed, int(p), 0, 1) for p in pixel[:64]], np.uint32)
    assert np.array_equal(GR.unit_f32(w[:, 3]), u[:64])


# ---------------------------------------------------------------- 4
@pytest.fixture(scope="module")
def slab_oracle():
    return GC.recipe_slab()(OracleApi(_orc()))


def test_the_box_is_wound_outwards(slab_oracle):
    rec, kinds, _ = slab_oracle.triangles()
    glass = np.flatnonzero(kinds == GR.DIELECTRIC)
    assert len(glass) == 12
    centre = 0.5 * (np.array(GC.SLAB["lo"]) + np.array(GC.SLAB["hi"]))
    out = ((rec[glass, 0:3] - centre) * rec[glass, 3:6]).sum(axis=1)  # (incenter - centre) . norm
    assert (out > 0).all()


def test_the_slab_view_shows_every_event(slab_oracle):
    orc = _orc()
    w, h = GC.VIEW["w"], GC.VIEW["h"]
    r = GR.render(orc, slab_oracle, orc.canonical_viewport(w, h), w, h, 4, 5, 8)
    print("events", r.pt.total, "passes", r.passes)
    assert all(r.pt.total[e] >= 10 for e in GR.EVENTS), r.pt.total
    assert all(p % 256 for p in r.passes[1:])  # no bounce queue is a whole number of blocks
    assert r.pt.exhausted.any()


def test_the_side_view_holds_paths_for_32_bounces(slab_oracle):
    orc = _orc()
    c = GC.SIDE_VIEW
    r = GR.render(orc, slab_oracle, GC.side_viewport(orc), c["w"], c["h"], 2, 5, 32)
    trapped = r.pt.exhausted & (r.pt.last_tir >= 30)
    assert trapped.sum() >= 2 and not r.color[trapped].any()


# ---------------------------------------------------------------- 5
def test_surface_kind_dielectric_exists():
    R = _R()
    s = R.SurfaceKind.Dielectric(1.5, R.make_color(255, 255, 255))
    assert R.DIELECTRIC == 3 and s.kind == 3 and s.alpha == 1.0 and s.scattering == 1.5
    assert R.SurfaceKind.Dielectric(1.33, R.make_color(1, 2, 3), 0.5).alpha == 0.5


def test_a_glass_triangle_flattens_to_kind_3_with_its_ior():
    R = _R()
    s = R.Scene(with_dummy=True)
    s.push_triangle(np.array([[0, 0, 5], [1, 0, 5], [0, 1, 5]], F32), R.SurfaceKind.Dielectric(1.5, R.make_color(10, 20, 30), 0.75), 0.0)
    _, kinds, surf = s.triangles()
    assert kinds[1] == 3 and surf[1, 4] == F32(1.5) and surf[1, 3] == F32(0.75)
    assert_bits_equal(surf[1, 0:3], R.make_color(10, 20, 30), "colour")
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(RuntimeError, match="index of refraction"):
            s.push_triangle(np.array([[0, 0, 5], [1, 0, 5], [0, 1, 5]], F32), R.SurfaceKind.Dielectric(bad, R.make_color(10, 20, 30)), 0.0)
    assert s.num_tris() == 2


def test_both_builds_of_the_slab_are_the_same_records():
    so, sp = GC.build_pair(GC.recipe_slab())
    (ro, ko, fo), (rp, kp, fp) = so.triangles(), sp.triangles()
    assert np.array_equal(ko, kp) and (ko == 3).sum() == 12
    assert_bits_equal(ro, rp, "records")
    assert_bits_equal(fo, fp, "surfaces")


def _abi_scene(kind, ior):
    from rust_raytrace_amd import _ffi
    so = GC.recipe_slab()(OracleApi(_orc()))
    rec, kinds, surf = so.triangles()
    kinds, surf = kinds.copy(), surf.copy()
    glass = np.flatnonzero(kinds == 3)
    kinds[glass[5]] = kind
    surf[glass[5], 4] = ior
    L = _ffi.lib()
    rc, h, msg = CC.create_one_leaf_scene(L, CC.abi_triangles(rec, kinds, surf))
    if rc == CC.RTMI_OK:
        L.rtmi_scene_destroy(h)
    return rc, msg, int(glass[5])


def test_raw_abi_accepts_kind_3_and_checks_the_ior():
    rc, msg, _ = _abi_scene(3, 1.5)
    assert rc in (CC.RTMI_OK, CC.RTMI_ERR_NO_DEVICE), (rc, msg)  # past the surface check: only the device can be missing
    for bad in (0.0, -1.0, float("nan"), float("inf"), float("-inf")):
        rc, msg, i = _abi_scene(3, bad)
        assert rc == CC.RTMI_ERR_INVALID and b"index of refraction" in msg and f"triangle {i}:".encode() in msg, (bad, rc, msg)
    rc, msg, _ = _abi_scene(4, 1.5)
    assert rc == CC.RTMI_ERR_INVALID and b"unknown surface kind" in msg, (rc, msg)
    rc, msg, _ = _abi_scene(2, float("nan"))  # the check is the dielectric's alone
    assert rc in (CC.RTMI_OK, CC.RTMI_ERR_NO_DEVICE), (rc, msg)
