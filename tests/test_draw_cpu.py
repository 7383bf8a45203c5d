"""The CPU oracle and the NumPy restatements (ao_ref.py, light_ref.py) against the float64 statistical referee
(tests/draw_ref.py): do Lambert sampling, fuzzy reflection, the pixel jitter, the AO rays and the light samples have the
distribution the reference's definitions say, independently across pixels, samples and bounces?  Every threshold is the
quantile at a false-alarm probability of 1e-6 for the test's own degrees of freedom, or comes from the float32 format; none is
taken from an output.  Every test prints its figures (run with -s); DESIGN.md section 2 (vii) holds the table.  No GPU."""
import functools

import numpy as np
import pytest

from conftest import OracleApi, ProductApi, assert_bits_equal
import ao_ref as AR
import draw_ref as D
import light_ref as LR

F32 = np.float32
DEPTHS = (2, 3, 5)
FUZZ = (0.3, 1.0)
FUZZ_DEPTHS = (2, 3)
AO_FRAME, AO_S, AO_K = 64, 4, 16
LIGHT_FRAME, LIGHT_S, LIGHT_K = 32, 4, 16


def _orc():
    from oracle import orc
    return orc


def probe_viewport(orc, w, h):
    v = D.VIEW
    return orc.create_viewport(w, h, v["size"], np.array(v["pos"], F32), orc.unit(list(v["aim"])), v["fov"], v["roll"])


# ---------------------------------------------------------------- shared cases (computed once)
@functools.lru_cache(maxsize=None)
def view(w=D.W, h=D.H):
    orc = _orc()
    vp = probe_viewport(orc, w, h)
    o4, d4 = orc.primary_rays(w, h, vp, 1)
    return vp, o4, d4


@functools.lru_cache(maxsize=None)
def referee(normal, floor, maxdepth):
    """The referee's chains for one floor: REF_FACTOR per observed primary hit, followed to `maxdepth` rays once"""
    _, o4, d4 = view()
    probe = D.Probe(normal)
    p, d = probe.primary_hits(o4, d4)
    rng = np.random.default_rng([20261019, sorted(D.NORMALS).index(normal), int(1000 * (floor[1] if len(floor) > 1 else 0))])
    end, face = D.chains(probe, *D.referee_points(p, d), floor, maxdepth, rng)
    return dict(probe=probe, p=p, d=d, end=end, face=face)


@functools.lru_cache(maxsize=None)
def oracle_scene(normal, floor, accel):
    return D.recipe(normal, floor=floor, accel=accel)(OracleApi(_orc()))


@functools.lru_cache(maxsize=None)
def oracle_image(normal, floor, accel, seed, depth):
    vp, _, _ = view()
    return oracle_scene(normal, floor, accel).render(D.W, D.H, vp, depth, 1, seed=seed, threads=4)


def oracle_frame(normal, floor, accel, seed, depth):
    img, cn = oracle_image(normal, floor, accel, seed, depth)
    return D.decode(img).reshape(-1), cn


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    for f in (view, referee, oracle_scene, oracle_image, ao_case, light_case):
        f.cache_clear()


def check_bins(bins, ref, depth, what, counters=None, min_bins=15, rays_test=True):
    """The conditions, then the two-sample chi-square of a frame's bins against the referee's, then (with counters) rays / N:
    a z-test with the variance of the referee's chain lengths.  rays_test=False (the fuzzy floors, where the issue asks for no
    such test and the referee's chains all have one length) prints the figure only."""
    obs = np.bincount(bins, minlength=D.UNDECODED + 1)
    exp = np.bincount(D.outcome(ref["end"], ref["face"], depth), minlength=D.UNDECODED + 1)
    r = D.two_sample_chi2(obs, exp)
    line = (f"  {what:44s} black {obs[D.BLACK] / len(bins):7.2%}  chi2 {r['chi2']:7.1f}  df {r['df']:3d}  threshold {r['threshold']:6.1f}"
            f"  bins {r['bins']:3d}")
    if r["pooled"] is not None:
        line += f"  pooled bin {r['pooled'][0]} (expected {r['pooled'][1]:.1f})"
    z = None
    if counters is not None:
        rr = D.rays(ref["end"], depth)
        z = D.z_test(counters["rays"] / len(bins), len(bins), rr.mean(), rr.var(), len(rr))
        line += f"  rays/N {counters['rays'] / len(bins):.4f} (referee {rr.mean():.4f}, z {z['z']:+.2f})"
    print(line)
    assert obs[D.UNDECODED] == 0, f"{what}: {obs[D.UNDECODED]} samples decode to no dome face, black or sky"
    assert obs[D.SKY] == 0, f"{what}: {obs[D.SKY]} samples left a watertight dome"
    assert r["bins"] >= min_bins, f"{what}: only {r['bins']} unpooled bins"
    assert r["ok"], f"{what}: chi2 {r['chi2']:.1f} over the threshold {r['threshold']:.1f} at 1e-6 (df {r['df']})"
    assert z is None or not rays_test or z["ok"], f"{what}: rays per sample {counters['rays'] / len(bins):.4f}, z {z['z']:.2f} against the referee"
    return r


# ---------------------------------------------------------------- the instrument itself
def test_probe_is_sound():
    orc = _orc()
    assert D.dome_triangles().shape == (80, 3, 3)
    for normal in D.NORMALS:
        probe = D.Probe(normal)
        assert probe.convex() <= 1e-12, "the plane form of the dome needs a convex dome"
        _, o4, d4 = view()
        p, _ = probe.primary_hits(o4, d4)
        # both floor triangles are listed in the leaf that holds C; the floor that faces the camera is parallel to an axis plane
        # and listed only where a corner or its centre lies (draw_ref._frame), so every point seen of it must lie in that leaf
        geo, topo, refs = oracle_scene(normal, ("matte",), "octree").tree_flatten()
        leaf = np.nonzero((topo[:, 2] == 1) & (np.abs(geo[:, :3] - D.C[None]) < geo[:, 3:4]).all(axis=1))[0]
        assert len(leaf) == 1
        b = int(leaf[0])
        assert {1, 2} <= set(refs[topo[b, 0]:topo[b, 0] + topo[b, 1]].tolist()), f"{normal}: the leaf at C does not list the floor"
        assert normal != "facing" or (np.abs(p - geo[b, :3]) < geo[b, 3] - 0.01).all()
    # the decoder: every dome colour, black, the sky, and two colours that are neither
    cols = np.array([orc.make_color(*D.dome_rgb(k)) for k in range(D.NFACES)] + [orc.make_color(0, 0, 0), orc.make_color(*D.SKY_RGB),
                    orc.make_color(*D.FLOOR_RGB), orc.make_color(1, 254, 7) * F32(0.5)])
    assert D.decode(cols).tolist() == list(range(D.NFACES)) + [D.BLACK, D.SKY, D.UNDECODED, D.UNDECODED]


def test_referee_imports_numpy_and_the_standard_library_only():
    import ast
    tree = ast.parse(open(D.__file__).read())
    names = {a.name for n in ast.walk(tree) if isinstance(n, ast.Import) for a in n.names}
    froms = {n.module for n in ast.walk(tree) if isinstance(n, ast.ImportFrom)}
    assert names <= {"math", "statistics", "numpy"} and not froms, (names, froms)


def test_thresholds_against_scipy():
    """Wilson-Hilferty against the exact quantile: never below it in the upper tail at 1e-6, within 16 % at df 1 and 5 % from
    df 5 on; the lower tail of the dispersion test (df in the thousands) within 0.1 %"""
    st = pytest.importorskip("scipy.stats")
    for df in (1, 2, 3, 5, 10, 20, 25, 40, 63, 100, 225, 1024, 4096):
        exact, wh = float(st.chi2.isf(D.P_FALSE, df)), D.chi2_threshold(df)
        print(f"  df {df:5d}: exact {exact:9.2f}  Wilson-Hilferty {wh:9.2f}  ({wh / exact - 1:+.2%})")
        assert exact <= wh <= exact * (1.16 if df < 5 else 1.05)
    for df in (1024, 4096):
        for p in (D.P_FALSE / 2, 1 - D.P_FALSE / 2):
            assert abs(D.chi2_threshold(df, p) / float(st.chi2.isf(p, df)) - 1) <= 1e-3
    assert abs(D.Z_TWO_SIDED - float(st.norm.isf(D.P_FALSE / 2))) <= 1e-9


# ---------------------------------------------------------------- Lambert and fuzzy reflection
@pytest.mark.parametrize("normal", list(D.NORMALS))
def test_lambert(normal):
    ref = referee(normal, ("matte",), max(DEPTHS))
    print(f"\nLambert, floor normal {normal}:")
    for accel in ("octree", "list"):
        for seed in D.SEEDS:
            for depth in DEPTHS:
                bins, cn = oracle_frame(normal, ("matte",), accel, seed, depth)
                check_bins(bins, ref, depth, f"oracle {accel} seed {seed} maxdepth {depth}", cn)


# The number of unpooled bins is a property of the instrument alone (the referee's expected counts at N), not of the renderer.
# At scattering 0.3 the reflected directions fill a cone of half-angle asin(0.3) = 17.5 degrees, 0.29 sr, and a dome face spans
# 4 pi / 80 = 0.157 sr: the cone reaches seven faces, so fifteen bins cannot exist there.  That case asks for five, and
# test_self_check_fuzzy_cone_has_power shows that seven bins still report a wrong sampler; every other case asks for fifteen.
FUZZ_MIN_BINS = {0.3: 5, 1.0: 15}


@pytest.mark.parametrize("scattering", FUZZ)
def test_fuzzy_reflection(scattering):
    floor = ("reflective", scattering)
    ref = referee("tilted", floor, max(FUZZ_DEPTHS))
    print(f"\nfuzzy reflection, scattering {scattering}:")
    for accel in ("octree", "list"):
        for seed in D.SEEDS:
            for depth in FUZZ_DEPTHS:
                bins, cn = oracle_frame("tilted", floor, accel, seed, depth)
                check_bins(bins, ref, depth, f"oracle {accel} seed {seed} maxdepth {depth}", cn, FUZZ_MIN_BINS[scattering], rays_test=False)


def check_independence(bins2, ref, what):
    """Neighbouring pixels at one sample per pixel: contingency of the coarse class (black, and the dome bins in five classes
    of about equal expected mass) of pixel p against p + 1 and against p + width, on a frame's bins at maxdepth 2.
    (Bounce against bounce has no table of its own: a chain's colour shows its last draw only, and the class at maxdepth 2 is a
    function of the bin at maxdepth 3, so such a table is test_lambert's maxdepth-3 histogram again.  That histogram is what
    holds the second draw, and test_self_check_wrong_samplers_are_reported shows it reports one r for bounce 1 and 2.)"""
    exp2 = np.bincount(D.outcome(ref["end"], ref["face"], 2), minlength=D.UNDECODED + 1)
    cls, ncls = D.coarse_classes(exp2)
    img = cls[bins2].reshape(D.H, D.W)
    right = D.contingency_chi2(img[:, :-1].reshape(-1), img[:, 1:].reshape(-1), ncls, ncls)
    below = D.contingency_chi2(img[:-1].reshape(-1), img[1:].reshape(-1), ncls, ncls)
    print(f"  {what:36s} p|p+1 chi2 {right['chi2']:6.1f}  p|p+w chi2 {below['chi2']:6.1f}  (df {right['df']}, threshold {right['threshold']:.1f})")
    assert right["df"] == (ncls - 1) ** 2 and right["min_expected"] >= D.MIN_EXPECTED
    assert right["ok"] and below["ok"], f"{what}: neighbouring pixels are not independent: {right}, {below}"
    return right, below


@pytest.mark.parametrize("normal", list(D.NORMALS))
def test_independence_at_one_sample(normal):
    ref = referee(normal, ("matte",), max(DEPTHS))
    print(f"\nindependence, floor normal {normal}:")
    for seed in D.SEEDS:
        check_independence(oracle_frame(normal, ("matte",), "octree", seed, 2)[0], ref, f"oracle octree seed {seed}")


# ---------------------------------------------------------------- the jitter
JW = JH = 128


def print_jitter(what, rep, margin):
    print(f"  {what:24s} margin {margin:.2e}  outside {rep['outside']}  twins {rep['twins']}  grid chi2 {rep['grid']['chi2']:.1f} (df 63, "
          f"threshold {rep['grid']['threshold']:.1f})  corr z {rep['corr']['z']:+.2f}  s|s+1 chi2 {rep['samples']['chi2']:.1f}  p|p+1 chi2 "
          f"{rep['pixels']['chi2']:.1f} (df 225, threshold {rep['pixels']['threshold']:.1f})  near pairs of all {rep['all_pairs']['count']} "
          f"(mean {rep['all_pairs']['mean']:.1f}, limit {rep['all_pairs']['limit']:.1f})")


@pytest.mark.parametrize("seed", D.SEEDS)
def test_jitter(seed):
    orc = _orc()
    vp = orc.canonical_viewport(JW, JH)
    o4, _ = orc.primary_rays(JW, JH, vp, 4, seed=seed)
    u, v, resid, margin = D.pixel_offsets(o4, vp, JW, JH, 4)
    rep = D.jitter_report(u, v, JW, JH, 4, margin)
    print()
    print_jitter(f"oracle seed {seed}", rep, margin)
    assert margin <= 1e-3 and resid <= margin / JW, (margin, resid)        # the origins lie in the viewport's plane
    assert rep["outside"] == 0, f"{rep['outside']} offsets outside [0, 1) by more than {margin:.2g}"
    assert rep["twins"] == 0, f"{rep['twins']} pairs of (pixel, sample) share their offsets"
    for k in D.JITTER_TESTS:
        assert rep[k]["ok"], (k, rep[k])


def test_jitter_at_one_sample_is_the_pixel_centre():
    orc = _orc()
    vp = orc.canonical_viewport(JW, JH)
    o4, _ = orc.primary_rays(JW, JH, vp, 1, seed=2)
    u, v, _, margin = D.pixel_offsets(o4, vp, JW, JH, 1)
    assert np.abs(u - 0.5).max() <= margin and np.abs(v - 0.5).max() <= margin
    # exactly: the origin is the float32 expression of pixel_ray with 0.5f
    assert_bits_equal(o4[:, :3], D.centre_origins(vp, JW, JH), "origins at one sample per pixel")


# ---------------------------------------------------------------- ambient occlusion (ao_ref.py)
AO_CASES = {"a": dict(occluder=False, flip=False, radius=np.inf), "b": dict(occluder=True, flip=False, radius=3.0),
            "c": dict(occluder=True, flip=True, radius=3.0), "d": dict(occluder=True, flip=False, radius=0.0)}


@functools.lru_cache(maxsize=None)
def ao_case(name):
    """scene parameters, the probe, the centre rays' hits as an (h, w, 3) grid, and the referee's visible share per pixel"""
    c = AO_CASES[name]
    vp, o4, d4 = view(AO_FRAME, AO_FRAME)
    probe = D.Probe("tilted", flip=c["flip"], dome=False, occluder=c["occluder"])
    p, d = probe.primary_hits(o4, d4)
    grid = p.reshape(AO_FRAME, AO_FRAME, 3)
    rng = np.random.default_rng([20261019, 7, ord(name)])
    p_hat, m_ref = D.ao_expectation(probe, grid, d, AO_S * AO_K, c["radius"], 0.001, rng)
    return dict(c, probe=probe, grid=grid, d=d, p_hat=p_hat, m_ref=m_ref, vp=vp)


def ao_recipe(name, accel):
    c = AO_CASES[name]
    return D.recipe("tilted", accel=accel, dome=False, occluder=c["occluder"], flip=c["flip"])


def check_ao(img, name, what):
    case = ao_case(name)
    n = AO_S * AO_K
    if name in ("a", "d"):
        assert (np.asarray(img) == F32(1.0)).all(), f"{what}: case {name} must read exactly 1.0 everywhere"
        assert (case["p_hat"] == 1.0).all()
        print(f"  {what:28s} case {name}: 1.0 on every pixel")
        return None
    rep = D.ao_report(D.ao_counts(img, n), n, case["p_hat"], case["m_ref"])
    t, dsp = rep["total"], rep["dispersion"]
    print(f"  {what:28s} case {name}: visible {t['share']:.4f} (referee {t['expected']:.4f}, z {t['z']:+.2f})  dispersion {dsp['chi2']:.0f} "
          f"in [{dsp['lo']:.0f}, {dsp['hi']:.0f}] (df {dsp['df']})")
    assert 0.05 <= t["expected"] <= 0.95 and dsp["df"] >= 0.9 * AO_FRAME * AO_FRAME, "the case must occlude a real share on nearly every pixel"
    assert t["ok"], f"{what}: case {name}: frame total off the referee's, z {t['z']:.2f}"
    assert dsp["ok"], f"{what}: case {name}: binomial dispersion {dsp['chi2']:.0f} outside [{dsp['lo']:.0f}, {dsp['hi']:.0f}]"
    return rep


@pytest.mark.parametrize("name", list(AO_CASES))
def test_ao(name):
    orc = _orc()
    case = ao_case(name)
    print()
    for accel in ("octree", "list"):
        so = ao_recipe(name, accel)(OracleApi(orc))
        for seed in D.SEEDS:
            r = AR.ao_ref(orc, so, AO_FRAME, AO_FRAME, case["vp"], AO_S, seed, AO_K, radius=case["radius"])
            assert r.nhit == r.npaths
            check_ao(r.ao, name, f"ao_ref {accel} seed {seed}")


# ---------------------------------------------------------------- direct light (light_ref.py)
def _frame_point(a, b, c):
    """C + a u + b v + c n in the tilted floor's frame"""
    n, u, v = D._frame(D.NORMALS["tilted"])
    return D.C + a * u + b * v + c * n


def blocker(lo=0.0):
    """A Solid quad 1.5 above the floor, covering u > lo: seen from C it hides the half of a light that sits above C"""
    q = [_frame_point(lo, -2.0, 1.5), _frame_point(lo + 2.0, -2.0, 1.5), _frame_point(lo + 2.0, 2.0, 1.5), _frame_point(lo, 2.0, 1.5)]
    return ((np.array([q[0], q[1], q[2]], F32), (9, 9, 9)), (np.array([q[0], q[2], q[3]], F32), (9, 9, 9)))


def wall():
    """A large Solid quad 6 above the floor: behind every light of these cases"""
    q = [_frame_point(-5.0, -5.0, 6.0), _frame_point(5.0, -5.0, 6.0), _frame_point(5.0, 5.0, 6.0), _frame_point(-5.0, 5.0, 6.0)]
    return ((np.array([q[0], q[1], q[2]], F32), (90, 9, 9)), (np.array([q[0], q[2], q[3]], F32), (90, 9, 9)))


LIGHT_CASES = {
    "point": dict(extra="blocker", orig=(0.0, 0.0, 3.0), len2=0.0, S=1, K=1),
    "box": dict(extra="blocker", orig=(-0.5, -0.5, 3.0), len2=1.0, S=LIGHT_S, K=LIGHT_K),
    "horizon": dict(extra=None, orig=(2.0, 0.0, 0.0), len2=1.0, S=LIGHT_S, K=LIGHT_K),
    "wall": dict(extra="blocker+wall", orig=(-0.5, -0.5, 3.0), len2=1.0, S=LIGHT_S, K=LIGHT_K),
}
LIGHT_BIAS = 0.005


def light_extra(kind):
    return {None: (), "blocker": blocker(), "blocker+wall": blocker() + wall()}[kind]


def light_orig(case):
    """the light's corner: the case's (a, b, c) in the floor's frame, as float32 (what the renderer is given)"""
    return _frame_point(*case["orig"]).astype(F32)


def light_recipe(name, accel):
    return D.recipe("tilted", accel=accel, dome=False, extra=light_extra(LIGHT_CASES[name]["extra"]))


@functools.lru_cache(maxsize=None)
def light_case(name, unbounded=False):
    c = LIGHT_CASES[name]
    vp, o4, d4 = view(LIGHT_FRAME, LIGHT_FRAME)
    probe = D.Probe("tilted", dome=False, extra=light_extra(c["extra"]))
    p, d = probe.primary_hits(o4, d4)
    grid = p.reshape(LIGHT_FRAME, LIGHT_FRAME, 3)
    out = dict(c, probe=probe, grid=grid, d=d, vp=vp, o=light_orig(c), p=p)
    if c["len2"] > 0:
        rng = np.random.default_rng([20261019, 9, sorted(LIGHT_CASES).index(name), int(unbounded)])
        out["exp"] = D.light_expectation(probe, grid, d, c["S"] * c["K"], out["o"].astype(np.float64), c["len2"], LIGHT_BIAS, rng, unbounded)
    return out


# float32 at these coordinates (|x| <= 8, shadow rays 3 long): the record's unit normal is about six roundings deep per lane,
# point = rd t + ro is good to an ulp of 8 (9.5e-7, 3e-7 of the ray's length), the direction's normalisation is three roundings
# and the ordered dot four: about 18 x 2^-24 in all; 32 x 2^-24 leaves the rest to the jitter-free pixel centre being exact.
IRRADIANCE_TOL = 32 * 2.0 ** -24
# a shadow ray is decided when it crosses the blocker's plane further than this from the blocker's edge: the float32 hit point
# is good to 1e-5 (geom_ref's EPS_P); a hundred times that
LIGHT_EDGE_MARGIN = 1e-3


def check_point_light(shadow, irradiance, what):
    """Deterministic: per pixel shadow in {0, 1} and irradiance = n . dir where lit, both against float64 geometry"""
    case = light_case("point")
    probe, p = case["probe"], case["p"]
    nf = probe.n * -np.sign(float(case["d"][0] @ probe.n))
    L = case["o"].astype(np.float64)
    v = L[None] - p
    r = np.linalg.norm(v, axis=1)
    dirs = v / r[:, None]
    c = dirs @ nf
    # where the shadow ray crosses the blocker's plane (1.5 above the floor), in the floor's frame
    n, fu, fv = D._frame(D.NORMALS["tilted"])
    s = (1.5 - (p - D.C) @ n) / (dirs @ n)
    x = p + s[:, None] * dirs - D.C
    a, b = x @ fu, x @ fv
    edge = np.minimum.reduce([np.abs(a - 0.0), np.abs(a - 2.0), np.abs(b + 2.0), np.abs(b - 2.0)])
    inside = (a > 0) & (a < 2) & (b > -2) & (b < 2)
    decided = edge > LIGHT_EDGE_MARGIN
    want_shadow = np.where(inside, 0.0, 1.0)
    sh, ir = np.asarray(shadow, np.float64).reshape(-1), np.asarray(irradiance, np.float64).reshape(-1)
    und = 1.0 - decided.mean()
    err = np.abs(ir - np.where(inside, 0.0, c))[decided].max()
    print(f"  {what:28s} point light: undecided {und:.2%}, lit {int((want_shadow[decided] == 1).sum())}, shadowed "
          f"{int((want_shadow[decided] == 0).sum())}, max irradiance error {err:.3g} (tolerance {IRRADIANCE_TOL:.3g})")
    assert und <= 0.10 and (c > 0.5).all()
    assert min((want_shadow[decided] == 1).sum(), (want_shadow[decided] == 0).sum()) >= 100, "both answers must occur"
    assert np.isin(sh, (0.0, 1.0)).all()
    assert (sh[decided] == want_shadow[decided]).all(), f"{what}: {int((sh[decided] != want_shadow[decided]).sum())} decided pixels differ"
    assert err <= IRRADIANCE_TOL, f"{what}: irradiance off n . dir by {err:.3g}"


def check_box_light(shadow, irradiance, live_rays, name, what, unbounded=False):
    case = light_case(name, unbounded)
    e, n = case["exp"], case["S"] * case["K"]
    npix = LIGHT_FRAME * LIGHT_FRAME
    counts = D.ao_counts(shadow, n)
    tot = D.share_z(counts.sum(), n, e["visible"], e["m_ref"])
    dsp = D.binomial_dispersion(counts, n, e["visible"], e["m_ref"])
    irr = D.mean_z(np.asarray(irradiance, np.float64).reshape(-1), n, e["irr_mean"], e["irr_var"], e["m_ref"])
    line = (f"  {what:28s} {name}: visible {tot['observed'] / (n * npix):.4f} (referee {tot['expected'] / (n * npix):.4f}, z {tot['z']:+.2f})  "
            f"dispersion {dsp['chi2']:.0f} in [{dsp['lo']:.0f}, {dsp['hi']:.0f}] (df {dsp['df']})  irradiance {irr['observed']:.4f} "
            f"(referee {irr['expected']:.4f}, z {irr['z']:+.2f})")
    lv = None
    if live_rays is not None:
        lv = D.share_z(live_rays, n, e["live"], e["m_ref"])
        line += f"  live {lv['observed'] / (n * npix):.4f} (referee {lv['expected'] / (n * npix):.4f}, z {lv['z']:+.2f})"
    print(line)
    assert tot["ok"], f"{what}: {name}: shadow total, z {tot['z']:.2f}"
    assert dsp["df"] >= 0.9 * npix and dsp["ok"], f"{what}: {name}: dispersion {dsp}"
    assert irr["ok"], f"{what}: {name}: irradiance mean, z {irr['z']:.2f}"
    assert lv is None or lv["ok"], f"{what}: {name}: live rays, z {lv['z']:.2f}"
    return e


def run_light_ref(name, accel, seed, unbounded=False):
    orc = _orc()
    case = light_case(name)
    so = light_recipe(name, accel)(OracleApi(orc))
    return LR.light_ref(orc, so, LIGHT_FRAME, LIGHT_FRAME, case["vp"], case["S"], seed, case["K"], case["o"], case["len2"], LIGHT_BIAS,
                        flags=LR.UNBOUNDED if unbounded else 0), so


def test_point_light():
    print()
    for accel in ("octree", "list"):
        r, _ = run_light_ref("point", accel, 1)
        assert r.nhit == r.npaths
        check_point_light(r.shadow, r.irradiance, f"light_ref {accel}")


@pytest.mark.parametrize("seed", D.SEEDS)
def test_box_light_half_hidden(seed):
    print()
    for accel in ("octree", "list"):
        r, _ = run_light_ref("box", accel, seed)
        e = check_box_light(r.shadow, r.irradiance, r.nlive, "box", f"light_ref {accel} seed {seed}")
        assert 0.2 <= e["visible"].mean() <= 0.8 and (e["live"] == 1).all()


@pytest.mark.parametrize("seed", D.SEEDS)
def test_light_partly_below_the_horizon(seed):
    print()
    for accel in ("octree", "list"):
        r, _ = run_light_ref("horizon", accel, seed)
        e = check_box_light(r.shadow, r.irradiance, r.nlive, "horizon", f"light_ref {accel} seed {seed}")
        assert 0.2 <= e["live"].mean() <= 0.8, "the horizon must cut the light"
        assert r.nculled == r.ncand - r.nlive and r.ncand == r.npaths * LIGHT_K


def test_wall_behind_the_light():
    """Bounded: a wall beyond the light changes no bit.  RTMI_LIGHT_UNBOUNDED: everything is in shadow."""
    print()
    with_wall, _ = run_light_ref("wall", "octree", 1)
    without, _ = run_light_ref("box", "octree", 1)
    assert_bits_equal(with_wall.shadow, without.shadow, "shadow with and without the wall")
    assert_bits_equal(with_wall.irradiance, without.irradiance, "irradiance with and without the wall")
    unb, _ = run_light_ref("wall", "octree", 1, unbounded=True)
    assert unb.nhit == unb.npaths and (unb.shadow == 0).all() and (unb.irradiance == 0).all()
    check_box_light(with_wall.shadow, with_wall.irradiance, with_wall.nlive, "wall", "light_ref octree, bounded")


def test_light_samples_lie_in_the_box():
    """adj = point + dir r of every candidate of light_ref lies in [orig, orig + len2)^3 (to the float32 rounding of a point
    3 away: 1e-5), and the samples fill the box: each coordinate's mean and spread are a uniform's"""
    orc = _orc()
    case = light_case("box")
    so = light_recipe("box", "list")(OracleApi(orc))
    import features_ref as FR
    rows = list(range(LIGHT_FRAME))
    o4, d4, npix, n = FR.tile_rays(orc, LIGHT_FRAME, LIGHT_FRAME, case["vp"], case["S"], 2, 0, None, rows)
    tri, t, face, _ = so.trace(o4, d4)
    rec, _, _ = so.triangles()
    pixel = np.repeat(np.arange(npix, dtype=np.int64), n)
    sample = np.tile(np.arange(n, dtype=np.int64), npix)
    hit, o, dirs, r, c = LR.candidates(orc, 2, o4, d4, tri, t, face, rec[:, 3:6].astype(F32), pixel, sample, case["K"], case["o"], case["len2"], LIGHT_BIAS)
    point = o4[hit, :3].astype(np.float64) + t[hit, None].astype(np.float64) * d4[hit, :3]
    adj = point[:, None, :] + dirs[..., :3].astype(np.float64) * r[..., None]
    rel = (adj - case["o"].astype(np.float64)) / case["len2"]
    assert rel.min() >= -1e-5 and rel.max() < 1 + 1e-5, (rel.min(), rel.max())
    m = rel.reshape(-1, 3)
    z_mean = (m.mean(axis=0) - 0.5) / (1 / 12 / len(m)) ** 0.5
    cells = np.bincount((np.clip(m, 0, 1 - 1e-9) * 4).astype(int) @ np.array([16, 4, 1]), minlength=64)
    chi2 = float(((cells - len(m) / 64) ** 2 / (len(m) / 64)).sum())
    print(f"\n  light samples: {len(m)} in the box, mean z {z_mean.round(2).tolist()}, 4 x 4 x 4 grid chi2 {chi2:.1f} (threshold {D.chi2_threshold(63):.1f})")
    assert (np.abs(z_mean) <= D.Z_TWO_SIDED).all() and chi2 <= D.chi2_threshold(63)


# ---------------------------------------------------------------- self-checks: the referee can fail
WRONG = {"sphere-uniform r": dict(sampler=D.wrong_sphere), "unnormalised r": dict(sampler=D.wrong_unnormalised),
         "a reused word": dict(sampler=D.wrong_reused_word), "an uncentred U": dict(sampler=D.wrong_uncentred),
         "a hemisphere about -n": dict(flip_hemisphere=True), "one r for bounce 1 and 2": dict(sampler=D.WrongSameDrawEveryBounce)}


@pytest.mark.parametrize("wrong", list(WRONG))
@pytest.mark.parametrize("normal", list(D.NORMALS))
def test_self_check_wrong_samplers_are_reported(normal, wrong):
    """A renderer with this sampler, simulated in NumPy, fails the Lambert test (at maxdepth 3, where a second draw exists)"""
    ref = referee(normal, ("matte",), max(DEPTHS))
    rng = np.random.default_rng([5, sorted(WRONG).index(wrong)])
    end, face = D.chains(ref["probe"], ref["p"], ref["d"], ("matte",), 3, rng, **WRONG[wrong])
    obs = np.bincount(D.outcome(end, face, 3), minlength=D.UNDECODED + 1)
    exp = np.bincount(D.outcome(ref["end"], ref["face"], 3), minlength=D.UNDECODED + 1)
    r = D.two_sample_chi2(obs, exp)
    print(f"\n  {normal}, {wrong}: chi2 {r['chi2']:.0f}, threshold {r['threshold']:.1f}")
    assert not r["ok"]


@pytest.mark.parametrize("normal,wrong", [("facing", "an uncentred U"), ("tilted", "one r for bounce 1 and 2")])
def test_self_check_a_wrong_chain_length_is_reported(normal, wrong):
    """The rays-per-sample z-test can fail: with an uncentred U every first vector goes behind the floor that faces the camera
    and no second one does (3 rays per sample), and a second bounce that reuses the first vector never goes behind the surface
    again.  (A hemisphere about -n is NOT seen by this test: it re-hits the floor just as often; the histogram reports it.)"""
    ref = referee(normal, ("matte",), max(DEPTHS))
    rng = np.random.default_rng([7, sorted(WRONG).index(wrong)])
    end, face = D.chains(ref["probe"], ref["p"], ref["d"], ("matte",), 5, rng, **WRONG[wrong])
    rr, mine = D.rays(ref["end"], 5), D.rays(end, 5)
    z = D.z_test(mine.mean(), len(mine), rr.mean(), rr.var(), len(rr))
    print(f"\n  {wrong}: rays/N {mine.mean():.4f} (referee {rr.mean():.4f}), z {z['z']:+.1f}, threshold {z['threshold']:.2f}")
    assert not z["ok"]


@pytest.mark.parametrize("normal", list(D.NORMALS))
def test_self_check_a_correct_sampler_passes(normal):
    ref = referee(normal, ("matte",), max(DEPTHS))
    rng = np.random.default_rng(424242)
    end, face = D.chains(ref["probe"], ref["p"], ref["d"], ("matte",), max(DEPTHS), rng)
    print()
    for depth in DEPTHS:
        check_bins(D.outcome(end, face, depth), ref, depth, f"NumPy, another seed, maxdepth {depth}", dict(rays=int(D.rays(end, depth).sum())))
    check_independence(D.outcome(end, face, 2), ref, "NumPy, another seed")
    refz = referee("tilted", ("reflective", 1.0), max(FUZZ_DEPTHS))
    end, face = D.chains(refz["probe"], refz["p"], refz["d"], ("reflective", 1.0), 3, rng)
    check_bins(D.outcome(end, face, 3), refz, 3, "NumPy, another seed, fuzz 1.0")
    # a few hundred stray samples on faces the definition never reaches are reported (the pooled bin is a chi-square term)
    stray = D.outcome(end, face, 3).copy()
    rare = np.nonzero(np.bincount(D.outcome(refz["end"], refz["face"], 3), minlength=D.UNDECODED + 1)[:D.NFACES] == 0)[0]
    assert len(rare) >= 5
    stray[:200] = rare[0]
    with pytest.raises(AssertionError, match="chi2"):
        check_bins(stray, refz, 3, "self-check: 200 stray samples")
    end, face = D.chains(refz["probe"], refz["p"], refz["d"], ("reflective", 1.0), 3, rng, sampler=D.wrong_sphere)
    assert not D.two_sample_chi2(np.bincount(D.outcome(end, face, 3), minlength=83), np.bincount(D.outcome(refz["end"], refz["face"], 3), minlength=83))["ok"]


@pytest.mark.parametrize("wrong", ["sphere-uniform r", "unnormalised r", "a reused word", "an uncentred U"])
def test_self_check_fuzzy_cone_has_power(wrong):
    """the seven bins of the scattering 0.3 cone report every wrong random vector"""
    ref = referee("tilted", ("reflective", 0.3), max(FUZZ_DEPTHS))
    rng = np.random.default_rng([6, sorted(WRONG).index(wrong)])
    end, face = D.chains(ref["probe"], ref["p"], ref["d"], ("reflective", 0.3), 2, rng, **WRONG[wrong])
    r = D.two_sample_chi2(np.bincount(D.outcome(end, face, 2), minlength=D.UNDECODED + 1),
                          np.bincount(D.outcome(ref["end"], ref["face"], 2), minlength=D.UNDECODED + 1))
    print(f"\n  scattering 0.3, {wrong}: chi2 {r['chi2']:.0f}, threshold {r['threshold']:.1f}, bins {r['bins']}")
    assert not r["ok"]
    end, face = D.chains(ref["probe"], ref["p"], ref["d"], ("reflective", 0.3), 2, rng)
    check_bins(D.outcome(end, face, 2), ref, 2, "NumPy, another seed, fuzz 0.3", min_bins=FUZZ_MIN_BINS[0.3])


def test_self_check_neighbour_dependence_is_reported():
    """A frame whose pixel p + 1 repeats the draw of pixel p fails the neighbour contingency"""
    ref = referee("tilted", ("matte",), max(DEPTHS))
    rng = np.random.default_rng(99)
    end, face = D.chains(ref["probe"], ref["p"], ref["d"], ("matte",), 3, rng)
    b2 = D.outcome(end, face, 2).reshape(D.H, D.W).copy()
    b2[:, 1::2] = b2[:, 0::2]
    with pytest.raises(AssertionError, match="neighbouring pixels"):
        check_independence(b2.reshape(-1), ref, "self-check")


def test_self_check_ao_rays_sharing_a_draw_are_reported():
    case = ao_case("b")
    n = AO_S * AO_K
    rng = np.random.default_rng(31)
    shared, _ = D.ao_expectation(case["probe"], case["grid"], case["d"], n, case["radius"], 0.001, rng, shared_k=AO_K)
    rep = D.ao_report(shared, n, case["p_hat"], case["m_ref"])
    print(f"\n  K rays sharing one r: dispersion {rep['dispersion']['chi2']:.0f}, allowed up to {rep['dispersion']['hi']:.0f}")
    assert rep["dispersion"]["chi2"] > rep["dispersion"]["hi"]
    good, _ = D.ao_expectation(case["probe"], case["grid"], case["d"], n, case["radius"], 0.001, rng, shared_k=1)
    rep = D.ao_report(good, n, case["p_hat"], case["m_ref"])
    assert rep["total"]["ok"] and rep["dispersion"]["ok"], rep
    # a hemisphere about the wrong side of the floor sees no occluder: the total reports it
    probe = case["probe"]
    pts = D.pixel_points(case["grid"], rng, n).reshape(-1, 3)
    wrong_nf = probe.n * np.sign(float(case["d"][0] @ probe.n))
    vis = D.ao_visible(probe, pts, np.broadcast_to(wrong_nf, pts.shape), 1, 3.0, 0.001, rng)
    rep = D.ao_report(vis.reshape(-1, n).sum(axis=1), n, case["p_hat"], case["m_ref"])
    assert not rep["total"]["ok"]


def test_self_check_wrong_jitter_is_reported():
    rng = np.random.default_rng(8)
    w = h = 64
    u, v = rng.random(w * h * 4), rng.random(w * h * 4)
    margin = 1e-4
    good = D.jitter_report(u, v, w, h, 4, margin)
    assert D.jitter_ok(good), good
    # a pixel's jitter equal to its right neighbour's
    U, V = u.reshape(h, w, 4).copy(), v.reshape(h, w, 4).copy()
    U[:, 1::2], V[:, 1::2] = U[:, 0::2], V[:, 0::2]
    rep = D.jitter_report(U.reshape(-1), V.reshape(-1), w, h, 4, margin)
    assert rep["twins"] >= w * h // 2 and not rep["pixels"]["ok"]
    # u = v
    rep = D.jitter_report(u, u.copy(), w, h, 4, margin)
    assert not rep["corr"]["ok"] and not rep["grid"]["ok"]
    # every sample of a pixel the same
    U = np.repeat(u.reshape(h, w, 4)[:, :, :1], 4, axis=2)
    V = np.repeat(v.reshape(h, w, 4)[:, :, :1], 4, axis=2)
    rep = D.jitter_report(U.reshape(-1), V.reshape(-1), w, h, 4, margin)
    assert rep["twins"] > 0 and not rep["samples"]["ok"]
    # a distant pixel's draws repeated (a key that wraps): neither a neighbour nor the same pixel
    U, V = u.reshape(h, w, 4).copy(), v.reshape(h, w, 4).copy()
    U[h // 2:], V[h // 2:] = U[:h // 2], V[:h // 2]
    rep = D.jitter_report(U.reshape(-1), V.reshape(-1), w, h, 4, margin)
    assert rep["twins"] == 0 and not rep["all_pairs"]["ok"]
    # offsets that leave the pixel
    assert D.jitter_report(u * 1.01, v, w, h, 4, margin)["outside"] > 0


# ---------------------------------------------------------------- the shared edge of the floor
def beside_c():
    """the unit direction from the origin to a point 0.01 beside C on the tilted floor"""
    _, u, _ = D._frame(D.NORMALS["tilted"])
    t = D.C + 0.01 * u
    return t / np.linalg.norm(t)


def test_ray_at_the_shared_edge():
    """C lies on the edge the two floor triangles share.  The reference's edge test is strict, so a ray that meets the edge
    exactly hits neither triangle and goes on to the dome, in the octree and in the list alike; 0.01 beside C it hits the
    floor.  (A fact about the reference that the single-ray tests of tests/test_draw.py must know; the 256 x 256 frames have
    no ray on that edge: every sample decodes and test_lambert's black share is a half.)"""
    o4, d4 = np.zeros((2, 4), F32), np.zeros((2, 4), F32)
    d4[0, 2] = 1.0
    d4[1, :3] = beside_c()
    for accel in ("octree", "list"):
        tri, t, _, _ = oracle_scene("tilted", ("matte",), accel).trace(o4, d4)
        assert tri[0] > 2 and t[0] > 8, "the ray at the shared edge passes between the triangles"
        assert tri[1] in (1, 2) and abs(t[1] - 5.0) < 0.01


# ---------------------------------------------------------------- the builder: a triangle in a split plane
def test_floor_in_a_split_plane_is_listed_in_no_leaf():
    """A triangle parallel to an axis plane fails every face test of the reference's builder (face_contains_triangle divides by
    1 - (n1.n2)^2 = 0, raytrace.rs:652-653) and box_contains_point is strict (raytrace.rs:636-643): with the floor in z = 5 and
    root ([0, 0, 5], 9) every corner lies ON a split plane, so no leaf lists the floor, and the octree does not see it.  Both
    builders agree on this; the linear list still hits the floor.  (the probe's root box avoids it.)"""
    orc = _orc()
    from rust_raytrace_amd import raytrace as R
    quad = np.array([[(-1.5, -1.5, 5), (1.5, -1.5, 5), (1.5, 1.5, 5)], [(-1.5, -1.5, 5), (1.5, 1.5, 5), (-1.5, 1.5, 5)]], F32)

    def make(api, accel):
        s = api.scene()
        for t in quad:
            api.add_triangle(s, t, api.matte(D.FLOOR_RGB, 1.0), 0.0)
        for k, t in enumerate(D.dome_triangles()):
            api.add_triangle(s, t, api.solid(D.dome_rgb(k)), 0.0)
        s.populate_triangle_numbers()
        if accel == "octree":
            s.build_bounding_box([0.0, 0.0, 5.0], 9.0, *D.OCTREE)
        else:
            s.build_trivial_bounding_box([0.0, 0.0, 5.0], 9.0)
        return s

    so, sp = make(OracleApi(orc), "octree"), make(ProductApi(R), "octree")
    og, ot, orefs = so.tree_flatten()
    pg, pt, prefs = sp.tree()
    assert_bits_equal(og, pg, "box geometry")
    assert np.array_equal(ot, pt) and np.array_equal(orefs, prefs)
    assert len(orefs) > 80 and not np.isin(orefs, (1, 2)).any(), "the floor is listed somewhere"
    _, o4, d4 = view(16, 16)
    off = ~np.isclose(np.abs(o4[:, 0]), np.abs(o4[:, 1]), rtol=1e-3)   # not the rays aimed at the edge the two triangles share
    o4, d4 = o4[off], d4[off]
    tri, _, _, _ = so.trace(o4, d4)
    assert (tri > 2).all(), "the octree must miss the floor and hit the dome behind it"
    ltri, lt, _, _ = make(OracleApi(orc), "list").trace(o4, d4)
    assert np.isin(ltri, (1, 2)).all() and np.allclose(lt, 5.0, atol=0.01)
