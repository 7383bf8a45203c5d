"""No GPU: the definition of environment sampling at matte hits (include/rtmi.h "SAMPLING THE ENVIRONMENT") as tests/envlight_ref.py
restates it.  First the restatement's own footing -- its vectorised Philox is the oracle's rng_block, and without the sampling its
loop is env_ref.path_trace's, bit for bit -- then the properties the definition must have: (a) its image is the plain render's in
expectation, (b) pb is the density of the reference's own Matte bounce, (c) pe integrates to 1 over the sphere, (d) the sampler
table's edge cases.  The statistical assertions run at draw_ref's false-alarm probability, corrected for the number of comparisons."""
from types import SimpleNamespace

import numpy as np
import pytest

import conftest as CT
import draw_ref as DR
import env_ref as ER
import envlight_ref as EL
import features_ref as FR
from glass_ref import keys_of
from rays_ref import vunit

F32 = np.float32
SUN = dict(sun_dir=(-0.75, 0.25, 0.6), sun_cos=0.95, sun_color=(30.0, 24.0, 16.0))  # a WIDE sun: 18 degrees of radius
# the smallest sun the unbiasedness test can afford on the CPU: 8 degrees of radius (0.5 % of the sphere, about 20 of the 64 x 64
# texels), ten times brighter.  A Matte bounce finds it about once in 100 draws, so a pixel of 2 048 plain samples holds some 20
# sun hits and its variance estimate is usable; a sun of 1 degree would need 64 times the samples for the same footing.
SUN8 = dict(sun_dir=(-0.75, 0.25, 0.6), sun_cos=0.9903, sun_color=(300.0, 240.0, 160.0))


def _orc():
    from oracle import orc
    return orc


@pytest.fixture(scope="module")
def teapot():
    return CT.recipe_canonical()(CT.OracleApi(_orc()))


def _rotation():
    a, b = 0.7, -0.4
    ra = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    rb = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    return (ra @ rb).astype(F32)


# ---------------------------------------------------------------- the restatement's footing
def test_vectorised_philox_is_the_oracles_rng_block():
    orc = _orc()
    rng = np.random.default_rng(0)
    px, sm = rng.integers(0, 2 ** 32, 40), rng.integers(0, 2 ** 31, 40)
    for blk in (0, 1, 7, EL.ENVLIGHT_BLOCK | 3):
        for seed in (1, 2 ** 40 + 12345):
            w = EL.rng_blocks(seed, px, sm, blk)
            for i in range(len(px)):
                assert np.array_equal(w[i], orc.rng_block(seed, int(px[i]), int(sm[i]), blk))
    assert EL.unit_f32(np.array([0xFFFFFFFF], np.uint32))[0] == F32(orc.u32_to_unit_f32(0xFFFFFFFF)) < 1


def test_without_the_sampling_the_loop_is_env_refs(teapot):
    orc = _orc()
    env = SimpleNamespace(table=ER.sky_table(8, SUN), frame=None)
    vo = orc.canonical_viewport(24, 24)
    want = ER.render(orc, teapot, vo, 24, 24, 2, 5, 5, env=env)
    got = EL.render(orc, teapot, vo, 24, 24, 2, 5, 5, env, nee=False)
    CT.assert_bits_equal(got.image, want.image, "nee=False against env_ref.render")
    assert got.rays == want.rays and got.nlive == 0
    nee = EL.render(orc, teapot, vo, 24, 24, 2, 5, 5, env)
    assert nee.rays == want.rays and nee.pt.passes == want.passes  # the paths do not move
    assert nee.nlive > 0 and not np.array_equal(nee.image, want.image)


# ---------------------------------------------------------------- (a) the definition is unbiased
W = H = 16     # a frame of 256 pixels
N = 1024       # samples per pixel and estimator (2 * N under the sun of 8 degrees)


def _pixel_stats(so, env, seed, nee, origin="bounce", N=N):
    orc = _orc()
    rows = list(range(H))
    o4, d4, npix, n = FR.tile_rays(orc, W, H, orc.canonical_viewport(W, H), N, seed, 0, None, rows)
    pixel, sample = keys_of(W, rows, n, 0)
    pt = EL.path_trace(so, o4, d4, pixel, sample, 4, seed, env, nee=nee, origin=origin)
    return pt.color.reshape(npix, n, 4)[..., :3].astype(np.float64), pt


def _max_z(a, b):
    """The largest two-sample |z| over pixels and channels of sample sets a (npix, na, 3), b (npix, nb, 3); lanes in which neither
    set varies must agree exactly"""
    va, vb = a.var(1, ddof=1) / a.shape[1], b.var(1, ddof=1) / b.shape[1]
    diff = a.mean(1) - b.mean(1)
    flat = (va + vb) == 0
    assert (diff[flat] == 0).all()
    return float(np.abs(diff[~flat] / np.sqrt((va + vb)[~flat])).max())


@pytest.mark.parametrize("case", ["sky, sun of 8 degrees radius", "random table, n = 11, rotated"])
def test_the_image_is_the_plain_renders_in_expectation(teapot, case):
    """The sky's sun is as small as the CPU affords (SUN8 above says why not smaller); the random table concentrates its light in
    single texels.  Per pixel and channel, the mean of N envlight samples (seed 1) against the mean of N plain samples (seed 2: independent
    draws), z = difference / sqrt(var_a / N + var_b / N), two-sided at 1e-6 over all 3 * 256 comparisons.  The condition on N: the
    plain reference's own two halves must pass the same comparison at the same bound -- with too few samples a pixel whose plain
    samples never found the sun has a variance estimate that is too small, and that comparison fails first."""
    if case.startswith("sky"):
        env, n_s = SimpleNamespace(table=ER.sky_table(64, SUN8), frame=None), 2 * N
    else:
        n_s = N
        env = SimpleNamespace(table=(np.random.default_rng(3).random((11, 11, 3)) ** 8 * 200.0).astype(F32), frame=_rotation())
        assert EL.frame_is_rotation(env.frame)
    bound = DR.z_quantile(DR.P_FALSE / (2 * 3 * W * H))
    a, pa = _pixel_stats(teapot, env, 1, True, N=n_s)
    b, pb_ = _pixel_stats(teapot, env, 2, False, N=n_s)
    assert sum(pa.nlive) > 10000 and sum(pa.occluded) > 1000 and sum(pa.nlive) - sum(pa.occluded) > 1000
    z_half = _max_z(b[:, :n_s // 2], b[:, n_s // 2:])
    z = _max_z(a, b)
    print(f"{case}: max |z| envlight vs plain {z:.2f}, plain half vs half {z_half:.2f}, bound {bound:.2f}; "
          f"mean variance per sample {a.var(1).mean():.4f} (envlight) {b.var(1).mean():.4f} (plain)")
    assert z_half <= bound
    assert z <= bound
    # ... and over the whole frame, where a small common bias would add up
    tot_a, tot_b = a.mean(1).sum(), b.mean(1).sum()
    se = np.sqrt((a.var(1, ddof=1) / n_s).sum() + (b.var(1, ddof=1) / n_s).sum())
    assert abs(tot_a - tot_b) <= DR.Z_TWO_SIDED * se


def test_a_shadow_ray_from_the_normal_offset_would_be_biased(teapot):
    """Why o = point + s * bias: the reference's Matte bounce starts at point + rv * 0.001f, behind the surface for half of the
    draws.  The same estimator with its shadow rays started at point + n * bias sees another scene and fails the comparison."""
    env = SimpleNamespace(table=ER.sky_table(32, SUN), frame=None)
    b, _ = _pixel_stats(teapot, env, 2, False)
    a, _ = _pixel_stats(teapot, env, 1, True, origin="normal")
    assert _max_z(a, b) > DR.z_quantile(DR.P_FALSE / (2 * 3 * W * H))


# ---------------------------------------------------------------- (b) pb is the bounce's density
def test_pb_is_the_density_of_the_references_matte_bounce():
    """For random normals n and directions d: the share of 4 * 10^6 bounces unit(n + random_vec) inside a cap of 0.06 rad around d
    against pb(n, d, s(d)) times the cap's solid angle, a binomial z-test per direction (the density varies by under 2 % across
    such a cap, which the tolerance on top of the z bound covers)"""
    rng = np.random.default_rng(11)
    M, cap = 4_000_000, 0.06
    omega_cap = 2 * np.pi * (1 - np.cos(cap))
    bound = DR.z_quantile(DR.P_FALSE / (2 * 3 * 8))
    for _ in range(3):
        n = vunit(np.concatenate([rng.normal(size=(1, 3)), np.zeros((1, 1))], axis=1).astype(F32))
        w = rng.integers(0, 2 ** 32, (M, 4), dtype=np.uint64).astype(np.uint32)
        rv = EL.random_vec(w)
        d = vunit((n + rv).astype(F32)).astype(np.float64)[:, :3]
        for k in range(8):
            t = d[k * 1000]
            share = float((d @ t > np.cos(cap)).mean())
            d4 = np.zeros((1, 4), F32)
            d4[0, :3] = t
            d4 = vunit(d4)
            p = float(EL.pb(n, d4, EL.bounce_s(n, d4))[0]) * omega_cap
            z = (share - p) / np.sqrt(p * (1 - p) / M)
            assert abs(share - p) <= bound * np.sqrt(p * (1 - p) / M) + 0.03 * p, (n, t, share, p, z)
    # the weights of the two strategies sum to one wherever both are defined
    pbv, pev = F32(0.37), F32(2.5)
    assert abs(float(EL.balance(pbv, pev)) + float(EL.balance(pev, pbv)) - 1.0) < 1e-6
    # ... pb is 0 below the horizon and s(d) inverts the bounce
    n = vunit(np.array([[0.2, -0.4, 0.9, 0.0]], F32))
    below = vunit(np.array([[0.0, 0.0, -1.0, 0.0]], F32))
    assert EL.pb(n, below, EL.bounce_s(n, below))[0] == 0
    rv = EL.random_vec(rng.integers(0, 2 ** 32, (1000, 4), dtype=np.uint64).astype(np.uint32))
    nn = np.broadcast_to(n, rv.shape)
    d = vunit((nn + rv).astype(F32))
    assert np.abs(EL.bounce_s(nn, d) - rv).max() < 1e-4 * max(1.0, float(1 / ER.vdot(nn, d).min()))


# ---------------------------------------------------------------- (c) pe integrates to 1
@pytest.mark.parametrize("n", [1, 2, 5, 64])
@pytest.mark.parametrize("frame", ["identity", "rotated"])
def test_pe_integrates_to_one_over_the_sphere(n, frame):
    """Midpoint quadrature over the octahedral square itself (K x K points per texel, each with the solid angle dpx dpy / r^3 of
    its cell): pe is piecewise smooth on exactly these cells, so the rule converges fast; 1e-3 covers its error at K = 8 and
    float32's in pe."""
    table = (np.random.default_rng(n).random((n, n, 3)) ** 6 * 1e3).astype(F32)
    fr = None if frame == "identity" else _rotation()
    smp = EL.sampler_of(SimpleNamespace(table=table, frame=fr))
    K = max(8, 256 // n)
    m = n * K
    p = (np.arange(m) + 0.5) / m * 2 - 1
    px, py = np.meshgrid(p, p)
    z = 1 - np.abs(px) - np.abs(py)
    low = z < 0
    sg = lambda v: np.where(v >= 0, 1.0, -1.0)
    fx, fy = np.where(low, (1 - np.abs(py)) * sg(px), px), np.where(low, (1 - np.abs(px)) * sg(py), py)
    v = np.stack([fx, fy, z], axis=-1).reshape(-1, 3)
    r = np.linalg.norm(v, axis=1)
    dm = v / r[:, None]                                   # map-space unit directions
    R = np.eye(3) if fr is None else fr.astype(np.float64)
    d4 = np.zeros((len(dm), 4), F32)
    d4[:, :3] = dm @ R                                    # world = R^T m
    d4 = vunit(d4)
    domega = (2.0 / m) ** 2 / r ** 3
    total = float((EL.pe(smp, d4).astype(np.float64) * domega).sum())
    assert abs(domega.sum() - 4 * np.pi) < 1e-3 * 4 * np.pi
    assert abs(total - 1.0) < 1e-3, total
    assert EL.pe(smp, d4).min() > 0


# ---------------------------------------------------------------- (d) the table
def test_sampler_table_cases():
    cases = EL.table_cases()
    for name, t in cases.items():
        q, total = EL.sampler_table(t)
        n = t.shape[0]
        assert q.shape == (n, n) and q.dtype == np.uint32 and q.min() >= 1 and q.max() <= 1048577, name
        assert total == sum(int(x) for x in q.reshape(-1)), name
    assert np.array_equal(EL.sampler_table(cases["hdr1"])[0], [[1048577]])
    q, total = EL.sampler_table(cases["all-zero map"])
    assert (q == 1).all() and total == 25
    q, _ = EL.sampler_table(cases["zero texels"])
    assert q[1, 2] == 1 and (q[4] == 1).all() and (q[:4] > 1).sum() >= 15
    q, _ = EL.sampler_table(cases["negative texels"])
    assert q[0, 0] == 1 and q[3, 1] == 1 and q[2, 3] > 1      # lum decides, not the lanes
    q, _ = EL.sampler_table(cases["NaN and inf texels"])
    assert all(q[j, i] == 1 for j, i in ((0, 1), (1, 1), (2, 2), (3, 3), (4, 0), (4, 4)))
    assert q.max() >= 1048576                                  # the dark texels do not dim the rest
    q, total = EL.sampler_table(cases["one bright texel"])
    assert q[3, 1] >= 1048576 and total == int(q[3, 1]) + 24
    # the weights follow lum / r^3: a texel of a uniform map covers the least solid angle at a pole of the octahedron (r = 1), more
    # at the middle of an edge, the most at the centre of a face (r^2 = 1/3)
    q, _ = EL.sampler_table(np.ones((64, 64, 3), F32))
    assert q[32, 32] < q[32, 16] < q[42, 42] and q.max() >= 1048576 and abs(int(q[0, 0]) - int(q[32, 32])) <= 1
    # C and the draw: T = 0 is the first texel, T = total - 1 the last, and a texel's share of the draws is q / total
    smp = EL.sampler_of(SimpleNamespace(table=cases["hdr5"], frame=None))
    w = np.array([[0, 0, 0, 0], [0xFFFFFFFF, 0xFFFFFFFF, 0, 0]], np.uint32)
    T, k = EL.sample_texel(smp, w)
    assert T[0] == 0 and k[0] == 0 and T[1] == smp.total - 1 and k[1] == 24
    w = np.random.default_rng(5).integers(0, 2 ** 32, (200000, 4), dtype=np.uint64).astype(np.uint32)
    _, k = EL.sample_texel(smp, w)
    share = np.bincount(k, minlength=25) / len(k)
    p = smp.q.reshape(-1) / smp.total
    assert (np.abs(share - p) <= DR.z_quantile(DR.P_FALSE / 50) * np.sqrt(p * (1 - p) / len(k))).all()


def test_sampled_directions_land_in_their_texel_and_follow_pe():
    """The direction drawn in texel (i, j) maps back to (i, j) under pe's own mapping (up to a neighbour when the point lies
    within rounding of a texel edge), also in a rotated frame"""
    for fr in (None, _rotation()):
        smp = EL.sampler_of(SimpleNamespace(table=EL.table_cases()["hdr5"], frame=fr))
        w = np.random.default_rng(9).integers(0, 2 ** 32, (20000, 4), dtype=np.uint64).astype(np.uint32)
        omega, i, j = EL.sample_dir(smp, w)
        assert np.abs(np.linalg.norm(omega[:, :3].astype(np.float64), axis=1) - 1).max() < 1e-6
        want = (smp.q[j, i].astype(np.float64) / smp.total) * (25 / 4.0)
        mx = np.abs(omega[:, :3].astype(np.float64) @ (np.eye(3) if fr is None else fr.astype(np.float64)).T).sum(1)
        got = EL.pe(smp, omega).astype(np.float64) * mx ** 3
        assert (np.abs(got - want) <= 1e-4 * want).mean() > 0.999


def test_invalid_arguments_are_refused_before_the_scene_is_used():
    EL.check_invalid_arguments()
