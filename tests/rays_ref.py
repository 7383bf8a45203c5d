"""Expectations for the explicit-ray calls (rtmi_render_rays*, rtmi_trace_device; include/rtmi.h defines them) from the oracle
and NumPy alone.  The oracle pins the call without a restatement of the shading: orc.primary_rays returns the renderer's own
rays in [pixel][sample] order with RNG key (row * w + col, sample), and those rays fed back with those keys must reproduce
Scene.render bit for bit.  What is restated here is only what the header spells out: the fold of colours to group means, vunit
and the colour of a path of depth 1.  A plain helper module of tests/test_rays_cpu.py and tests/test_rays.py."""
import numpy as np

from features_ref import SKY, features_from_hits  # noqa: F401  (features_from_hits: the guides, re-exported)

F32 = np.float32

# test 1: the canonical view, centred rays (1 spp); test 2: jittered rays (4 spp); both with seed 7 at depth 5
CENTRED = dict(w=33, h=33, spp=1, seed=7, maxdepth=5)
JITTERED = dict(w=24, h=24, spp=4, seed=7, maxdepth=5)
# test 3: a second camera inside the scene looking elsewhere, rendered with test 2's seed and depth (one call has one seed)
SECOND = dict(w=20, h=16, spp=2, seed=7, maxdepth=5, size=(1.0, 0.7), pos=(1.5, 2.0, 1.0), aim=(-0.2, -0.3, 1.0), fov=70.0, roll=0.3)
# test 5: every scene kind at this size
KINDS = dict(w=16, h=16, spp=2, seed=3, maxdepth=4)


def camera_keys(w, h, spp):
    """(pixel, sample) of the renderer's rays in [pixel][sample] order: (h * w * spp, 2) uint32."""
    pix = np.repeat(np.arange(h * w, dtype=np.uint32), spp)
    smp = np.tile(np.arange(spp, dtype=np.uint32), h * w)
    return np.ascontiguousarray(np.stack([pix, smp], axis=1))


def camera_rays(orc, vp12, w, h, spp, seed, **_):
    """The renderer's own primary rays of a view and their RNG keys: (o4, d4, keys)."""
    o4, d4 = orc.primary_rays(w, h, np.asarray(vp12, F32), spp, seed)
    return o4, d4, camera_keys(w, h, spp)


def second_viewport(orc):
    c = SECOND
    return orc.create_viewport(c["w"], c["h"], c["size"], np.array(c["pos"], F32), orc.unit(list(c["aim"])), c["fov"], c["roll"])


def zero_component_rays(d4):
    d = np.asarray(d4, F32).reshape(-1, 4)
    return int(((d[:, :3] == 0).any(axis=1)).sum())


def fold(color, group):
    """mean[g]: acc = 0.f; acc = acc + color[g G + s] in s order; acc * (1.f / (float)G), all in float32."""
    c = np.asarray(color, F32).reshape(-1, group, 4)
    acc = np.zeros((c.shape[0], 4), F32)
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(group):
            acc = acc + c[:, s]
        return (acc * (F32(1.0) / F32(group))).astype(F32)


def vunit(d4):
    """make_ray's direction: the ordered four-lane dot seeded with +0, r = sqrt(.), v * (1.f / r), all in float32."""
    d = np.asarray(d4, F32).reshape(-1, 4)
    with np.errstate(all="ignore"):
        dot = np.zeros(d.shape[0], F32)
        for k in range(4):
            dot = (dot + d[:, k] * d[:, k]).astype(F32)
        inv = (F32(1.0) / np.sqrt(dot).astype(F32)).astype(F32)
        return np.ascontiguousarray((d * inv[:, None]).astype(F32))


def depth1_color(tri, face, kinds, surf):
    """The colour of a path of depth 1 from its ray's closest hit: the sky for a miss, black for an edge face, the surface's
    colour for Solid, and for Matte / Reflective mix_color(color, black, alpha) = color * (1.f - alpha) + 0 * alpha (the
    bounce ray would have depth 0, which is black).  kinds / surf as Scene.triangles() returns them."""
    tri = np.asarray(tri, np.uint32)
    face = np.asarray(face, np.uint32)
    out = np.zeros((tri.shape[0], 4), F32)
    col = np.zeros((tri.shape[0], 4), F32)
    col[:, :3] = surf[tri, 0:3].astype(F32)
    alpha = surf[tri, 3].astype(F32)
    mixed = (col * (F32(1.0) - alpha)[:, None] + np.zeros_like(col) * alpha[:, None]).astype(F32)
    solid = kinds[tri] == 0
    out[:] = np.where(solid[:, None], col, mixed)
    out[(face & 2) != 0] = 0.0
    out[tri == 0] = np.array([SKY[0], SKY[1], SKY[2], 0.0], F32)
    return out


def edge_case_rays():
    """The rays of tests/test_gpu_parity.py::test_trace_edge_case_rays (for the scene of conftest.recipe_axis_box): origins on
    planes, axis-parallel and zero-component directions, NaN / inf components, a NaN lane 3, a zero direction."""
    rays = []
    for ox in (-1.0, -0.5, 0.0, 0.25, 1.0):
        for oy in (-1.0, 0.0, 0.25, 0.5):
            for dvec in ((0, 0, 1), (0, 0, -1), (1, 0, 0), (0, 1, 0), (0, -1, 0), (-1, 0, 0), (0.6, 0, 0.8), (0, 0.6, 0.8),
                         (-0.0, 0.0, 1.0), (1e-30, 0, 1), (0.57735026, 0.57735026, 0.57735026)):
                rays.append(((ox, oy, 3.5, 0.0), (*dvec, 0.0)))
                rays.append(((ox, oy, 5.0, 0.0), (*dvec, 0.0)))
                rays.append(((-1.0, oy, 4.0, 0.0), (*dvec, 0.0)))
    rays += [((0, 0, 0, 0), (np.nan, 0, 1, 0)), ((np.nan, 0, 0, 0), (0, 0, 1, 0)), ((0, 0, 0, np.nan), (0, 0, 1, 0)),
             ((0, 0, 0, 0), (0, 0, 1, np.nan)), ((np.inf, 0, 0, 0), (0, 0, 1, 0)), ((0, 0, 0, 0), (0, 0, 0, 0))]
    return np.array([r[0] for r in rays], F32), np.array([r[1] for r in rays], F32)


def arbitrary_rays(nrandom=1000, seed=11):
    """Test 6's set for the axis-box scene (root box: centre (0, 0, 4), half edge 4): random origins in the box with random unit
    directions, then the edge-case rays.  nrandom + 666 rays: more than one block, no multiple of 256."""
    rng = np.random.default_rng(seed)
    o4 = np.zeros((nrandom, 4), F32)
    d4 = np.zeros((nrandom, 4), F32)
    o4[:, :3] = rng.uniform(-4, 4, (nrandom, 3)) + np.array([0, 0, 4.0])
    d = rng.normal(size=(nrandom, 3))
    d4[:, :3] = d / np.linalg.norm(d, axis=1, keepdims=True)
    eo, ed = edge_case_rays()
    return np.ascontiguousarray(np.concatenate([o4, eo])), np.ascontiguousarray(np.concatenate([d4, ed]))


def unnormalised(d4, seed=5):
    """Directions of every length between 1/8 and 8 times the given ones (test 7)."""
    rng = np.random.default_rng(seed)
    d = np.asarray(d4, F32).reshape(-1, 4)
    return np.ascontiguousarray((d * rng.uniform(0.125, 8.0, (d.shape[0], 1)).astype(F32)).astype(F32))
