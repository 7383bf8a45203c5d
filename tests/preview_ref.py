"""The definition of the shaded preview (rtmi_render_preview*, include/rtmi.h) in float32 NumPy, from the oracle as it is and
from the restatements of its three layers: FR.tile_rays makes the renderer's primary rays, Scene.trace their closest hits and
the secondary rays' closest hits, FR.features_from_hits the per-sample albedo and the feature buffers, AR.ao_rays the AO rays,
LR.candidates every light's candidates, OR.from_hits the occlusion rule.  The composition is per SAMPLE, every operation rounded
to float32 in the order the header states.  A plain helper module of tests/test_preview_cpu.py and tests/test_preview.py."""
from types import SimpleNamespace

import numpy as np

import ao_ref as AR
import features_ref as FR
import light_ref as LR
import occluded_ref as OR

F32 = np.float32
AMBIENT = (0.3, 0.3, 0.3)  # rtmi_preview_defaults
AO = dict(rays=4, radius=np.inf, bias=0.001)  # rtmi_ao_defaults
LIGHT = dict(orig=(0.0, 0.0, 0.0), len2=0.0, rays=4, flags=0, bias=0.005, color=(1.0, 1.0, 1.0))  # rtmi_light_defaults, white


def _occlusion(orc, so, o4, d4, tmax, occluded):
    """(answers, closest hits tri / t or None, the oracle's counters or None) of one set of secondary rays"""
    if occluded is not None:
        occ = np.asarray(occluded(o4, d4, tmax), np.uint8) if o4.shape[0] else np.zeros(0, np.uint8)
        return occ, None, None, None
    if o4.shape[0]:
        tri, t, _, cn = so.trace(o4, d4)
    else:
        tri, t, cn = np.zeros(0, np.uint32), np.zeros(0, F32), dict.fromkeys(orc.COUNTER_NAMES, 0)
    return OR.from_hits(tri, t, tmax), tri, t, cn


def preview_ref(orc, so, w, h, vp12, spp, seed, ambient=AMBIENT, ao=None, lights=(), sample0=0, nsamples=None, tile=None, trace=None,
                occluded=None):
    """Expected outputs of a preview call on oracle scene `so` and everything they were made from.  ao: None = the default AO,
    False = none (Ka = 0), or a dict over AO; lights: dicts over LIGHT.  trace(o4, d4) -> (tri, t, face) and occluded(o4, d4,
    tmax) -> bytes replace the oracle's closest hits and the rule on them (the not-bit-exact modes are held against the
    product's own rtmi_trace / rtmi_occluded).  Returns a namespace: color / albedo / normal (rows, w, 4), ids (rows, w), ao
    (rows, w) or None, shadow / irradiance (L, rows, w) or None; e (npix, n, 3) the per-sample colours, a (npix, n, 4) the
    per-sample albedo, f (paths that hit,), g (L, paths that hit); tri, face; npaths, nhit, nedge, n_ao, ao_occ, per light nculled /
    nlive / nocc (lists), rays (the stats' ray count); ao_rays / light_rays: the rays of each set as (o4, d4, tmax); cn_primary,
    cn_ao, cn_lights: the oracle's counters of each set (None with a custom trace / occluded)."""
    rows = list(range(h)) if tile is None else FR.tile_rows(tile)
    o4, d4, npix, n = FR.tile_rays(orc, w, h, vp12, spp, seed, sample0, nsamples, rows)
    cn_primary = None
    if trace is None:
        tri, t, face, cn_primary = so.trace(o4, d4)
    else:
        tri, t, face = trace(o4, d4)
    tri, face = np.asarray(tri), np.asarray(face)
    rec, _, surf = so.triangles()
    norm = rec[:, 3:6].astype(F32)
    pixel = np.repeat(np.array([r * w + c for r in rows for c in range(w)], np.int64), n)
    sample = np.tile(np.arange(sample0, sample0 + n, dtype=np.int64), npix)
    albedo, normal, ids = FR.features_from_hits(tri, t, face, rec, surf, npix, n)
    a = FR.features_from_hits(tri, t, face, rec, surf, npix * n, 1)[0]  # one sample per "pixel": the per-sample albedo itself
    hit = np.nonzero(tri != 0)[0]
    nh = len(hit)
    ao = dict(AO) if ao is None else (dict(AO, rays=0) if ao is False else dict(AO, **ao))
    Ka = int(ao["rays"])
    lights = [dict(LIGHT, **li) for li in lights]

    # the AO factor of every sample that hit
    f = np.ones(nh, F32)
    ao_plane, ao_rays, cn_ao, ao_occ = None, None, dict.fromkeys(orc.COUNTER_NAMES, 0), 0
    if Ka:
        ao_o, ao_d, _ = AR.ao_rays(orc, seed, o4, d4, tri, t, face, norm, pixel, sample, Ka, ao["bias"])
        tmax = np.full(ao_o.shape[0], ao["radius"], F32)
        occ, _, _, cn_ao = _occlusion(orc, so, ao_o, ao_d, tmax, occluded)
        v = Ka - np.asarray(occ, np.int64).reshape(nh, Ka).sum(axis=1)
        f = (v.astype(F32) * (F32(1.0) / F32(Ka))).astype(F32)
        ao_plane = AR.resolve(tri, occ, npix, n, Ka).reshape(len(rows), w)
        ao_rays, ao_occ = (ao_o, ao_d, tmax), int(np.asarray(occ).sum())

    # every light's g of every sample that hit, and its two planes
    g, shadow, irradiance, light_rays, cn_lights = [], [], [], [], []
    nculled, nlive, nocc = [], [], []
    for li in lights:
        K = int(li["rays"])
        _, o, dirs, r, c = LR.candidates(orc, seed, o4, d4, tri, t, face, norm, pixel, sample, K, li["orig"], li["len2"], li["bias"])
        with np.errstate(invalid="ignore"):
            live = c > F32(0.0)
        l_o, l_d, l_r = np.ascontiguousarray(o[live]), np.ascontiguousarray(dirs[live]), np.ascontiguousarray(r[live])
        tmax = None if int(li["flags"]) & LR.UNBOUNDED else l_r
        occ, _, _, cn = _occlusion(orc, so, l_o, l_d, tmax, occluded)
        lit = np.zeros(live.shape, bool)
        lit[live] = np.asarray(occ) == 0
        acc = np.zeros(nh, F32)
        with np.errstate(all="ignore"):
            for k in range(K):  # k order
                acc = np.where(lit[:, k], (acc + c[:, k]).astype(F32), acc)
            g.append((acc * (F32(1.0) / F32(K))).astype(F32))
        sh, ir = LR.resolve(tri, live, occ, c, npix, n, K)
        shadow.append(sh.reshape(len(rows), w))
        irradiance.append(ir.reshape(len(rows), w))
        light_rays.append((l_o, l_d, tmax))
        cn_lights.append(cn)
        nculled.append(int((~live).sum()))
        nlive.append(int(live.sum()))
        nocc.append(int(np.asarray(occ).sum()))

    # the composition, per sample and per channel: L = ambient * f; L = L + colour_l * g_l; e = a * L; a miss: e = a
    e = a[:, :3].copy()
    with np.errstate(all="ignore"):
        L = (np.asarray(ambient, F32)[None, :] * f[:, None]).astype(F32)
        for li, gl in zip(lights, g):
            L = (L + (np.asarray(li["color"], F32)[None, :] * gl[:, None]).astype(F32)).astype(F32)
        e[hit] = (a[hit, :3] * L).astype(F32)
        e = e.reshape(npix, n, 3)
        acc = np.zeros((npix, 3), F32)
        for s in range(n):  # sample order
            acc = (acc + e[:, s]).astype(F32)
        color = np.zeros((npix, 4), F32)
        color[:, :3] = (acc * (F32(1.0) / F32(n))).astype(F32)
    nr = len(rows)
    return SimpleNamespace(
        color=color.reshape(nr, w, 4), albedo=albedo.reshape(nr, w, 4), normal=normal.reshape(nr, w, 4), ids=ids.reshape(nr, w),
        ao=ao_plane, shadow=np.stack(shadow) if lights else None, irradiance=np.stack(irradiance) if lights else None,
        e=e, a=a.reshape(npix, n, 4), f=f, g=np.stack(g) if lights else np.zeros((0, nh), F32), tri=tri, face=face,
        npaths=npix * n, nhit=nh, nedge=int(((face[hit] & 2) != 0).sum()), n_ao=nh * Ka, ao_occ=ao_occ, nculled=nculled, nlive=nlive,
        nocc=nocc, rays=npix * n + nh * Ka + sum(nlive), ao_rays=ao_rays, light_rays=light_rays, cn_primary=cn_primary, cn_ao=cn_ao,
        cn_lights=cn_lights)
