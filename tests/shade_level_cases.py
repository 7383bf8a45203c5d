"""Rows, scenes and expectations of the mode x level matrix (tests/test_shade_level_matrix_cpu.py pins the conditions on the inputs,
tests/test_shade_level_matrix.py holds the product to them).  One row per shading level above PLAIN -- glass, env, smooth, tex, nmap
-- and `all`, the normal-map patch with glass, mirrors, matte, solid, mapped and unmapped triangles under vertex normals and a sky.

Every expectation comes from tests/nmap_ref.py, the top of the restatement ladder, on the oracle's closest hits, records and RNG:
  expect(row)        one render at S samples; its sample colours (S, H, W, 4); the tolerance test_adaptive.pick_tol picks from
                     them; test_adaptive.replay's counts, accum, sumsq, passes, unconverged; out = accum * (1 / count) per pixel;
                     the refinement passes' pixel lists; the rays of exactly the (pixel, sample) pairs with sample < count.
  expect_tile        the same over the rows of a striped tile.
  pass_refs          the uneven progressive passes [0,1) [1,3) [3,8), each continued from the one before.
  view_refs          three views with three seeds.
  rays_case          the frame's primary rays and keys under a fixed permutation, and the same rays un-keyed in groups of G.
The product's own walk_samples is never the source of a colour.  plan_batches restates the batch plan of a tile call
(rtmi_device.hip, plan_tile) so that the CPU test can show that a tuning cuts a pass into several batches.  `plain` (the canonical
scene with nothing set) is no row of the matrix: the workspace test renders it between two textured levels."""
import functools
from types import SimpleNamespace

import numpy as np

import conftest as CT
import denoise_var_ref as DV
import env_ref as ER
import features_ref as FR
import glass_cases as GC
import nmap_cases as NC
import nmap_ref as NR
import smooth_cases as SC
import smooth_ref as SR
import tex_cases as TC
import tex_ref as TR
from camera_ref import fold
from test_adaptive import pick_tol, replay

F32 = np.float32
W = H = 32
S, M, P, DEPTH, SEED = 8, 2, 2, 5, 5
ROWS = ("glass", "env", "smooth", "tex", "nmap", "all")
BELOW = {"smooth": "env", "tex": "smooth", "nmap": "tex", "all": "nmap"}  # the row below each row above env
LEVEL_KEY = {"env": "env", "smooth": "normals", "tex": "tex", "nmap": "nm"}  # the keyword that makes the row's level
GLASSY = ("glass", "all")
WRAPPED = ("tex", "nmap", "all")  # the rows of the adaptive denoised wrapper
NTEAPOT = 6320  # triangles 1 .. 6320 of the canonical scene are the teapot's
LO, SCALE = (-1.7, -0.4, 3.1), 0.9  # tests/test_tex.py's box projection of the teapot
HEIGHT_SCALE = 2.0  # tests/test_nmap.py's height field
SUN = dict(sun_dir=(-0.75, 0.25, 0.6), sun_cos=0.8, sun_color=(30.0, 24.0, 16.0))
STRIPED = (1, 16, 4, 8)  # rows 1-4, 9-12, 17-20, 25-28
PASSES = ((0, 1), (1, 2), (3, 5))  # (sample0, nsamples): [0,1) [1,3) [3,8)
SMALL = {"streams": 4, "batch_paths": 40, "subtile_min_paths": 1}
ONE_STREAM = {"streams": 1, "batch_paths": 500}
VIEW_SPP, VIEW_BATCH = 4, 600
THIRD_VIEW = dict(GC.SIDE_VIEW, pos=(0.5, 1.0, 1.5), aim=(0.1, -0.1, 1.0), fov=70.0)  # tests/test_nmap.py's second camera
RAYS_BATCH, G = 500, 4


def _orc():
    from oracle import orc
    return orc


def _R():
    from rust_raytrace_amd import raytrace as R
    return R


# ---------------------------------------------------------------- the scenes, on both sides
def _recipe(name):
    return {"glass": GC.recipe_slab, "all": NC.recipe_patch}.get(name, CT.recipe_canonical)()


def _sky():
    return SimpleNamespace(table=ER.sky_table(8, SUN), frame=None)


def _teapot_normals(rec):
    out = np.zeros((len(rec), 3, 3), F32)
    out[1:1 + NTEAPOT] = SR.generate(rec[1:1 + NTEAPOT, 20:29], rec[1:1 + NTEAPOT, 3:6], 0.5)
    return out


def _teapot_textures(rec, images):
    uvs, tot = np.zeros((len(rec), 3, 2), F32), np.zeros(len(rec), np.uint32)
    uvs[1:1 + NTEAPOT] = TR.project(rec[1:1 + NTEAPOT, 20:29], rec[1:1 + NTEAPOT, 3:6], LO, SCALE)
    tot[1:1 + NTEAPOT] = 1
    return TR.textures(images, uvs, tot)


def _teapot_maps(n):
    nm = np.zeros(n, np.uint32)
    nm[1:1 + NTEAPOT] = 2
    return NR.maps(nm)


@functools.lru_cache(maxsize=None)
def row(name):
    """The oracle's side of a row: so (the oracle scene), kw (the keywords of nmap_ref.render / path_trace), vo (the canonical
    viewport's 12 floats), normals / tex / nm (None where the row has none) for the guides"""
    orc = _orc()
    so = _recipe(name)(CT.OracleApi(orc))
    rec = so.triangles()[0]
    kw = {}
    if name in ("env", "tex", "nmap", "all"):
        kw["env"] = _sky()
    if name in ("smooth", "tex", "nmap"):
        kw["normals"] = _teapot_normals(rec)
    if name == "tex":
        kw["tex"] = _teapot_textures(rec, [TC.images()[3]])
    if name == "nmap":
        kw["tex"] = _teapot_textures(rec, [TC.images()[3], NR.from_height(NC.heights(), HEIGHT_SCALE)])
        kw["nm"] = _teapot_maps(len(rec))
    if name == "all":
        n = len(rec)
        uvs, tot = NC.patch_uvs(n)
        nrm = np.zeros((n, 3, 3), F32)
        nrm[:SC.NTRI_PATCH + 1] = SC.patch_normals(rec)[:SC.NTRI_PATCH + 1]
        kw.update(normals=nrm, tex=TR.textures(NC.images(), uvs, tot), nm=NR.maps(NC.patch_nmaps(n)))
    return SimpleNamespace(name=name, so=so, kw=kw, vo=orc.canonical_viewport(W, H), normals=kw.get("normals"), tex=kw.get("tex"),
                           nm=kw.get("nm"))


def dress(sp, name):
    """Set on product scene sp (of the row's recipe) what the row's level needs; `plain` clears everything"""
    R = _R()
    if name == "plain":
        sp.clear_textures()
        sp.clear_vertex_normals()
        sp.clear_environment()
        return sp
    if name in ("env", "tex", "nmap", "all"):
        sp.set_sky(8, **SUN)
    if name in ("smooth", "tex", "nmap"):
        sp.smooth_normals(1, NTEAPOT)
    if name == "tex":
        sp.set_textures([TC.images()[3]], None, None)
        sp.project_uvs(1, NTEAPOT, LO, SCALE, 1)
    if name == "nmap":
        sp.set_textures([TC.images()[3], R.normal_map_from_height(NC.heights(), HEIGHT_SCALE)], None, None)
        sp.project_uvs(1, NTEAPOT, LO, SCALE, 1)
        sp.set_normal_maps(np.full(NTEAPOT, 2, np.uint32))
    if name == "all":
        r = row(name)
        sp.set_textures(NC.images(), r.tex.uvs[1:], r.tex.tex_of_tri[1:].astype(np.uint32))
        sp.set_normal_maps(NC.patch_nmaps(len(r.tex.uvs))[1:])
        sp.set_vertex_normals(r.normals[1:])
    return sp


def product(name):
    """A fresh product scene of a row (or of `plain`)"""
    return dress(_recipe(name)(CT.ProductApi(_R())), name)


def viewport(spp=S, vp12=None):
    R = _R()
    return R.canonical_viewport(W, H, DEPTH, spp) if vp12 is None else R.Viewport(W, H, vp12, DEPTH, spp)


# ---------------------------------------------------------------- the restatement's renders
def _side(name):
    """(oracle scene, keywords) of a row, or of `plain`: the canonical scene without a keyword"""
    r = row("env" if name == "plain" else name)
    return r, ({} if name == "plain" else r.kw)


def render(name, spp=S, vp12=None, seed=SEED, **more):
    """nmap_ref.render of a row (or of `plain`)"""
    r, kw = _side(name)
    return NR.render(_orc(), r.so, r.vo if vp12 is None else vp12, W, H, spp, seed, DEPTH, **kw, **more)


def path_trace(name, o4, d4, pixel, sample):
    r, kw = _side(name)
    return NR.path_trace(_orc(), r.so, o4, d4, pixel, sample, DEPTH, SEED, **kw)


def sample_colours(ref, nrows=H):
    """(S, nrows, W, 4) from a render's .color, one row per (pixel, sample), pixel-major"""
    return np.ascontiguousarray(ref.color.reshape(nrows, W, -1, 4).transpose(2, 0, 1, 3))


def _replayed(name, ref, cols, rows, tol):
    counts, accum, sumsq, passes, unconverged = replay(cols, M, P, *tol)
    with np.errstate(all="ignore"):
        out = (accum * (F32(1.0) / counts.astype(F32))[..., None]).astype(F32)
    # the pixel list of refinement pass k (k = 1 ..): the pixels the stop rule left active after M + (k - 1) * P samples
    lists = [np.flatnonzero(counts.ravel() > M + k * P) for k in range(passes - 1)]
    frame_counts = np.zeros((H, W), np.int64)
    frame_counts[rows] = counts
    sel = ref.sample < frame_counts.ravel()[ref.pixel]
    pt = path_trace(name, ref.o4[sel], ref.d4[sel], ref.pixel[sel], ref.sample[sel])
    return SimpleNamespace(ref=ref, cols=cols, tol=tol, counts=counts, accum=accum, sumsq=sumsq, passes=passes, unconverged=unconverged,
                           out=out, lists=lists, samples=int(counts.sum()), rays=pt.rays, subset=sel, subset_color=pt.color, rows=rows)


@functools.lru_cache(maxsize=None)
def expect(name):
    """The adaptive expectations of a row on the full frame (the module's docstring); tests must not modify them"""
    ref = render(name)
    cols = sample_colours(ref)
    return _replayed(name, ref, cols, list(range(H)), pick_tol(cols, M, P))


@functools.lru_cache(maxsize=None)
def expect_tile(name, tile=STRIPED):
    """The same over the rows of a striped tile, at the full frame's tolerance: the replay of those rows' colours"""
    rows = FR.tile_rows(tile)
    ref = render(name, tile=tile)
    return _replayed(name, ref, sample_colours(ref, len(rows)), rows, expect(name).tol)


@functools.lru_cache(maxsize=None)
def pass_refs(name, tile=None):
    """The renders of PASSES in turn, each continued from the accum of the one before"""
    out, accum = [], None
    for k0, n in PASSES:
        ref = render(name, sample0=k0, nsamples=n, tile=tile, accum0=accum)
        accum = ref.accum
        out.append(ref)
    return out


def views():
    """The three views' 12 floats: canonical, glass_cases' side view, tests/test_nmap.py's second camera"""
    orc = _orc()
    c = THIRD_VIEW
    third = orc.create_viewport(W, H, c["size"], np.array(c["pos"], F32), orc.unit(list(c["aim"])), c["fov"], orc.to_radians(c["roll"]))
    return [orc.canonical_viewport(W, H), GC.side_viewport(orc, W, H), third]


@functools.lru_cache(maxsize=None)
def view_refs(name):
    return [render(name, spp=VIEW_SPP, vp12=v, seed=SEED + k) for k, v in enumerate(views())]


def permutation(n):
    return np.random.default_rng(11).permutation(n)


@functools.lru_cache(maxsize=None)
def rays_case(name):
    """The frame's primary rays under permutation(): o4, d4, keys (n, 2) and the restatement's colours in that order; and the same
    rays un-keyed in groups of G: mean, albedo, normal, ids of path_trace / the guides with pixel = group, sample = place in group"""
    r, e = row(name), expect(name)
    ref = e.ref
    n = len(ref.o4)
    perm = permutation(n)
    o4, d4 = np.ascontiguousarray(ref.o4[perm]), np.ascontiguousarray(ref.d4[perm])
    keys = np.stack([ref.pixel[perm], ref.sample[perm]], axis=1).astype(np.uint32)
    grp = path_trace(name, o4, d4, np.arange(n) // G, np.arange(n) % G)
    mean = fold(grp.color, n // G, G)[1]  # walk_ray_set's mean of each group of G consecutive rays
    rays = (o4, d4, n // G, G)
    if r.tex is not None:
        alb, nrm, ids = NR.features(_orc(), r.so, r.normals, r.tex, r.nm, 0, 0, None, G, SEED, rays=rays)
    else:
        nn = np.zeros((len(r.so.triangles()[0]), 3, 3), F32) if r.normals is None else r.normals
        alb, nrm, ids = SR.features(_orc(), r.so, nn, 0, 0, None, G, SEED, rays=rays)
    return SimpleNamespace(perm=perm, o4=o4, d4=d4, keys=keys, color=ref.color[perm], rays=ref.rays, group_color=grp.color, group_rays=grp.rays,
                           mean=mean, albedo=alb, normal=nrm, ids=ids)


@functools.lru_cache(maxsize=None)
def wrapper_inputs(name):
    """What rtmi_render_adaptive_denoised filters: the replay's colour, the guides of the first M samples, rtmi_variance of the moments"""
    r, e = row(name), expect(name)
    alb, nrm, _ = NR.features(_orc(), r.so, r.normals, r.tex, r.nm, W, H, r.vo, S, SEED, nsamples=M)
    return SimpleNamespace(color=e.out, albedo=alb, normal=nrm, var=DV.variance_ref(e.accum, e.sumsq, e.counts))


# ---------------------------------------------------------------- the batch plan, restated
def plan_batches(npix_call, spp, tuning, nrows=None, refinement=False):
    """plan_tile's streams and batches for a call of npix_call pixels with spp samples each under `tuning` (a dict; streams = 0 is
    automatic): a list, one entry per stream, of the (first, count) pixel runs of its batches.  A list pass (nrows None) cuts its
    list into contiguous chunks, one per stream; a tile call deals its nrows rows of W pixels out one at a time."""
    auto = 1 if refinement else 3
    nsub = min(tuning.get("streams", 0) or auto, npix_call if nrows is None else nrows)
    if npix_call * spp < tuning.get("subtile_min_paths", 32768):
        nsub = 1
    if nrows is None:
        base = [npix_call * t // nsub for t in range(nsub + 1)]
        sub = [base[t + 1] - base[t] for t in range(nsub)]
    else:
        sub = [(nrows - t + nsub - 1) // nsub * W for t in range(nsub)]
    want = max(tuning.get("batch_paths", 256 << 20), 1) // nsub
    ppb = max(1, want // spp)
    mx = max(sub)
    if ppb < mx:
        nb = -(-mx // ppb)
        ppb = mx if mx * 8 <= ppb * 9 else -(-mx // nb)
    ppb = min(ppb, mx)
    return [[(p0, min(ppb, n - p0)) for p0 in range(0, n, ppb)] for n in sub]


def runs(pixels):
    """The number of runs of consecutive pixels in an ascending list"""
    pixels = np.asarray(pixels)
    return 0 if len(pixels) == 0 else 1 + int((np.diff(pixels) != 1).sum())
