"""Scenes, views and lamps of the tests of box lights on shaded surfaces (tests/test_lit_surfaces_cpu.py, tests/test_lit_surfaces.py):
the exact recipes the GPU file renders, so that the CPU file can check their case mix on the restatement alone.

The patch is tests/nmap_cases.py's with smooth_cases' hand-set normals, its textures and its tame maps, seen through PATCH_VIEW: the
canonical view shows mostly floor, and fewer than a quarter of its level-0 candidates have a shading normal of their own; from
(0, 2, 1) 36 % have.  The teapot is the canonical scene with generated vertex normals (crease 0.5), tests/test_nmap.py's box
projection, 8 x 8 texture and height-field map.  The slab is glass_cases.recipe_slab with a lamp on the camera's side of the glass,
so that what reaches the Matte strip and the floor behind the slab has to cross it; it is built as a linear list, because in the
reference's octree a ray can miss the slab's large faces, which reach outside the root box, and "every crossing candidate is
occluded" is then not a property of the closest hits the definition stands on."""
from types import SimpleNamespace

import numpy as np

import glass_cases as GC
import lit_ref as LT
import nmap_cases as NC
import nmap_ref as NR
import smooth_cases as SC
import smooth_ref as SR
import tex_cases as TC
import tex_ref as TR

F32 = np.float32
SEED = 5
NTEAPOT = 6320                      # triangles 1 .. 6320 of the canonical scene are the teapot's
LO, SCALE = (-1.7, -0.4, 3.1), 0.9  # tests/test_tex.py's box projection of the teapot
HEIGHT_SCALE = 2.0
CREASE = 0.5
TEAPOT = dict(w=32, h=32, spp=4, depth=4)
PATCH = dict(w=16, h=16, spp=2, depths=(1, 2, 3))
PATCH_VIEW = dict(pos=(0.0, 2.0, 1.0), aim=(0.0, 0.0, 1.0), fov=90.0)
AB = (LT.A, LT.B)
# lit_ref.FOUR with bake_lit_ref's third light: the unbounded one
FOUR = (LT.A, LT.B, LT.light((3.0, 2.0, 7.0), 0.25, (0.5, 0.0, 0.25), unbounded=True), LT.FOUR[3])
SLAB_LAMP = LT.light((-3.0, 0.5, 2.0), 0.25, (1.0, 0.9, 0.8))
SLAB = dict(w=16, h=16, spp=2, depth=3)


def patch_view(orc):
    """The 12 floats of PATCH_VIEW at the patch's frame size"""
    c = PATCH_VIEW
    return orc.create_viewport(PATCH["w"], PATCH["h"], (1.0, 1.0), np.array(c["pos"], F32), orc.unit(list(c["aim"])), c["fov"], orc.to_radians(0.0))


def patch_inputs(so):
    """What the restatement takes for the featured patch on oracle scene `so`: normals, uvs, tot, nmaps, tex, nm"""
    rec = so.triangles()[0]
    n = len(rec)
    uvs, tot = NC.patch_uvs(n)
    nmaps = NC.patch_nmaps(n)
    nrm = np.zeros((n, 3, 3), F32)
    nrm[:SC.NTRI_PATCH + 1] = SC.patch_normals(rec)[:SC.NTRI_PATCH + 1]
    return SimpleNamespace(normals=nrm, uvs=uvs, tot=tot, nmaps=nmaps, tex=TR.textures(NC.images(), uvs, tot), nm=NR.maps(nmaps))


def feature_patch(sp, p, normals=True, textures=True, maps=True):
    """The same on product scene `sp`; a feature switched off is left out (maps need the uvs: textures are then set with no
    triangle textured)"""
    if normals:
        sp.set_vertex_normals(p.normals[1:])
    if textures or maps:
        sp.set_textures(NC.images(), p.uvs[1:], p.tot[1:] if textures else np.zeros_like(p.tot[1:]))
    if maps:
        sp.set_normal_maps(p.nmaps[1:])


def teapot_inputs(so):
    """What the restatement takes for the featured teapot on oracle scene `so`: normals, tex, nm"""
    rec = so.triangles()[0]
    uvs, tot, nm = np.zeros((len(rec), 3, 2), F32), np.zeros(len(rec), np.uint32), np.zeros(len(rec), np.uint32)
    t = slice(1, 1 + NTEAPOT)
    uvs[t] = TR.project(rec[t, 20:29], rec[t, 3:6], LO, SCALE)
    tot[t] = 1
    nm[t] = 2
    nrm = np.zeros((len(rec), 3, 3), F32)
    nrm[t] = SR.generate(rec[t, 20:29], rec[t, 3:6], CREASE)
    return SimpleNamespace(normals=nrm, tex=TR.textures([TC.images()[3], NR.from_height(NC.heights(), HEIGHT_SCALE)], uvs, tot), nm=NR.maps(nm))


def feature_teapot(R, sp):
    """The same on product scene `sp`: smooth_normals and tests/test_nmap.py's _map_the_teapot"""
    sp.smooth_normals(1, NTEAPOT, CREASE)
    sp.set_textures([TC.images()[3], R.normal_map_from_height(NC.heights(), HEIGHT_SCALE)], None, None)
    sp.project_uvs(1, NTEAPOT, LO, SCALE, 1)
    sp.set_normal_maps(np.full(NTEAPOT, 2, np.uint32))


def crosses_slab(point, lamp, shrink=0.0):
    """float64: whether the segment from each point (m, 3) to `lamp` (m, 3) crosses the slab's box, shrunk by `shrink` on every side"""
    lo, hi = np.array(GC.SLAB["lo"], np.float64) + shrink, np.array(GC.SLAB["hi"], np.float64) - shrink
    p, d = np.asarray(point, np.float64), np.asarray(lamp, np.float64) - np.asarray(point, np.float64)
    with np.errstate(all="ignore"):
        t0, t1 = (lo - p) / d, (hi - p) / d
    tn, tf = np.minimum(t0, t1).max(axis=1), np.maximum(t0, t1).min(axis=1)
    return (tn <= tf) & (tf >= 0.0) & (tn <= 1.0)
