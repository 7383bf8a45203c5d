"""The four call families that trace shadow rays inside the bounce loop (rtmi_render_lit*, the same with RTMI_LIT_SURFACES,
rtmi_render_envlight*, rtmi_render_emissive*) as one table: each family's scenes, lights or lamps, sizes and reference function are
those of its own test file, so that the rows of tests/test_shadow_matrix.py reuse references those files already justify.  A plain
module (not a conftest), shared by test_shadow_matrix_cpu.py (which asserts from the references alone every condition the rows rely
on) and test_shadow_matrix.py (the product on the GPU).  It holds the families, the rows, the recording hook, the shared sizes and
what a row runs on the product; nothing in here asserts anything about the code under test."""
import ctypes as C
import functools
from types import SimpleNamespace

import numpy as np

import conftest as CT
import emissive_cases as EC
import emissive_ref as EM
from envlight_cases import SUN, hdr as _hdr, rotation as _rotation
import env_ref as ER
import envlight_ref as EL
import lit_ref as LT
import lit_surfaces_cases as LC
import lit_surfaces_ref as LS

F32 = np.float32
SEED = 5
WORK = ("box_tests", "tri_tests", "full_tests", "nodes", "leaves")
# DCtrl::hyb (hybrid.hpp)
OFFERED, REFUSED, MISSES, TIES, F_ABSENT, F_NOCOLLIDE, F_TMIN, F_NOTRI, FALLBACKS, VIOLATIONS, F_BOUNDS, CONFIRMED = range(12)

# the sizes: every family's file renders 32 x 32, spp 4, depth 4 by default; the linear lists are each file's own
DEFAULT = dict(w=32, h=32, spp=4, depth=4)
LIST = dict(lit=dict(w=16, h=16, spp=4, depth=4), lit_surf=dict(w=16, h=16, spp=2, depth=3), envlight=dict(w=16, h=16, spp=4, depth=4),
            emissive=dict(w=16, h=16, spp=4, depth=4))
DEEP = dict(w=16, h=16, spp=1, depth=32)  # RTMI_MAX_PASSES levels: the shadow queue index pass + 1 reaches 31


# ---------------------------------------------------------------- the depth-32 scene
DEEP_LAMPS = (9, 10)


def recipe_matte_corridor(lamp=False):
    """shadowed_ref.recipe_corridor with Matte walls: two large walls facing each other (z = +-6, tilted by a few 1e-4), the canonical
    camera between them, so that every level's hit is Matte and gets its candidates (the corridor of test_shadowed.py is Reflective,
    and these calls sample at Matte hits only).  The reference starts a Lambertian bounce at point + random_vec * 0.001, behind the
    surface for half the draws; such a ray meets its own wall from behind, bounces off its back and leaves the scene, which alone
    ends a quarter of the paths per level.  So each wall (triangles 1 .. 4) is backed by a Reflective wall without scattering 0.02
    behind it (triangles 5 .. 8): a reflected ray always starts on the side it came from, and a path that slips behind a Matte wall
    bounces between the two until it slips back.  Every path is then alive at level 31.
    lamp: tests/emissive_cases.py's wall lamp (a small Solid quad at z ~ 2.5) as triangles 9, 10."""
    def r(api):
        s = api.scene()
        for surf, behind in ((api.matte((220, 200, 180), 0.3), 0.0), (api.reflective(0.0, (230, 230, 230), 0.7), 0.02)):
            for zc, flip in ((6.0 + behind, 1.0), (-6.0 - behind, -1.0)):
                z = lambda x, y: zc + flip * (0.0001 * x + 0.0002 * y)
                a, b, c, d = ([-98.0, -101.0], [104.0, -101.0], [104.0, 101.0], [-98.0, 101.0])
                p = lambda q: [q[0], q[1], z(*q)]
                api.add_triangle(s, np.array([p(a), p(b), p(c)], F32), surf, 0.0)
                api.add_triangle(s, np.array([p(a), p(c), p(d)], F32), surf, 0.0)
        if lamp:
            zl = lambda x, y: 2.5 + 0.02 * x - 0.01 * y
            q = [[x, y, zl(x, y)] for x, y in ((3.5, 0.5), (5.0, 0.5), (5.0, 2.0), (3.5, 2.0))]
            surf = EC.solid_f32(api, EC.LAMP_COLOR)
            api.add_triangle(s, np.array([q[0], q[1], q[2]], F32), surf, 0.0)
            api.add_triangle(s, np.array([q[0], q[2], q[3]], F32), surf, 0.0)
        s.populate_triangle_numbers()
        s.build_bounding_box([2.0, 0.0, 0.0], 128.0, 2, 1)
        return s
    return r


def corridor_normals(rec):
    """Hand-set corner normals for the corridor's four wall triangles: the geometric normal tilted by 0.2 towards a direction of
    the corner's own, (ntris, 3, 3) float32 with the sentinel's row zero"""
    rec = np.asarray(rec, F32)
    out = np.zeros((len(rec), 3, 3), F32)
    for i in range(1, 5):
        ng = rec[i, 3:6].astype(np.float64)
        for k, t in enumerate(((0.2, 0.0, 0.0), (-0.1, 0.15, 0.0), (0.0, -0.2, 0.0))):
            v = ng + np.array(t)
            out[i, k] = (v / np.linalg.norm(v)).astype(F32)
    return out


# ---------------------------------------------------------------- the recording hook
class Recorder:
    """trace= of every reference: forwards to the oracle's closest hits and sums the oracle's work counters and the rays over every
    batch it is handed -- the expected work of the call, independent of the code under test"""

    def __init__(self, so):
        self.so = so
        self.rays = 0
        self.batches = 0
        self.counters = {k: 0 for k in WORK}
        self.oracle_rays = 0

    def __call__(self, o4, d4):
        tri, t, face, cn = self.so.trace(o4, d4)
        self.rays += int(np.asarray(o4).reshape(-1, 4).shape[0])
        self.oracle_rays += cn["rays"]
        self.batches += 1
        for k in WORK:
            self.counters[k] += cn[k]
        return tri, t, face


def _orc():
    from oracle import orc
    return orc


def _R():
    from rust_raytrace_amd import raytrace as R
    return R


# ---------------------------------------------------------------- the families
class Family:
    """One call family: scenes of kind "octree" (the default size), "list" (its linear list) and "deep" (the depth-32 corridor)"""
    name = None
    per_path = 1  # shadow rays a path can queue per level, at most

    def size(self, kind):
        return {"octree": DEFAULT, "list": LIST[self.name], "deep": DEEP}[kind]

    @functools.lru_cache(maxsize=None)
    def oracle(self, kind):
        """(oracle scene, what the reference takes beside it)"""
        so = self.recipe(kind)(CT.OracleApi(_orc()))
        return so, self.inputs(so, kind)

    def product(self, kind):
        sp = self.recipe(kind)(CT.ProductApi(_R()))
        self.feature(sp, kind)
        return sp

    def feature(self, sp, kind):
        pass

    def inputs(self, so, kind):
        return None

    def render(self, kind, size=None, trace=None, plain=False):
        """The family's reference for one frame; plain: the same paths without their shadow rays"""
        so, x = self.oracle(kind)
        k = size or self.size(kind)
        orc = _orc()
        return self._render(orc, so, x, orc.canonical_viewport(k["w"], k["h"]), k, trace, plain)

    def call(self, c, sp, kind, size=None, plain=False):
        """(image, accum, stats) of the family's host call on product scene sp"""
        k = size or self.size(kind)
        vp = _R().canonical_viewport(k["w"], k["h"], k["depth"], k["spp"])
        img, ctx = self._call(c, vp, sp, plain)
        return img, ctx.accum, ctx.stats


class Lit(Family):
    name = "lit"
    per_path = 2
    lights = (LT.A, LT.B)

    def recipe(self, kind):
        return {"octree": CT.recipe_canonical(), "list": CT.recipe_canonical(accel="trivial", obj=CT.TEAPOT), "deep": recipe_matte_corridor()}[kind]

    def _render(self, orc, so, x, vo, k, trace, plain):
        return LT.render(orc, so, vo, k["w"], k["h"], k["spp"], SEED, k["depth"], () if plain else self.lights, trace=trace)

    def _call(self, c, vp, sp, plain):
        return c.walk_rays_lit(vp, sp, c.lit_params(() if plain else self.lights))

    def _paths(self, orc, so, x, r, sel, depth):
        return LT.path_trace(so, r.o4[sel], r.d4[sel], r.pixel[sel], r.sample[sel], depth, SEED, self.lights)

    def levels(self, ref):
        pt = getattr(ref, "pt", ref)
        return [sum(x) for x in pt.live], [sum(x) for x in pt.occluded]


class LitSurf(Family):
    name = "lit_surf"
    per_path = 2
    lights = LC.AB

    def recipe(self, kind):
        return Lit.recipe(self, kind)

    def inputs(self, so, kind):
        rec = so.triangles()[0]
        if kind == "octree":
            return LC.teapot_inputs(so)
        if kind == "deep":
            return SimpleNamespace(normals=corridor_normals(rec), tex=None, nm=None)
        # tests/test_lit_surfaces.py's linear list: this teapot file has its own triangle count, every triangle gets the treatment
        import nmap_cases as NC
        import nmap_ref as NR
        import smooth_ref as SR
        import tex_cases as TC
        import tex_ref as TR
        n = len(rec) - 1
        uvs, tot, nm = np.zeros((n + 1, 3, 2), F32), np.zeros(n + 1, np.uint32), np.zeros(n + 1, np.uint32)
        uvs[1:] = TR.project(rec[1:, 20:29], rec[1:, 3:6], LC.LO, LC.SCALE)
        tot[1:], nm[1:] = 1, 2
        nrm = np.zeros((n + 1, 3, 3), F32)
        nrm[1:] = SR.generate(rec[1:, 20:29], rec[1:, 3:6], LC.CREASE)
        return SimpleNamespace(normals=nrm, tex=TR.textures([TC.images()[3], NR.from_height(NC.heights(), LC.HEIGHT_SCALE)], uvs, tot), nm=NR.maps(nm))

    def feature(self, sp, kind):
        R = _R()
        if kind == "octree":
            LC.feature_teapot(R, sp)
        elif kind == "deep":
            sp.set_vertex_normals(corridor_normals(sp.triangles()[0])[1:])
        else:
            import nmap_cases as NC
            import tex_cases as TC
            n = len(sp.triangles()[0]) - 1
            sp.smooth_normals(1, n, LC.CREASE)
            sp.set_textures([TC.images()[3], R.normal_map_from_height(NC.heights(), LC.HEIGHT_SCALE)], None, None)
            sp.project_uvs(1, n, LC.LO, LC.SCALE, 1)
            sp.set_normal_maps(np.full(n, 2, np.uint32))

    def _render(self, orc, so, f, vo, k, trace, plain):
        return LS.render(orc, so, vo, k["w"], k["h"], k["spp"], SEED, k["depth"], () if plain else self.lights, False, None, f.normals, f.tex,
                         f.nm, trace=trace)

    def _call(self, c, vp, sp, plain):
        return c.walk_rays_lit(vp, sp, c.lit_params(() if plain else self.lights, surfaces=True))

    def _paths(self, orc, so, f, r, sel, depth):
        return LS.path_trace(orc, so, r.o4[sel], r.d4[sel], r.pixel[sel], r.sample[sel], depth, SEED, self.lights, False, None, f.normals,
                             f.tex, f.nm)

    def levels(self, ref):
        pt = getattr(ref, "pt", ref)
        return [sum(x) for x in pt.live], [sum(x) for x in pt.occluded]


class Envlight(Family):
    name = "envlight"

    def recipe(self, kind):
        return Lit.recipe(self, kind)

    def inputs(self, so, kind):
        if kind == "list":
            return SimpleNamespace(table=_hdr(5), frame=_rotation())
        return SimpleNamespace(table=ER.sky_table(16, SUN), frame=None)

    def feature(self, sp, kind):
        if kind == "list":
            sp.set_environment(_hdr(5), _rotation())
        else:
            sp.set_sky(16, **SUN)

    def _render(self, orc, so, env, vo, k, trace, plain):
        return EL.render(orc, so, vo, k["w"], k["h"], k["spp"], SEED, k["depth"], env, nee=not plain, trace=trace)

    def _call(self, c, vp, sp, plain):
        assert not plain
        return c.walk_rays_envlight(vp, sp)

    def _paths(self, orc, so, env, r, sel, depth):
        return EL.path_trace(so, r.o4[sel], r.d4[sel], r.pixel[sel], r.sample[sel], depth, SEED, env)

    def levels(self, ref):
        pt = getattr(ref, "pt", ref)
        return list(pt.nlive), list(pt.occluded)


class Emissive(Family):
    name = "emissive"

    def recipe(self, kind):
        return {"octree": EC.recipe_teapot_lamp(), "list": EC.recipe_teapot_lamp("trivial"), "deep": recipe_matte_corridor(lamp=True)}[kind]

    def inputs(self, so, kind):
        return DEEP_LAMPS if kind == "deep" else EC.TEAPOT_LAMPS

    def feature(self, sp, kind):
        sp.set_emitters(np.array(self.inputs(None, kind)))

    def _render(self, orc, so, lamps, vo, k, trace, plain):
        return EM.render(orc, so, vo, k["w"], k["h"], k["spp"], SEED, k["depth"], lamps, nee=not plain, trace=trace)

    def _call(self, c, vp, sp, plain):
        assert not plain
        return c.walk_rays_emissive(vp, sp)

    def _paths(self, orc, so, lamps, r, sel, depth):
        return EM.path_trace(so, r.o4[sel], r.d4[sel], r.pixel[sel], r.sample[sel], depth, SEED, lamps)

    def levels(self, ref):
        pt = getattr(ref, "pt", ref)
        return list(pt.nlive), list(pt.lost)  # (a shadow ray that does not reach its lamp is lost)


FAMILIES = {f.name: f for f in (Lit(), LitSurf(), Envlight(), Emissive())}


@functools.lru_cache(maxsize=None)
def expected(fam, kind):
    """The reference of family `fam` on its scene of `kind` at the kind's size, through the recording hook: (ref, Recorder).
    Computed once; tests must not modify it.  (test_shadow_matrix_cpu.py shows that the hook changes no bit.)"""
    f = FAMILIES[fam]
    rec = Recorder(f.oracle(kind)[0])
    return f.render(kind, trace=rec), rec


# ---------------------------------------------------------------- the batch split of a frame call (plan_tile, rtmi_device.hip)
SMALL = dict(streams=4, batch_paths=40, subtile_min_paths=1)


def batch_paths_of(tuning, k):
    """The paths one batch holds under `tuning` for a whole frame of size k: the rows are dealt out to the streams, a stream's
    share of batch_paths is cut into whole pixels, and equal batches cover the largest sub-tile"""
    npix_call, spp = k["w"] * k["h"], k["spp"]
    nsub = min(tuning["streams"], k["h"])
    if npix_call * spp < tuning["subtile_min_paths"]:
        nsub = 1
    max_sub = -(-k["h"] // nsub) * k["w"]
    per = max(1, (max(tuning["batch_paths"], 1) // nsub) // spp)
    if per < max_sub:
        nb = -(-max_sub // per)
        per = max_sub if max_sub * 8 <= per * 9 else -(-max_sub // nb)
    return min(per, max_sub) * spp


def batch_pixels(tuning, k, t, b):
    """The frame pixels (row * w + column) of batch b of stream t under `tuning`: the stream's rows are t, t + nsub, ..., its
    pixels run row by row, and a batch is the next batch_paths_of / spp of them"""
    nsub = min(tuning["streams"], k["h"])
    per = batch_paths_of(tuning, k) // k["spp"]
    sub = [r * k["w"] + c for r in range(t, k["h"], nsub) for c in range(k["w"])]
    return sub[b * per:(b + 1) * per]


def batch_levels(fam, kind, tuning, t, b):
    """The live shadow rays per level of that one batch: the family's path trace on the batch's own primary rays (a path's rays
    depend on its pixel and sample alone, so the subset's paths are the frame's)"""
    f = FAMILIES[fam]
    ref, _ = expected(fam, kind)
    so, x = f.oracle(kind)
    k = f.size(kind)
    sel = np.isin(ref.pixel, batch_pixels(tuning, k, t, b))
    return f.levels(f._paths(_orc(), so, x, ref, sel, k["depth"]))[0], int(sel.sum())


# ---------------------------------------------------------------- the rows
ALL = tuple(FAMILIES)
# the tuning rows run on lit (the nlights-wide queue through launch_occluded) and emissive (launch_trace alone); lit_surf and envlight
# take the same two branches, and with their twelve rows the two files ran longer than the four families' own files
TUNED = ("lit", "emissive")
# name: kind of scene, options (names of R.OPT_*), tuning, creation-time environment (a fresh child process), the families
ROWS = {
    "default_counters": dict(opts=("COUNTERS",)),
    "default_route": dict(),
    "generic": dict(opts=("GENERIC",)),
    "generic_counters": dict(opts=("GENERIC", "COUNTERS")),
    "hybrid_off_counters": dict(opts=("COUNTERS",), env={"RTMI_HYBRID": "0"}),
    "anyhit": dict(env={"RTMI_LIT_FROM_HITS": "0"}, fams=("lit", "lit_surf")),
    "linear_from_hits": dict(kind="list", opts=("COUNTERS",), env={"RTMI_OCCLUDED_ANYHIT": "0"}, fams=("lit", "lit_surf", "envlight")),
    "tune_xcd1": dict(tuning={"xcd_aware": 1}, fams=TUNED),
    "tune_xcd2_one_stream": dict(tuning={"xcd_aware": 2, "streams": 1}, fams=TUNED),
    "tune_one_wave_per_cu": dict(tuning={"oct_waves_per_cu": 1}, fams=TUNED),
    "tune_refill_1": dict(tuning={"refill_min0": 1, "refill_min": 1}, fams=TUNED),
    "tune_refill_64": dict(tuning={"refill_min0": 64, "refill_min": 64}, fams=TUNED),
    "tune_small_batches": dict(tuning=SMALL, fams=TUNED),
    "depth32": dict(kind="deep"),
    "fast": dict(opts=("FAST",), own=True),
    "bvh": dict(opts=("BVH",), own=True, fams=("lit", "lit_surf", "envlight")),
}
CASES = [(f, r) for r, row in ROWS.items() for f in row.get("fams", ALL)]


def options_of(row, extra=()):
    R = _R()
    o = 0
    for name in tuple(row.get("opts", ())) + tuple(extra):
        o |= getattr(R, "OPT_" + name)
    return o


# ---------------------------------------------------------------- what a row runs on the product
def hybrid_readout(sp):
    """(DCtrl::hyb of the main workspaces, whether the scene qualifies for hybrid passes, DCtrl::hyb of the shadow workspaces) of
    the resident scene's last call, each summed over the streams (their last batches)"""
    from rust_raytrace_amd import _ffi
    L = _ffi.lib()
    L.rth_debug_hybrid_counters.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.rth_debug_shadow_hybrid_counters.argtypes = [C.c_void_p, C.c_void_p]
    d, on, sh = (C.c_ulonglong * 12)(), C.c_int(0), (C.c_ulonglong * 12)()
    assert L.rth_debug_hybrid_counters(sp.h, d, C.byref(on)) == 0
    assert L.rth_debug_shadow_hybrid_counters(sp.h, sh) == 0
    return [int(x) for x in d], int(on.value), [int(x) for x in sh]


def ints(stats):
    return {k: int(v) for k, v in stats.items() if isinstance(v, (int, np.integer))}


def run_call(f, c, sp, kind, plain=False):
    """One call and its readout: (arrays, info)"""
    img, acc, st = f.call(c, sp, kind, plain=plain)
    main, on, shadow = hybrid_readout(sp)
    return dict(image=img, accum=acc), dict(stats=ints(st), main=main, on=on, shadow=shadow)


def run_row(fam, name, sp=None):
    """Row `name` of family `fam` on the product: ({key: array}, {key: info}) with key "call" and, for the any-hit row, "counting"
    (the same call under RTMI_OPT_COUNTERS) and "plain" (the call without its lights, counting: the plain per-pass pipeline).  sp:
    a product scene of the row's kind to reuse (the caller restores its tuning)."""
    R = _R()
    f, row = FAMILIES[fam], ROWS[name]
    kind = row.get("kind", "octree")
    sp = sp or f.product(kind)
    arrays, info = {}, {}
    a, info["call"] = run_call(f, R.HipRayCaster(seed=SEED, options=options_of(row), tuning=row.get("tuning")), sp, kind)
    arrays.update({"call_" + k: v for k, v in a.items()})
    if name == "anyhit":
        cc = R.HipRayCaster(seed=SEED, options=options_of(row, ("COUNTERS",)))
        a, info["counting"] = run_call(f, cc, sp, kind)
        arrays.update({"counting_" + k: v for k, v in a.items()})
        _, info["plain"] = run_call(f, cc, sp, kind, plain=True)
    return arrays, info
