"""NumPy restatement of the first-hit feature buffers (rtmi_render_features*, include/rtmi.h) from the oracle as it is:
orc.primary_rays makes the renderer's primary rays ([pixel][sample]), Scene.trace their closest hits, Scene.triangles the
normals and colours.  Everything after that is float32 NumPy in the order the header states: per lane acc = 0; acc = acc + x
per sample in sample order; acc * (1 / n).  A plain helper module of tests/test_features_cpu.py and tests/test_features.py."""
import numpy as np

F32 = np.float32
SKY = np.array([128.0, 180.0, 255.0], F32) / F32(255.0)  # raytrace.rs:1264


def tile_rows(tile):
    """Image rows of an rtmi_tile_t (row0, nrows, stripe_rows, stripe_step), in the order of the tile's rows."""
    row0, nrows, sr, step = (int(x) for x in tile)
    return [row0 + (L // sr) * step + L % sr for L in range(nrows)]


def tile_rays(orc, w, h, vp12, spp, seed, sample0=0, nsamples=None, rows=None):
    """The primary rays of samples [sample0, sample0 + nsamples) of a frame of `spp` samples, for every pixel of image rows
    `rows` (default: all), in [pixel][sample] order: (o4, d4, number of pixels, nsamples)."""
    n = spp - sample0 if nsamples is None else nsamples
    rows = list(range(h)) if rows is None else list(rows)
    o4, d4 = orc.primary_rays(w, h, np.asarray(vp12, F32), spp, seed)
    sel = lambda a: np.ascontiguousarray(a.reshape(h, w, spp, 4)[rows][:, :, sample0:sample0 + n].reshape(-1, 4))
    return sel(o4), sel(d4), len(rows) * w, n


def features_from_hits(tri, t, face, rec, surf, npix, n):
    """(albedo (npix, 4), normal (npix, 4), ids (npix,)) from the closest hits of npix * n rays in [pixel][sample] order;
    rec / surf as Scene.triangles() returns them (rec[:, 3:6] = norm, surf[:, 0:3] = colour)."""
    tri = np.asarray(tri, np.uint32).reshape(npix, n)
    face = np.asarray(face, np.uint32).reshape(npix, n)
    t = np.asarray(t, F32).reshape(npix, n)
    miss = tri == 0
    edge = (face & 2) != 0
    back = (face & 1) != 0
    a = np.zeros((npix, n, 4), F32)
    a[..., 0:3] = np.where(miss[..., None], SKY, np.where(edge[..., None], F32(0.0), surf[tri, 0:3].astype(F32)))
    a[..., 3] = np.where(miss, F32(0.0), F32(1.0))
    norm = rec[tri, 3:6].astype(F32)
    norm = np.where(back[..., None], norm * F32(-1.0), norm)
    nd = np.zeros((npix, n, 4), F32)
    nd[..., 0:3] = np.where(miss[..., None], F32(0.0), norm)
    nd[..., 3] = np.where(miss, F32(0.0), t)
    inv = F32(1.0) / F32(n)
    out = []
    with np.errstate(invalid="ignore", over="ignore"):
        for x in (a, nd):
            acc = np.zeros((npix, 4), F32)
            for s in range(n):
                acc = acc + x[:, s]
            out.append((acc * inv).astype(F32))
    ids = (tri[:, 0] | (face[:, 0] << np.uint32(30))).astype(np.uint32)
    ids[miss[:, 0]] = 0
    return out[0], out[1], ids


def features_ref(orc, so, w, h, vp12, spp, seed, sample0=0, nsamples=None, tile=None):
    """Expected buffers of a features call on oracle scene `so`: albedo (rows, w, 4), normal (rows, w, 4), ids (rows, w), and
    the oracle's work counters for exactly those rays."""
    rows = None if tile is None else tile_rows(tile)
    o4, d4, npix, n = tile_rays(orc, w, h, vp12, spp, seed, sample0, nsamples, rows)
    tri, t, face, cn = so.trace(o4, d4)
    rec, _, surf = so.triangles()
    alb, nrm, ids = features_from_hits(tri, t, face, rec, surf, npix, n)
    nr = npix // w
    return alb.reshape(nr, w, 4), nrm.reshape(nr, w, 4), ids.reshape(nr, w), cn
