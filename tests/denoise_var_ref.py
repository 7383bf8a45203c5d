"""NumPy float32 restatement of the variance image and the variance-guided a-trous filter (rtmi_variance*, rtmi_denoise_var*;
include/rtmi.h states them operation by operation).  Vectorised over pixels, sequential over taps, as tests/denoise_ref.py is,
whose g, len2 and K it reuses: every pixel's additions happen in the stated order (dy outer, dx inner) and a tap of weight 0 is
not added.  Depends on nothing but NumPy and denoise_ref.  A plain helper module of tests/test_denoise_var_cpu.py and
tests/test_denoise_var.py."""
import numpy as np

from denoise_ref import DEMODULATE, EPS, F32, INF, K, g, len2

DEFAULTS = dict(iterations=1, flags=0, sigma_color=3.0, sigma_normal=0.5, sigma_depth=0.1, sigma_albedo=np.inf)
K3 = np.array([0.25, 0.5, 0.25], F32)
TINY = F32(2.0 ** -40)


def lane_sum(v):
    """((0 + v_r) + v_g) + v_b of the last axis"""
    s = np.zeros(v.shape[:-1], F32)
    for c in range(3):
        s = s + v[..., c]
    return s


def variance_ref(accum, sumsq, counts):
    """Expected output of rtmi_variance: (..., 4) float32 sums and sums of squares, (...) uint32 counts -> (..., 4) float32, the
    variance of the mean per channel and their ordered sum; all four lanes +inf where count < 2."""
    s, q = np.asarray(accum, F32), np.asarray(sumsq, F32)
    cnt = np.asarray(counts, np.uint32)
    assert s.shape == q.shape and s.shape[-1] == 4 and cnt.shape == s.shape[:-1]
    with np.errstate(all="ignore"):
        n = cnt.astype(F32)[..., None]
        n1 = (cnt - np.uint32(1)).astype(F32)[..., None]  # count 0 wraps like the device's n - 1u; those pixels are overwritten
        inv = F32(1.0) / n
        m = s[..., 0:3] * inv
        v = (q[..., 0:3] - s[..., 0:3] * m) / n1
        vm = v / n
        vm = np.where(vm < 0, F32(0.0), vm).astype(F32)
        out = np.zeros(s.shape, F32)
        out[..., 0:3] = vm
        out[..., 3] = lane_sum(vm)
    out[cnt < 2] = INF
    return out


def prefilter3(vs):
    """gv: the 3 x 3 prefilter of lane 3 of the variance, (H, W) -> (H, W); taps outside the image are skipped"""
    H, W = vs.shape
    num = np.zeros((H, W), F32)
    den = np.zeros((H, W), F32)
    for dy in range(-1, 2):
        for dx in range(-1, 2):
            kk = F32(K3[dy + 1] * K3[dx + 1])
            y0, y1 = max(0, -dy), min(H, H - dy)
            x0, x1 = max(0, -dx), min(W, W - dx)
            if y0 >= y1 or x0 >= x1:
                continue
            P = (slice(y0, y1), slice(x0, x1))
            Q = (slice(y0 + dy, y1 + dy), slice(x0 + dx, x1 + dx))
            num[P] = num[P] + kk * vs[Q]
            den[P] = den[P] + kk
    return (num / den).astype(F32)


def atrous_var_iteration(u, var, a, cov, n, d, step, s2n, sd, s2a, sc2):
    """One iteration at tap spacing `step`: u (H, W, 3), var (H, W, 4) -> u' (H, W, 3), var' (H, W, 4)."""
    H, W = u.shape[:2]
    num = np.zeros((H, W, 3), F32)
    nv = np.zeros((H, W, 3), F32)
    den = np.zeros((H, W), F32)
    sdp = sd * d
    s2d = sdp * sdp
    s2c = sc2 * prefilter3(var[..., 3]) + TINY
    vm = var[..., 0:3]
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            kk = F32(K[dy + 2] * K[dx + 2])
            oy, ox = dy * step, dx * step
            y0, y1 = max(0, -oy), min(H, H - oy)
            x0, x1 = max(0, -ox), min(W, W - ox)
            if y0 >= y1 or x0 >= x1:
                continue
            P = (slice(y0, y1), slice(x0, x1))
            Q = (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))
            uq = u[Q]
            if dx == 0 and dy == 0:
                w = np.full(den[P].shape, kk, F32)
            else:
                gc = g(len2(u[P] - uq), s2c[P])
                w = kk * g(len2(n[P] - n[Q]), s2n)
                dd = d[P] - d[Q]
                w = w * g(dd * dd, s2d[P])
                dc = cov[P] - cov[Q]
                w = w * g(dc * dc, F32(0.25))
                w = w * g(len2(a[P] - a[Q]), s2a)
                w = w * gc
                sky = (cov[P] == 0) & (cov[Q] == 0)
                w = np.where(sky, kk * gc, w).astype(F32)
            add = w > 0
            num[P] = np.where(add[..., None], num[P] + w[..., None] * uq, num[P])
            nv[P] = np.where(add[..., None], nv[P] + (w * w)[..., None] * vm[Q], nv[P])
            den[P] = np.where(add, den[P] + w, den[P])
    vout = np.zeros((H, W, 4), F32)
    vout[..., 0:3] = nv / (den * den)[..., None]
    vout[..., 3] = lane_sum(vout[..., 0:3])
    return (num / den[..., None]).astype(F32), vout


def denoise_var_ref(color, albedo, normal, variance, iterations=1, flags=0, sigma_color=3.0, sigma_normal=0.5, sigma_depth=0.1,
                    sigma_albedo=np.inf):
    """Expected (out, var_out) of rtmi_denoise_var for (H, W, 4) float32 images: out has lane 3 = 0, var_out lane 3 = the
    ordered sum of its three channels."""
    color, albedo, normal, variance = (np.ascontiguousarray(x, F32) for x in (color, albedo, normal, variance))
    assert color.ndim == 3 and color.shape[2] == 4 and color.shape == albedo.shape == normal.shape == variance.shape
    sc, sn, sd, sa = F32(sigma_color), F32(sigma_normal), F32(sigma_depth), F32(sigma_albedo)
    a, cov = albedo[..., 0:3], albedo[..., 3]
    n, d = normal[..., 0:3], normal[..., 3]
    with np.errstate(all="ignore"):
        mod = a + EPS
        u = color[..., 0:3].copy()
        var = variance.copy()
        if flags & DEMODULATE:
            u = u / mod
            var[..., 0:3] = (var[..., 0:3] / mod) / mod
            var[..., 3] = lane_sum(var[..., 0:3])
        for i in range(int(iterations)):
            u, var = atrous_var_iteration(u, var, a, cov, n, d, 1 << i, sn * sn, sd, sa * sa, sc * sc)
        if flags & DEMODULATE:
            u = u * mod
            var[..., 0:3] = (var[..., 0:3] * mod) * mod
            var[..., 3] = lane_sum(var[..., 0:3])
    out = np.zeros(color.shape, F32)
    out[..., 0:3] = u
    return out, var.astype(F32)
