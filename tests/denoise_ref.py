"""NumPy float32 restatement of the a-trous denoiser (rtmi_denoise*, include/rtmi.h states it operation by operation).
Vectorised over pixels, sequential over taps: every pixel's additions happen in the stated order (dy outer, dx inner), and a
tap of weight 0 is not added (np.where(w > 0, num + w * u_q, num)).  Depends on nothing but NumPy.  A plain helper module of
tests/test_denoise_cpu.py and tests/test_denoise.py."""
import numpy as np

F32 = np.float32
INF = F32(np.inf)
DEMODULATE = 1
DEFAULTS = dict(iterations=3, flags=0, sigma_color=1.0, sigma_normal=0.5, sigma_depth=0.1, sigma_albedo=np.inf)
K = np.array([1.0 / 16.0, 1.0 / 4.0, 3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0], F32)
EPS = F32(1.0 / 256.0)


def g(x2, s2):
    """Tukey's biweight (x2 < s2) ? (1 - x2/s2)^2 : 0; NaN -> 0."""
    x2, s2 = np.broadcast_arrays(np.asarray(x2, F32), np.asarray(s2, F32))
    ok = x2 < s2
    t = F32(1.0) - np.divide(x2, s2, out=np.zeros(x2.shape, F32), where=ok)
    return np.where(ok, t * t, F32(0.0)).astype(F32)


def len2(v):
    """((0 + x*x) + y*y) + z*z of the last axis"""
    s = np.zeros(v.shape[:-1], F32)
    for c in range(3):
        s = s + v[..., c] * v[..., c]
    return s


def atrous_iteration(u, a, cov, n, d, step, s2n, sd, s2a, s2c):
    """One iteration at tap spacing `step`: u (H, W, 3) -> u' (H, W, 3)."""
    H, W = u.shape[:2]
    num = np.zeros((H, W, 3), F32)
    den = np.zeros((H, W), F32)
    sdp = sd * d
    s2d = sdp * sdp
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            kk = F32(K[dy + 2] * K[dx + 2])
            oy, ox = dy * step, dx * step
            # pixels p = (y, x) whose tap q = (y + oy, x + ox) is inside the image
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
                gc = g(len2(u[P] - uq), s2c)
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
            den[P] = np.where(add, den[P] + w, den[P])
    return (num / den[..., None]).astype(F32)


def denoise_ref(color, albedo, normal, iterations=3, flags=0, sigma_color=1.0, sigma_normal=0.5, sigma_depth=0.1,
                sigma_albedo=np.inf):
    """Expected output of rtmi_denoise for (H, W, 4) float32 images: (H, W, 4) float32 with lane 3 = 0."""
    color, albedo, normal = (np.ascontiguousarray(x, F32) for x in (color, albedo, normal))
    assert color.ndim == 3 and color.shape[2] == 4 and color.shape == albedo.shape == normal.shape
    sc, sn, sd, sa = F32(sigma_color), F32(sigma_normal), F32(sigma_depth), F32(sigma_albedo)
    a, cov = albedo[..., 0:3], albedo[..., 3]
    n, d = normal[..., 0:3], normal[..., 3]
    with np.errstate(all="ignore"):
        mod = a + EPS
        u = color[..., 0:3] / mod if flags & DEMODULATE else color[..., 0:3].copy()
        s2c = sc * sc
        scale = F32(1.0)
        for i in range(int(iterations)):
            u = atrous_iteration(u, a, cov, n, d, 1 << i, sn * sn, sd, sa * sa, F32(s2c * scale))
            scale = F32(scale * F32(0.25))
        if flags & DEMODULATE:
            u = u * mod
    out = np.zeros(color.shape, F32)
    out[..., 0:3] = u
    return out
