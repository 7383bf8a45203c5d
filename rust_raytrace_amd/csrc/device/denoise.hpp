// denoise.hpp — the a-trous filter of rtmi_denoise* and rtmi_denoise_var*, and the variance image of rtmi_variance*
// (include/rtmi.h states them operation by operation).  One launch of k_atrous is one iteration of either
// filter: a thread owns one pixel and sums its 25 taps in the stated order (dy outer, dx inner), so the result does not depend
// on the tile shape, on the staging or on the launch geometry.  VAR, the variance-guided filter, is the plain one with a colour
// width per pixel, taken from the 3 x 3 prefilter of the pixel's variance, and with the variance carried along.  Only + - * /
// and comparisons in f32 (-ffp-contract=off): tests/denoise_ref.py and tests/denoise_var_ref.py repeat them in NumPy, bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace rtmi {

constexpr int DN_TW = 32, DN_TH = 8;      // pixels of a block's tile: one thread per pixel, a wave covers two rows of 32
// largest tap spacing whose tile + halo is staged through LDS (40 x 16 pixels = 30 KB, 40 KB with the variance)
constexpr uint32_t DN_LDS_MAX_STEP = 2;
enum { DN_DEMOD_IN = 1u, DN_REMOD_OUT = 2u };  // first / last launch of a call with RTMI_DENOISE_DEMODULATE

// Per-launch constants: sigma^2 of the normal, albedo and colour terms, sigma of depth.  s2c: plain, already scaled by 4^-i;
// VAR, in variances of the pixel.
struct DenoiseK { float s2n, sd, s2a, s2c; };

// What a tap reads of a pixel: the running colour u, and the guides
struct DnPix { float ux, uy, uz, ax, ay, az, cov, nx, ny, nz, d; };

// Tukey's biweight; a NaN argument or s2 <= x2 gives 0
__device__ __forceinline__ float dn_g(float x2, float s2) {
    if (x2 < s2) { const float t = 1.f - x2 / s2; return t * t; }
    return 0.f;
}
__device__ __forceinline__ float dn_len2(float x, float y, float z) {
    float s = 0.f;
    s = s + x * x; s = s + y * y; s = s + z * z;
    return s;
}
__device__ __forceinline__ DnPix dn_pix(const float4 c, const float4 a, const float4 n, bool demod) {
    DnPix p{c.x, c.y, c.z, a.x, a.y, a.z, a.w, n.x, n.y, n.z, n.w};
    if (demod) { p.ux = c.x / (a.x + 0.00390625f); p.uy = c.y / (a.y + 0.00390625f); p.uz = c.z / (a.z + 0.00390625f); }
    return p;
}
// Weight of a tap q != p; kk = k[dy+2] * k[dx+2], s2d = (sigma_depth * d_p)^2, s2c = the colour width (of pixel p, with VAR)
__device__ __forceinline__ float dn_weight(float kk, const DnPix& p, const DnPix& q, const DenoiseK& k, float s2d, float s2c) {
    const float gc = dn_g(dn_len2(p.ux - q.ux, p.uy - q.uy, p.uz - q.uz), s2c);
    if (p.cov == 0.f && q.cov == 0.f) return kk * gc;  // sky beside sky: the guides say nothing
    float w = kk * dn_g(dn_len2(p.nx - q.nx, p.ny - q.ny, p.nz - q.nz), k.s2n);
    const float dd = p.d - q.d, dc = p.cov - q.cov;
    w = w * dn_g(dd * dd, s2d);
    w = w * dn_g(dc * dc, 0.25f);
    w = w * dn_g(dn_len2(p.ax - q.ax, p.ay - q.ay, p.az - q.az), k.s2a);
    return w * gc;
}

__device__ __forceinline__ float dnv_sum3(float x, float y, float z) {
    float s = 0.f;
    s = s + x; s = s + y; s = s + z;
    return s;
}

// The variance of the mean of every pixel from the moments an adaptive render leaves: s = accum, q = sumsq, n = count.
// The first two steps are adapt_stop's own arithmetic.  n < 2: nothing is known, +inf.
__global__ void __launch_bounds__(256) k_variance(uint64_t npixels, const float4* __restrict__ accum, const float4* __restrict__ sumsq,
                                                  const uint32_t* __restrict__ counts, float4* __restrict__ out) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < npixels; p += stride) {
        const uint32_t n = counts[p];
        if (n < 2u) { out[p] = make_float4(INFINITY, INFINITY, INFINITY, INFINITY); continue; }
        const float4 s = accum[p], q = sumsq[p];
        const float fn = (float)n, inv = 1.f / fn, dn1 = (float)(n - 1u);
        const float mr = s.x * inv, mg = s.y * inv, mb = s.z * inv;
        float vr = (q.x - s.x * mr) / dn1, vg = (q.y - s.y * mg) / dn1, vb = (q.z - s.z * mb) / dn1;
        vr = vr / fn; vg = vg / fn; vb = vb / fn;
        vr = vr < 0.f ? 0.f : vr; vg = vg < 0.f ? 0.f : vg; vb = vb < 0.f ? 0.f : vb;  // a NaN stays
        out[p] = make_float4(vr, vg, vb, dnv_sum3(vr, vg, vb));
    }
}

// The variance a tap reads of a pixel; demod: divided twice by (albedo + 1/256), lane 3 summed again
__device__ __forceinline__ float4 dnv_var(float4 v, const float4 a, bool demod) {
    if (demod) {
        v.x = (v.x / (a.x + 0.00390625f)) / (a.x + 0.00390625f);
        v.y = (v.y / (a.y + 0.00390625f)) / (a.y + 0.00390625f);
        v.z = (v.z / (a.z + 0.00390625f)) / (a.z + 0.00390625f);
        v.w = dnv_sum3(v.x, v.y, v.z);
    }
    return v;
}

// One iteration at tap spacing `step` over a W x H image: src -> dst (never the same buffer).  flags: DN_DEMOD_IN divides the
// colours read from src by (albedo + 1/256), DN_REMOD_OUT multiplies the result by the pixel's.  Blocks walk the 32 x 8 tiles
// of the image grid-stride.  STAGE: the tile and its halo of 2 * step pixels go through LDS first (one float4 per image and
// pixel, dynamic LDS of (32 + 4 step) * (8 + 4 step) * 16 B * the number of images), demodulated once there; otherwise every
// tap is one global load per image.
// VAR: a fourth image, the variance, is carried along: (src, vsrc) -> (dst, vdst), no two the same buffer; vdst may be NULL
// (the last iteration of a call without var_out).  DN_DEMOD_IN divides the variances read from vsrc by (albedo + 1/256)^2,
// DN_REMOD_OUT multiplies them back.  The colour width of a pixel is prm.s2c times the 3 x 3 prefilter of its variance, which
// reads the staged tile with STAGE (the halo is >= 2).  Without VAR, vsrc and vdst are not used and everything behind
// `if (VAR)` compiles away.
template <bool STAGE, bool VAR>
__global__ void __launch_bounds__(DN_TW * DN_TH) k_atrous(uint32_t W, uint32_t H, uint32_t step, const float4* __restrict__ src,
                                                          const float4* __restrict__ vsrc, const float4* __restrict__ albedo,
                                                          const float4* __restrict__ normal, float4* __restrict__ dst,
                                                          float4* __restrict__ vdst, DenoiseK prm, uint32_t flags) {
    extern __shared__ float4 dn_lds[];
    const bool demod = (flags & DN_DEMOD_IN) != 0;
    const uint32_t tiles_x = (W + DN_TW - 1) / DN_TW, tiles_y = (H + DN_TH - 1) / DN_TH;
    const uint32_t ntiles = tiles_x * tiles_y;  // fits: W * H < 2^32 is the caller's check
    const int lx = threadIdx.x % DN_TW, ly = threadIdx.x / DN_TW;
    const int halo = 2 * (int)step, tw = DN_TW + 2 * halo, th = DN_TH + 2 * halo;
    const float kern[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    const float k3[3] = {0.25f, 0.5f, 0.25f};
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t x0 = (int64_t)(tile % tiles_x) * DN_TW, y0 = (int64_t)(tile / tiles_x) * DN_TH;
        const int64_t x = x0 + lx, y = y0 + ly;
        if (STAGE) {
            float4* s_u = dn_lds;
            float4* s_a = dn_lds + tw * th;
            float4* s_n = dn_lds + 2 * tw * th;
            float4* s_v = dn_lds + 3 * tw * th;
            __syncthreads();  // the previous tile's taps are done
            for (int i = threadIdx.x; i < tw * th; i += DN_TW * DN_TH) {
                const int64_t gx = x0 - halo + i % tw, gy = y0 - halo + i / tw;
                if (gx >= 0 && gx < (int64_t)W && gy >= 0 && gy < (int64_t)H) {  // a slot outside the image is never read
                    const size_t g = (size_t)gy * W + (size_t)gx;
                    float4 c = src[g];
                    const float4 a = albedo[g];
                    if (demod) { c.x = c.x / (a.x + 0.00390625f); c.y = c.y / (a.y + 0.00390625f); c.z = c.z / (a.z + 0.00390625f); }
                    s_u[i] = c; s_a[i] = a; s_n[i] = normal[g];
                    if (VAR) s_v[i] = dnv_var(vsrc[g], a, demod);
                }
            }
            __syncthreads();
        }
        if (x >= (int64_t)W || y >= (int64_t)H) continue;
        const size_t pi = (size_t)y * W + (size_t)x;
        const int li = (ly + halo) * tw + lx + halo;
        const DnPix p = STAGE ? dn_pix(dn_lds[li], dn_lds[tw * th + li], dn_lds[2 * tw * th + li], false)
                              : dn_pix(src[pi], albedo[pi], normal[pi], demod);
        float4 vp = make_float4(0.f, 0.f, 0.f, 0.f);
        float s2c = prm.s2c;
        if (VAR) {
            vp = STAGE ? dn_lds[3 * tw * th + li] : dnv_var(vsrc[pi], albedo[pi], demod);
            // the colour width of this pixel: sigma_color^2 times the 3 x 3 prefilter of the variance's lane 3, taps at spacing 1
            float gnum = 0.f, gden = 0.f;
#pragma unroll
            for (int dy = -1; dy <= 1; dy++) {
#pragma unroll
                for (int dx = -1; dx <= 1; dx++) {
                    const int64_t qx = x + dx, qy = y + dy;
                    if (qx < 0 || qx >= (int64_t)W || qy < 0 || qy >= (int64_t)H) continue;
                    const float kk = k3[dy + 1] * k3[dx + 1];
                    float vs;
                    if (dx == 0 && dy == 0) vs = vp.w;
                    else if (STAGE) vs = dn_lds[3 * tw * th + li + dy * tw + dx].w;
                    else {
                        const size_t g = (size_t)qy * W + (size_t)qx;
                        vs = demod ? dnv_var(vsrc[g], albedo[g], true).w : vsrc[g].w;
                    }
                    gnum = gnum + kk * vs; gden = gden + kk;
                }
            }
            s2c = prm.s2c * (gnum / gden) + 0x1p-40f;
        }
        const float sdp = prm.sd * p.d, s2d = sdp * sdp;
        float nr = 0.f, ng = 0.f, nb = 0.f, den = 0.f, vr = 0.f, vg = 0.f, vb = 0.f;
#pragma unroll
        for (int dy = -2; dy <= 2; dy++) {
#pragma unroll
            for (int dx = -2; dx <= 2; dx++) {
                const float kk = kern[dy + 2] * kern[dx + 2];
                if (dx == 0 && dy == 0) {  // the centre: always, with its full weight
                    nr = nr + kk * p.ux; ng = ng + kk * p.uy; nb = nb + kk * p.uz; den = den + kk;
                    if (VAR) { const float k2 = kk * kk; vr = vr + k2 * vp.x; vg = vg + k2 * vp.y; vb = vb + k2 * vp.z; }
                    continue;
                }
                const int64_t qx = x + (int64_t)dx * step, qy = y + (int64_t)dy * step;
                if (qx < 0 || qx >= (int64_t)W || qy < 0 || qy >= (int64_t)H) continue;
                const int qi = li + dy * (int)step * tw + dx * (int)step;  // the tap's slot of the staged tile (STAGE)
                const size_t g = (size_t)qy * W + (size_t)qx;              // the tap's pixel of the image (direct)
                DnPix q;
                float4 qa = make_float4(0.f, 0.f, 0.f, 0.f);  // direct VAR: the tap's albedo, which demodulates its variance too
                if (STAGE) q = dn_pix(dn_lds[qi], dn_lds[tw * th + qi], dn_lds[2 * tw * th + qi], false);
                else if (VAR) { qa = albedo[g]; q = dn_pix(src[g], qa, normal[g], demod); }  // albedo first: the order of the
                else q = dn_pix(src[g], albedo[g], normal[g], demod);  // loads is each filter's own (measured)
                const float w = dn_weight(kk, p, q, prm, s2d, s2c);
                if (w > 0.f) {
                    // VAR: STAGE and direct share this body, because either way a tap's variance is read only when w > 0
                    // (direct: a fourth global load), and before the colour sums
                    const float4 vq = !VAR ? make_float4(0.f, 0.f, 0.f, 0.f) : STAGE ? dn_lds[3 * tw * th + qi] : dnv_var(vsrc[g], qa, demod);
                    const float w2 = w * w;
                    nr = nr + w * q.ux; ng = ng + w * q.uy; nb = nb + w * q.uz; den = den + w;
                    if (VAR) { vr = vr + w2 * vq.x; vg = vg + w2 * vq.y; vb = vb + w2 * vq.z; }
                }
            }
        }
        float r = nr / den, g = ng / den, b = nb / den;
        if (VAR) { const float d2 = den * den; vr = vr / d2; vg = vg / d2; vb = vb / d2; }
        if (flags & DN_REMOD_OUT) {
            const float mx = p.ax + 0.00390625f, my = p.ay + 0.00390625f, mz = p.az + 0.00390625f;
            r = r * mx; g = g * my; b = b * mz;
            if (VAR) { vr = (vr * mx) * mx; vg = (vg * my) * my; vb = (vb * mz) * mz; }
        }
        dst[pi] = make_float4(r, g, b, 0.f);
        if (VAR && vdst) vdst[pi] = make_float4(vr, vg, vb, dnv_sum3(vr, vg, vb));
    }
}

}  // namespace rtmi
