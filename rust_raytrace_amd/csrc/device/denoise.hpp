// denoise.hpp — the feature-guided a-trous filter of rtmi_denoise* (include/rtmi.h states it operation by operation;
// DESIGN.md 4.12).  One launch of k_atrous is one iteration: a thread owns one pixel and sums its 25 taps in the stated order
// (dy outer, dx inner), so the result does not depend on the tile shape, on the staging or on the launch geometry.
// Only + - * / and comparisons in f32 (-ffp-contract=off): tests/denoise_ref.py repeats them in NumPy, bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace rtmi {

constexpr int DN_TW = 32, DN_TH = 8;      // pixels of a block's tile: one thread per pixel, a wave covers two rows of 32
constexpr uint32_t DN_LDS_MAX_STEP = 2;   // largest tap spacing whose tile + halo is staged through LDS (40 x 16 pixels = 30 KB)
enum { DN_DEMOD_IN = 1u, DN_REMOD_OUT = 2u };  // first / last launch of a call with RTMI_DENOISE_DEMODULATE

// Per-launch constants: sigma^2 of the normal, albedo and colour terms (the colour's already scaled by 4^-i), sigma of depth.
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
// Weight of a tap q != p; kk = k[dy+2] * k[dx+2], s2d = (sigma_depth * d_p)^2
__device__ __forceinline__ float dn_weight(float kk, const DnPix& p, const DnPix& q, const DenoiseK& k, float s2d) {
    const float gc = dn_g(dn_len2(p.ux - q.ux, p.uy - q.uy, p.uz - q.uz), k.s2c);
    if (p.cov == 0.f && q.cov == 0.f) return kk * gc;  // sky beside sky: the guides say nothing
    float w = kk * dn_g(dn_len2(p.nx - q.nx, p.ny - q.ny, p.nz - q.nz), k.s2n);
    const float dd = p.d - q.d, dc = p.cov - q.cov;
    w = w * dn_g(dd * dd, s2d);
    w = w * dn_g(dc * dc, 0.25f);
    w = w * dn_g(dn_len2(p.ax - q.ax, p.ay - q.ay, p.az - q.az), k.s2a);
    return w * gc;
}

// One iteration at tap spacing `step` over a W x H image: src -> dst (never the same buffer).  flags: DN_DEMOD_IN divides the
// colours read from src by (albedo + 1/256), DN_REMOD_OUT multiplies the result by the pixel's.  Blocks walk the 32 x 8 tiles
// of the image grid-stride.  STAGE: the tile and its halo of 2 * step pixels go through LDS first (three float4 per pixel,
// dynamic LDS of (32 + 4 step) * (8 + 4 step) * 48 B), demodulated once there; otherwise every tap is three global loads.
template <bool STAGE>
__global__ void __launch_bounds__(DN_TW * DN_TH) k_atrous(uint32_t W, uint32_t H, uint32_t step, const float4* __restrict__ src,
                                                          const float4* __restrict__ albedo, const float4* __restrict__ normal,
                                                          float4* __restrict__ dst, DenoiseK prm, uint32_t flags) {
    extern __shared__ float4 dn_lds[];
    const bool demod = (flags & DN_DEMOD_IN) != 0;
    const uint32_t tiles_x = (W + DN_TW - 1) / DN_TW, tiles_y = (H + DN_TH - 1) / DN_TH;
    const uint32_t ntiles = tiles_x * tiles_y;  // fits: W * H < 2^32 is the caller's check
    const int lx = threadIdx.x % DN_TW, ly = threadIdx.x / DN_TW;
    const int halo = 2 * (int)step, tw = DN_TW + 2 * halo, th = DN_TH + 2 * halo;
    const float kern[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t x0 = (int64_t)(tile % tiles_x) * DN_TW, y0 = (int64_t)(tile / tiles_x) * DN_TH;
        const int64_t x = x0 + lx, y = y0 + ly;
        if (STAGE) {
            float4* s_u = dn_lds;
            float4* s_a = dn_lds + tw * th;
            float4* s_n = dn_lds + 2 * tw * th;
            __syncthreads();  // the previous tile's taps are done
            for (int i = threadIdx.x; i < tw * th; i += DN_TW * DN_TH) {
                const int64_t gx = x0 - halo + i % tw, gy = y0 - halo + i / tw;
                if (gx >= 0 && gx < (int64_t)W && gy >= 0 && gy < (int64_t)H) {  // a slot outside the image is never read
                    const size_t g = (size_t)gy * W + (size_t)gx;
                    float4 c = src[g];
                    const float4 a = albedo[g];
                    if (demod) { c.x = c.x / (a.x + 0.00390625f); c.y = c.y / (a.y + 0.00390625f); c.z = c.z / (a.z + 0.00390625f); }
                    s_u[i] = c; s_a[i] = a; s_n[i] = normal[g];
                }
            }
            __syncthreads();
        }
        if (x >= (int64_t)W || y >= (int64_t)H) continue;
        const size_t pi = (size_t)y * W + (size_t)x;
        const int li = (ly + halo) * tw + lx + halo;
        const DnPix p = STAGE ? dn_pix(dn_lds[li], dn_lds[tw * th + li], dn_lds[2 * tw * th + li], false)
                              : dn_pix(src[pi], albedo[pi], normal[pi], demod);
        const float sdp = prm.sd * p.d, s2d = sdp * sdp;
        float nr = 0.f, ng = 0.f, nb = 0.f, den = 0.f;
#pragma unroll
        for (int dy = -2; dy <= 2; dy++) {
#pragma unroll
            for (int dx = -2; dx <= 2; dx++) {
                const float kk = kern[dy + 2] * kern[dx + 2];
                if (dx == 0 && dy == 0) {  // the centre: always, with its full weight
                    nr = nr + kk * p.ux; ng = ng + kk * p.uy; nb = nb + kk * p.uz; den = den + kk;
                    continue;
                }
                const int64_t qx = x + (int64_t)dx * step, qy = y + (int64_t)dy * step;
                if (qx < 0 || qx >= (int64_t)W || qy < 0 || qy >= (int64_t)H) continue;
                DnPix q;
                if (STAGE) {
                    const int qi = li + dy * (int)step * tw + dx * (int)step;
                    q = dn_pix(dn_lds[qi], dn_lds[tw * th + qi], dn_lds[2 * tw * th + qi], false);
                } else {
                    const size_t g = (size_t)qy * W + (size_t)qx;
                    q = dn_pix(src[g], albedo[g], normal[g], demod);
                }
                const float w = dn_weight(kk, p, q, prm, s2d);
                if (w > 0.f) { nr = nr + w * q.ux; ng = ng + w * q.uy; nb = nb + w * q.uz; den = den + w; }
            }
        }
        float r = nr / den, g = ng / den, b = nb / den;
        if (flags & DN_REMOD_OUT) { r = r * (p.ax + 0.00390625f); g = g * (p.ay + 0.00390625f); b = b * (p.az + 0.00390625f); }
        dst[pi] = make_float4(r, g, b, 0.f);
    }
}

}  // namespace rtmi
