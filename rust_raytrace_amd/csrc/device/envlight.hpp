// envlight.hpp — sampling the environment at matte hits (rtmi_render_envlight*, rtmi_scene_get_env_sampler; include/rtmi.h
// "SAMPLING THE ENVIRONMENT" defines it operation by operation): the sampler table of a scene's environment
// (three kernels) and the two elementwise kernels of the pass, which is rtmi_render_shadowed*'s pass structure.  Per pass j:
//   (the scene's closest-hit launch of path queue j)
//   k_envlight_rays   one candidate shadow ray per queue entry that hit a Matte surface that bounces, towards a direction drawn
//                     from the map's brightness; the live ones compacted into shadow queue j as k_shadow_rays does it, with
//                     L * wgt per entry
//   (the occlusion walk of shadow queue j: launch_occluded, on an octree through the closest-hit launch)
//   k_shade_envlight  shade_hit's plain arm with the direct light of the level on a stack beside the surface stack and the
//                     bounce's own balance weight in one float per path, applied where the path escapes
// The rays, the RNG blocks 0 .. maxdepth and the queue order rules are shade_pass's.  Included by rtmi_device.hip after
// shadowed.hpp, whose slot values it uses.
#pragma once

namespace rtmi {

#define RTMI_ENVQ_SCALE 1048576.f  // the quantised weight of the brightest texel (2^20)

// The sampler of an environment: q[j * n + i] = the texel's integer weight (>= 1), ex[j * n + i] = the sum of the q left of it
// in its row (< 2^32 for n <= 4096), rows[j] = the sum of the rows above row j, rows[n] = total.  C, the inclusive prefix sum
// in row-major order, is rows[j] + ex[j * n + i] + q[j * n + i].
struct EnvSampler { const uint32_t* __restrict__ q; const uint32_t* __restrict__ ex; const unsigned long long* __restrict__ rows; unsigned long long total; };

// w of texel (i, j): lum / r^3 at the texel centre's map point, the point as k_env_sky computes it before normalising
__device__ inline float envq_weight(const float4* __restrict__ tab, uint32_t n, float fn, uint32_t i, uint32_t j) {
    const float4 c = tab[(size_t)j * n + i];
    float lum = (c.x + c.y) + c.z;
    if (!(lum > 0.f) || !(lum <= FLT_MAX)) lum = 0.f;  // not > 0 (a NaN too) or not finite
    float px = ((float)i + 0.5f) / fn * 2.f - 1.f, py = ((float)j + 0.5f) / fn * 2.f - 1.f;
    const float z = (1.f - fabsf(px)) - fabsf(py);
    if (z < 0.f) oct_fold(px, py);
    const float r2 = (px * px + py * py) + z * z;
    float w = lum / (r2 * sqrtf(r2));
    if (!(w <= FLT_MAX)) w = 0.f;  // overflowed
    return w;
}

// wmax: the maximum of w over the table.  One thread per texel, one atomic per block; w >= 0, so the bit patterns order as
// the floats do, and a maximum is exact in any order.
__global__ void __launch_bounds__(256) k_envq_max(const float4* __restrict__ tab, uint32_t n, float fn, uint32_t* __restrict__ wmax_bits) {
    __shared__ uint32_t s_max[4];
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t b = 0u;
    if (k < n * n) {
        const uint32_t j = k / n, i = k - j * n;
        b = __float_as_uint(envq_weight(tab, n, fn, i, j));
    }
    for (int o = 32; o > 0; o >>= 1) b = max(b, (uint32_t)__shfl_xor((int)b, o));
    if ((threadIdx.x & 63u) == 0u) s_max[threadIdx.x >> 6] = b;
    __syncthreads();
    if (threadIdx.x == 0) atomicMax(wmax_bits, max(max(s_max[0], s_max[1]), max(s_max[2], s_max[3])));
}

// q and the in-row exclusive prefix sums: a wave per row (four rows per block), 64 columns at a time with a cross-lane scan
// and a running carry; rowsum[j] = the row's total.
__global__ void __launch_bounds__(256) k_envq_rows(const float4* __restrict__ tab, uint32_t n, float fn, const uint32_t* __restrict__ wmax_bits,
                                                   uint32_t* __restrict__ q, uint32_t* __restrict__ ex, unsigned long long* __restrict__ rowsum) {
    const uint32_t lane = threadIdx.x & 63u, j = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (j >= n) return;  // whole waves leave together
    const float wmax = __uint_as_float(*wmax_bits);
    const float scale = RTMI_ENVQ_SCALE / wmax;
    unsigned long long carry = 0ull;
    for (uint32_t i0 = 0; i0 < n; i0 += 64u) {
        const uint32_t i = i0 + lane;
        uint32_t qq = 0u;
        if (i < n) {
            qq = 1u;
            if (wmax != 0.f) {
                float s = envq_weight(tab, n, fn, i, j) * scale;
                s = !(s >= 0.f) ? 0.f : (s > RTMI_ENVQ_SCALE ? RTMI_ENVQ_SCALE : s);
                qq = 1u + (uint32_t)s;
            }
        }
        unsigned long long inc = qq;  // inclusive scan over the wave's 64 columns
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned long long up = __shfl_up(inc, o);
            if ((int)lane >= o) inc += up;
        }
        if (i < n) {
            q[(size_t)j * n + i] = qq;
            ex[(size_t)j * n + i] = (uint32_t)(carry + inc - qq);
        }
        carry += __shfl(inc, 63);
    }
    if (lane == 0) rowsum[j] = carry;
}

// rows[j] = the sum of rowsum[0 .. j), rows[n] = total: one block, every thread a run of consecutive rows (n <= 4096: at most 16)
__global__ void __launch_bounds__(256) k_envq_scan(const unsigned long long* __restrict__ rowsum, uint32_t n, unsigned long long* __restrict__ rows) {
    __shared__ unsigned long long s_sum[256];
    const uint32_t per = (n + 255u) / 256u, j0 = threadIdx.x * per, j1 = min(j0 + per, n);
    unsigned long long sum = 0ull;
    for (uint32_t j = j0; j < j1; j++) sum += rowsum[j];
    s_sum[threadIdx.x] = sum;
    __syncthreads();
    unsigned long long base = 0ull;
    for (uint32_t t = 0; t < threadIdx.x; t++) base += s_sum[t];
    for (uint32_t j = j0; j < j1; j++) { rows[j] = base; base += rowsum[j]; }
    if (threadIdx.x == 255u) rows[n] = base;  // (the last thread's run ends at n, or is empty behind it)
}

// env_lookup's own mapping of a world unit direction d to the texel that holds it, and a = the L1 norm of its map-space vector
__device__ inline uint32_t envq_texel_of(const EnvTab& e, V4 d, float& a) {
    auto v4 = [](float4 q) { return V4{q.x, q.y, q.z, q.w}; };
    const float mx = vdot(v4(e.r0), d), my = vdot(v4(e.r1), d), mz = vdot(v4(e.r2), d);
    a = (fabsf(mx) + fabsf(my)) + fabsf(mz);
    float px = mx / a, py = my / a;
    if (mz < 0.f) oct_fold(px, py);
    const float top = e.fn - 1.f;
    float gx = floorf((px * 0.5f + 0.5f) * e.fn), gy = floorf((py * 0.5f + 0.5f) * e.fn);
    gx = !(gx >= 0.f) ? 0.f : (gx > top ? top : gx);
    gy = !(gy >= 0.f) ? 0.f : (gy > top ? top : gy);
    return (uint32_t)gy * e.n + (uint32_t)gx;
}
// pe: the environment pdf per solid angle of a world unit direction d
__device__ inline float env_pdf(const EnvTab& e, const EnvSampler& es, V4 d) {
    float a;
    const uint32_t k = envq_texel_of(e, d, a);
    return (((float)es.q[k] / (float)es.total) * ((e.fn * e.fn) * 0.25f)) / ((a * a) * a);
}
// pb: the pdf per solid angle of the reference's Matte bounce dir = unit(n + s) at d, s the random_vec behind d
__device__ inline float bounce_pdf(V4 n, V4 d, V4 s) {
    const float c = vdot(n, d);
    const float m = fmaxf(fmaxf(fabsf(s.x), fabsf(s.y)), fabsf(s.z));
    const float p = c / (6.f * ((m * m) * m));
    return c > 0.f ? p : 0.f;
}

// One thread per entry of path queue `pass`; the compaction is k_shadow_rays' (ballot + popcount per wave, ONE atomic per block
// on sctrl->count[pass + 1]).  lw[q] = L * wgt of shadow queue entry q.
__global__ void __launch_bounds__(256) k_envlight_rays(DScene sc, DView v, uint64_t seed, uint32_t pix0, int pass, EnvTab env, EnvSampler es,
                                                       float bias, const float4* __restrict__ qo, const float4* __restrict__ qd,
                                                       const uint32_t* __restrict__ qpath, const uint32_t* __restrict__ hit_tf,
                                                       const float* __restrict__ hit_t, const DCtrl* __restrict__ ctrl,
                                                       float4* __restrict__ lq_o, float4* __restrict__ lq_d, float4* __restrict__ lw,
                                                       uint32_t* __restrict__ slot, DCtrl* __restrict__ sctrl) {
    __shared__ uint32_t s_cnt[4], s_base;
    auto v4 = [](float4 q) { return V4{q.x, q.y, q.z, q.w}; };
    const uint32_t count = ctrl->count[pass];
    const uint32_t stride = gridDim.x * blockDim.x;
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint32_t bound = (count + 255u) & ~255u;  // whole blocks stay converged for the ballots and the barriers
    // (launched for the passes whose Matte hits bounce, maxdepth - pass - 1 != 0: an exhausted level gets no sample)
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < bound; i += stride) {
        bool live = false;
        V4 o{}, omega{}, Lw{};
        if (i < count) {
            const uint32_t tf = hit_tf[i], tri = tf & 0x3FFFFFFFu;
            if (tri != 0u && !((tf >> 30) & 2u)) {
                const float4 p1 = sc.tplane[2 * tri + 1];
                const float4 m1 = sc.mats[2 * __float_as_uint(p1.w) + 1];
                if (__float_as_uint(m1.y) == RTMI_MATTE) {
                    const float t = hit_t[i];
                    const float4 o4 = qo[i], d4 = qd[i];
                    const V4 point = vadd(vmul(V4{d4.x, d4.y, d4.z, d4.w}, t), V4{o4.x, o4.y, o4.z, o4.w});
                    V4 n = mk(p1.x, p1.y, p1.z);
                    if ((tf >> 30) & 1u) n = vmul(n, -1.f);
                    uint32_t row, col, sample;
                    path_pixel<Samp::PASS>(v, pix0, qpath[i], row, col, sample, nullptr);
                    uint32_t w[4];
                    rng_block(seed, row * v.width + col, sample, 0xC0000000u | (uint32_t)pass, w);
                    // the texel: the first k with C[k] > T, by binary search over the row starts, then inside the row
                    const unsigned long long T = __umul64hi(((unsigned long long)w[0] << 32) | w[1], es.total);
                    uint32_t lo = 0u, hi = env.n - 1u;  // the last row j with rows[j] <= T
                    while (lo < hi) {
                        const uint32_t mid = (lo + hi + 1u) >> 1;
                        if (es.rows[mid] <= T) lo = mid; else hi = mid - 1u;
                    }
                    const uint32_t tj = lo;
                    const unsigned long long tr = T - es.rows[tj];
                    const uint32_t* __restrict__ exr = es.ex + (size_t)tj * env.n;
                    lo = 0u; hi = env.n - 1u;  // the last column i with ex[i] <= tr
                    while (lo < hi) {
                        const uint32_t mid = (lo + hi + 1u) >> 1;
                        if ((unsigned long long)exr[mid] <= tr) lo = mid; else hi = mid - 1u;
                    }
                    const uint32_t ti = lo;
                    float px = ((float)ti + u32_to_unit_f32(w[2])) / env.fn * 2.f - 1.f, py = ((float)tj + u32_to_unit_f32(w[3])) / env.fn * 2.f - 1.f;
                    const float z = (1.f - fabsf(px)) - fabsf(py);
                    if (z < 0.f) oct_fold(px, py);
                    const V4 m = vunit(mk(px, py, z));
                    omega = vunit(vadd(vadd(vmul(v4(env.r0), m.x), vmul(v4(env.r1), m.y)), vmul(v4(env.r2), m.z)));
                    const float c = vdot(n, omega);
                    const V4 s = vsub(vmul(omega, 2.f * c), n);  // the random_vec whose bounce is omega
                    o = vadd(point, vmul(s, bias));              // ... and where that bounce ray would start: the same visibility
                    if (c > 0.f) {
                        const V4 L = env_lookup(env, omega);
                        const float pbv = bounce_pdf(n, omega, s);
                        const float wgt = pbv / (pbv + env_pdf(env, es, omega));
                        live = wgt > 0.f && (L.x != 0.f || L.y != 0.f || L.z != 0.f);
                        Lw = vmul(L, wgt);
                    }
                }
            }
        }
        const unsigned long long mask = __ballot(live);
        if (lane == 0) s_cnt[wv] = (uint32_t)__popcll(mask);
        __syncthreads();
        if (threadIdx.x == 0) {
            const uint32_t total = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
            s_base = total ? atomicAdd(&sctrl->count[pass + 1], total) : 0u;
        }
        __syncthreads();
        if (live) {
            uint32_t q = s_base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
            for (uint32_t k = 0; k < wv; k++) q += s_cnt[k];
            store_stream(&lq_o[q], make_float4(o.x, o.y, o.z, o.w));
            store_stream(&lq_d[q], make_float4(omega.x, omega.y, omega.z, omega.w));
            store_stream(&lw[q], make_float4(Lw.x, Lw.y, Lw.z, Lw.w));
            store_stream(&slot[i], q);
        } else if (i < count) {
            store_stream(&slot[i], RTMI_SHADOW_NONE);
        }
        __syncthreads();  // s_cnt / s_base are rewritten by the next iteration
    }
}

// shade_hit's plain arm (Solid, Matte, Reflective, flat triangles) for ONE traced ray of an envlight path: the same rays, stack
// and return value.  `direct` is the level's sampled light (L * wgt where the candidate was live and not occluded, else 0):
// stored on dstack[pass][path] whenever a level is pushed (0 for a Reflective level and at exhausted depth).  wbuf[path] holds the
// balance weight of the path's last bounce (1.f for a Reflective one), read from pass 1 on where the path escapes.  The fold:
// c = mix_color(color_j, c + direct_j, alpha_j), inside-out.
__device__ inline bool shade_hit_envlight(const DScene& sc, const EnvTab& env, const EnvSampler& es, uint32_t maxdepth, uint64_t seed,
                                          uint32_t npaths, uint32_t path, uint32_t pixel, uint32_t sample, uint32_t pass, uint32_t tf, float t,
                                          V4 ro, V4 rd, V4 direct, uint16_t* __restrict__ mstack, float4* __restrict__ dstack,
                                          float* __restrict__ wbuf, float4* __restrict__ scol, RayV& nr) {
    const uint32_t tri = tf & 0x3FFFFFFFu, face = tf >> 30;
    const V4 black = mk(0.f / 255.f, 0.f / 255.f, 0.f / 255.f);
    V4 c;
    uint32_t npushed = pass;
    if (tri == 0) {
        c = vmul(env_lookup(env, rd), pass ? wbuf[path] : 1.f);
    } else if (face & 2u) {
        c = black;  // edge faces are Solid black, raytrace.rs:452-457
    } else {
        const float4 p1 = sc.tplane[2 * tri + 1];  // triangles only: the caller refuses analytic spheres
        const uint32_t mat = __float_as_uint(p1.w);
        const float4 m0 = sc.mats[2 * mat], m1 = sc.mats[2 * mat + 1];
        const uint32_t kind = __float_as_uint(m1.y);
        if (kind == RTMI_SOLID) {
            c = mk(m0.x, m0.y, m0.z);
        } else {
            mstack[(size_t)pass * npaths + path] = (uint16_t)mat;
            npushed = pass + 1;
            c = black;  // project_ray at depth 0, raytrace.rs:1261-1263
            if (maxdepth - pass - 1u != 0u) {
                const V4 point = vadd(vmul(rd, t), ro);  // Ray::at, raytrace.rs:227-229
                V4 norm = mk(p1.x, p1.y, p1.z);
                if (face & 1u) norm = vmul(norm, -1.f);  // raytrace.rs:441-449
                const V4 rv = random_vec(seed, pixel, sample, pass + 1u);
                float wb = 1.f;
                if (kind == RTMI_MATTE) {
                    nr = make_ray(vadd(point, vmul(rv, 0.001f)), vadd(norm, rv));  // lambertian_ray, :292-297
                    const float pbv = bounce_pdf(norm, nr.dir, rv);
                    wb = pbv / (pbv + env_pdf(env, es, nr.dir));
                } else {
                    const float ddot = fabsf(vdot(rd, norm));  // reflect_ray, :278-290
                    const V4 dir_p = vmul(norm, ddot);
                    const V4 dir_o = vadd(rd, dir_p);
                    const V4 reflect = vadd(dir_p, dir_o);
                    const V4 rvf = vmul(rv, m1.x);
                    const V4 reflect_dir = vunit(vadd(reflect, rvf));
                    nr = make_ray(vadd(point, vmul(reflect_dir, 0.001f)), vunit(vadd(reflect, rvf)));
                    direct = black;
                }
                store_stream(&dstack[(size_t)pass * npaths + path], make_float4(direct.x, direct.y, direct.z, direct.w));
                wbuf[path] = wb;
                return true;
            }
            dstack[(size_t)pass * npaths + path] = make_float4(0.f, 0.f, 0.f, 0.f);  // no sample at exhausted depth
        }
    }
    // inside-out evaluation of the nested mix_color calls (raytrace.rs:1233-1251), each level's inner colour plus its direct light
    for (int j = (int)npushed - 1; j >= 0; j--) {
        const uint32_t mj = mstack[(size_t)j * npaths + path];
        const float4 mm = sc.mats[2 * mj], dj = dstack[(size_t)j * npaths + path];
        c = mix_color(mk(mm.x, mm.y, mm.z), vadd(c, V4{dj.x, dj.y, dj.z, dj.w}), mm.w);
    }
    store_stream(&scol[path], make_float4(c.x, c.y, c.z, c.w));
    return false;
}

// k_shade_shadowed's loop with the entry's direct light for its shadow bit
__global__ void __launch_bounds__(256) k_shade_envlight(DScene sc, DView v, uint64_t seed, uint32_t pix0, uint32_t npaths, int pass, EnvTab env,
                                                        EnvSampler es, const float4* __restrict__ qo, const float4* __restrict__ qd,
                                                        const uint32_t* __restrict__ qpath, const uint32_t* __restrict__ hit_tf,
                                                        const float* __restrict__ hit_t, const uint32_t* __restrict__ slot,
                                                        const uint8_t* __restrict__ occ, const float4* __restrict__ lw,
                                                        float4* __restrict__ qo_n, float4* __restrict__ qd_n, uint32_t* __restrict__ qpath_n,
                                                        uint16_t* __restrict__ mstack, float4* __restrict__ dstack, float* __restrict__ wbuf,
                                                        float4* __restrict__ scol, DCtrl* __restrict__ ctrl) {
    __shared__ uint32_t s_cnt[4], s_base;
    const uint32_t count = ctrl->count[pass];
    const uint32_t stride = gridDim.x * blockDim.x;
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint32_t bound = (count + 255u) & ~255u;  // whole blocks stay converged for the ballot and the queue reservation
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < bound; i += stride) {
        bool push = false;
        RayV nr;
        uint32_t path = 0;
        if (i < count) {
            path = qpath[i];
            const uint32_t tf = hit_tf[i];
            float t = 0.f;
            const float4 o4 = qo[i], d4 = qd[i];  // (a miss looks the environment up in its ray's direction)
            V4 direct = mk(0.f, 0.f, 0.f);
            if ((tf & 0x3FFFFFFFu) != 0u && !((tf >> 30) & 2u)) {
                t = hit_t[i];
                // (the exhausted pass has no candidates: k_envlight_rays is not launched for it and the slots are stale)
                const uint32_t e = v.maxdepth - (uint32_t)pass - 1u != 0u ? slot[i] : RTMI_SHADOW_NONE;
                if (e != RTMI_SHADOW_NONE && occ[e] == 0) {
                    const float4 l4 = lw[e];
                    direct = V4{l4.x, l4.y, l4.z, l4.w};
                }
            }
            uint32_t prow, pcol, sample;
            path_pixel<Samp::PASS>(v, pix0, path, prow, pcol, sample, nullptr);
            push = shade_hit_envlight(sc, env, es, v.maxdepth, seed, npaths, path, prow * v.width + pcol, sample, (uint32_t)pass, tf, t,
                                      V4{o4.x, o4.y, o4.z, o4.w}, V4{d4.x, d4.y, d4.z, d4.w}, direct, mstack, dstack, wbuf, scol, nr);
        }
        const unsigned long long mask = __ballot(push);
        if (lane == 0) s_cnt[wv] = (uint32_t)__popcll(mask);
        __syncthreads();
        if (threadIdx.x == 0) {
            const uint32_t total = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
            s_base = total ? atomicAdd(&ctrl->count[pass + 1], total) : 0u;
        }
        __syncthreads();
        {
            uint32_t base = s_base;
            for (uint32_t k = 0; k < wv; k++) base += s_cnt[k];
            if (push) {
                const uint32_t q = base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
                store_stream(&qo_n[q], make_float4(nr.orig.x, nr.orig.y, nr.orig.z, nr.orig.w));
                store_stream(&qd_n[q], make_float4(nr.dir.x, nr.dir.y, nr.dir.z, nr.dir.w));
                store_stream(&qpath_n[q], path);
            }
        }
        __syncthreads();  // s_cnt / s_base are rewritten by the next iteration
    }
}

}  // namespace rtmi
