// emissive.hpp — sampling emissive triangles at matte hits (rtmi_scene_set_emitters, rtmi_render_emissive*,
// rtmi_scene_get_emitter_sampler; include/rtmi.h "EMISSIVE TRIANGLES" defines it operation by operation): the
// sampler table of a scene's lamps (two kernels) and the two elementwise kernels of the pass, which is rtmi_render_envlight*'s pass
// structure.  Per pass j:
//   (the scene's closest-hit launch of path queue j)
//   k_emissive_rays   one candidate shadow ray per queue entry that hit a Matte surface that bounces, towards a point drawn on the
//                     lamps by area * radiance; the live ones compacted into shadow queue j as k_lit_rays does it, with
//                     (pb, d2, the lamp's number) per entry
//   (the scene's closest-hit launch of shadow queue j, into hit records of its own)
//   k_shade_emissive  shade_hit's plain arm with the direct light of the level on a stack beside the surface stack (counted when
//                     the shadow ray's first hit is the lamp it was drawn on) and the bounce's own pb in one float per path,
//                     applied where the path's bounce ends on a lamp
// The rays, the RNG blocks 0 .. maxdepth and the queue order rules are shade_pass's.  Included by rtmi_device.hip after envlight.hpp
// (bounce_pdf, RTMI_ENVQ_SCALE) and shadowed.hpp (the slot values).
#pragma once

namespace rtmi {

#define RTMI_EMISSIVE_BLOCK 0xC0040000u  // | j: the RNG block of level j's candidate (lights 0 .. 3 of rtmi_render_lit* use 0xC000 .. 0xC003)
#define RTMI_EMISSIVE_NO_SAMPLE (-1.f)   // wbuf of a path whose last ray no sample stood beside: a primary ray, a Reflective bounce
#define RTMI_EMISSIVE_REC 5u             // float4 per lamp record

// The lamps of a scene.  lampidx[tri] = the lamp's number e (1-based, in triangle order), 0 for every other triangle.  Lamp e's
// record is lamp[5 * (e - 1) ..]: (c0, A), (e1, w), (e2, 0), (the record's unit normal, 0), (radiance, 0).  q[e - 1] = its integer
// weight (>= 1), cum[e - 1] = the inclusive prefix sum, total = cum[n - 1].
struct EmTab {
    const uint32_t* __restrict__ lampidx; const float4* __restrict__ lamp; const uint32_t* __restrict__ q;
    const unsigned long long* __restrict__ cum; unsigned long long total; uint32_t n;
};

// Lamp k (0-based) of the list tri[]: its record from the corners (3 float4 per lamp), the triangle record's normal and the
// surface's colour; wmax = the maximum of w.  One thread per lamp, one atomic per block (w >= 0: the bit patterns order as the floats).
__global__ void __launch_bounds__(256) k_emq_lamps(DScene sc, const uint32_t* __restrict__ tri, const float4* __restrict__ corners, uint32_t n,
                                                   float4* __restrict__ lamp, uint32_t* __restrict__ wmax_bits) {
    __shared__ uint32_t s_max[4];
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t b = 0u;
    if (k < n) {
        const uint32_t g = tri[k];
        const float4 a4 = corners[3 * k], b4 = corners[3 * k + 1], c4 = corners[3 * k + 2];
        const V4 c0 = mk(a4.x, a4.y, a4.z), e1 = vsub(mk(b4.x, b4.y, b4.z), c0), e2 = vsub(mk(c4.x, c4.y, c4.z), c0);
        const V4 x = mk(e1.y * e2.z - e1.z * e2.y, e1.z * e2.x - e1.x * e2.z, e1.x * e2.y - e1.y * e2.x);
        const float A = 0.5f * sqrtf(vdot(x, x));
        const float4 p1 = sc.tplane[2 * g + 1];
        const float4 m0 = sc.mats[2 * __float_as_uint(p1.w)];
        float w = A * ((m0.x + m0.y) + m0.z);
        if (!(w > 0.f) || !(w <= FLT_MAX)) w = 0.f;  // not > 0 (a NaN too) or not finite
        float4* r = lamp + (size_t)RTMI_EMISSIVE_REC * k;
        r[0] = make_float4(c0.x, c0.y, c0.z, A);
        r[1] = make_float4(e1.x, e1.y, e1.z, w);
        r[2] = make_float4(e2.x, e2.y, e2.z, 0.f);
        r[3] = make_float4(p1.x, p1.y, p1.z, 0.f);
        r[4] = make_float4(m0.x, m0.y, m0.z, 0.f);
        b = __float_as_uint(w);
    }
    for (int o = 32; o > 0; o >>= 1) b = max(b, (uint32_t)__shfl_xor((int)b, o));
    if ((threadIdx.x & 63u) == 0u) s_max[threadIdx.x >> 6] = b;
    __syncthreads();
    if (threadIdx.x == 0) atomicMax(wmax_bits, max(max(s_max[0], s_max[1]), max(s_max[2], s_max[3])));
}

// q and the inclusive prefix sums: ONE block, 256 lamps at a time: a cross-lane scan in every wave, a scan of the four wave totals
// through LDS, a running carry from tile to tile.  total[0] = the sum of q.  (k_envq_rows' quantisation.)
__global__ void __launch_bounds__(256) k_emq_scan(const float4* __restrict__ lamp, uint32_t n, const uint32_t* __restrict__ wmax_bits,
                                                  uint32_t* __restrict__ q, unsigned long long* __restrict__ cum,
                                                  unsigned long long* __restrict__ total) {
    __shared__ unsigned long long s_tot[4];
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const float wmax = __uint_as_float(*wmax_bits);
    const float scale = RTMI_ENVQ_SCALE / wmax;
    unsigned long long carry = 0ull;
    for (uint32_t k0 = 0; k0 < n; k0 += 256u) {  // (n is the same in every thread: whole blocks stay converged for the barriers)
        const uint32_t k = k0 + threadIdx.x;
        uint32_t qq = 0u;
        if (k < n) {
            qq = 1u;
            if (wmax != 0.f) {
                float s = lamp[(size_t)RTMI_EMISSIVE_REC * k + 1].w * scale;
                s = !(s >= 0.f) ? 0.f : (s > RTMI_ENVQ_SCALE ? RTMI_ENVQ_SCALE : s);
                qq = 1u + (uint32_t)s;
            }
        }
        unsigned long long inc = qq;  // inclusive scan over the wave's 64 lamps
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned long long up = __shfl_up(inc, o);
            if ((int)lane >= o) inc += up;
        }
        if (lane == 63u) s_tot[wv] = inc;
        __syncthreads();
        unsigned long long off = carry;
        for (uint32_t t = 0; t < wv; t++) off += s_tot[t];
        if (k < n) { q[k] = qq; cum[k] = off + inc; }
        carry += ((s_tot[0] + s_tot[1]) + s_tot[2]) + s_tot[3];
        __syncthreads();  // s_tot is rewritten by the next tile
    }
    if (threadIdx.x == 0) total[0] = carry;
}

// pe'(x2): the density per solid angle, seen from a ray's origin, of the point where the ray along `dir` meets lamp e (1-based), x2
// the squared distance the caller measures it by (t * t of a hit record: pe'; |y - point|^2 of a drawn point: pe_true)
__device__ inline float em_pdf(const EmTab& em, uint32_t e, float x2, V4 dir) {
    const float4* __restrict__ r = em.lamp + (size_t)RTMI_EMISSIVE_REC * (e - 1u);
    const float4 n4 = r[3];
    const float ndot = fabsf(vdot(mk(n4.x, n4.y, n4.z), dir));
    const float sel = (float)em.q[e - 1u] / (float)em.total;
    return ((sel / r[0].w) * x2) / ndot;
}

// One thread per entry of path queue `pass`; the compaction is k_lit_rays' (ballot + popcount per wave, ONE atomic per block on
// sctrl->count[pass + 1]).  lw[q] = (pb, d2, the lamp's number e, 0) of shadow queue entry q.
__global__ void __launch_bounds__(256) k_emissive_rays(DScene sc, DView v, uint64_t seed, uint32_t pix0, int pass, EmTab em,
                                                       const float4* __restrict__ qo, const float4* __restrict__ qd,
                                                       const uint32_t* __restrict__ qpath, const uint32_t* __restrict__ hit_tf,
                                                       const float* __restrict__ hit_t, const DCtrl* __restrict__ ctrl,
                                                       float4* __restrict__ lq_o, float4* __restrict__ lq_d, float4* __restrict__ lw,
                                                       uint32_t* __restrict__ slot, DCtrl* __restrict__ sctrl) {
    __shared__ uint32_t s_cnt[4], s_base;
    const uint32_t count = ctrl->count[pass];
    const uint32_t stride = gridDim.x * blockDim.x;
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint32_t bound = (count + 255u) & ~255u;  // whole blocks stay converged for the ballots and the barriers
    // (launched for the passes whose Matte hits bounce, maxdepth - pass - 1 != 0: an exhausted level gets no sample)
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < bound; i += stride) {
        bool live = false;
        V4 o{}, omega{};
        float4 rec = make_float4(0.f, 0.f, 0.f, 0.f);
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
                    rng_block(seed, row * v.width + col, sample, RTMI_EMISSIVE_BLOCK | (uint32_t)pass, w);
                    // the lamp: the first k with cum[k] > T.  T differs from lane to lane, so every probe is one vector load per
                    // wave (no chain of scalar loads), and the chain is log2(n) probes long: 10 for a thousand lamps.
                    const unsigned long long T = __umul64hi(((unsigned long long)w[0] << 32) | w[1], em.total);
                    uint32_t lo = 0u, hi = em.n - 1u;
                    while (lo < hi) {
                        const uint32_t mid = (lo + hi) >> 1;
                        if (em.cum[mid] > T) hi = mid; else lo = mid + 1u;
                    }
                    const uint32_t e = lo + 1u;
                    const float4* __restrict__ r = em.lamp + (size_t)RTMI_EMISSIVE_REC * lo;
                    const float4 r0 = r[0], r1 = r[1], r2 = r[2], r3 = r[3], r4 = r[4];
                    float a = u32_to_unit_f32(w[2]), b = u32_to_unit_f32(w[3]);
                    if (a + b > 1.f) { a = 1.f - a; b = 1.f - b; }  // the fold of the unit square onto the triangle
                    const V4 y = vadd(vadd(mk(r0.x, r0.y, r0.z), vmul(mk(r1.x, r1.y, r1.z), a)), vmul(mk(r2.x, r2.y, r2.z), b));
                    const V4 dv = vsub(y, point);
                    const float d2 = vdot(dv, dv);
                    omega = vunit(dv);
                    const float c = vdot(n, omega);
                    const V4 s = vsub(vmul(omega, 2.f * c), n);  // the random_vec whose bounce is omega
                    o = vadd(point, vmul(s, 0.001f));            // ... and where that bounce ray starts: the same visibility
                    const float ndot = fabsf(vdot(mk(r3.x, r3.y, r3.z), omega));
                    live = c > 0.f && ndot > 0.f && (r4.x != 0.f || r4.y != 0.f || r4.z != 0.f);
                    // (the shading recognises the lamp's triangle in the shadow ray's hit record by lampidx[tri] == e)
                    rec = make_float4(bounce_pdf(n, omega, s), d2, __uint_as_float(e), 0.f);
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
            store_stream(&lw[q], rec);
            store_stream(&slot[i], q);
        } else if (i < count) {
            store_stream(&slot[i], RTMI_SHADOW_NONE);
        }
        __syncthreads();  // s_cnt / s_base are rewritten by the next iteration
    }
}

// shade_hit_lit's arm for ONE traced ray of an emissive path: the same rays, stack and return value.  `direct` is the level's
// sampled light (radiance * (pb / pe_true) * wB where the candidate's first hit was its lamp, else 0).  wbuf[path] holds pb of the
// path's last bounce (RTMI_EMISSIVE_NO_SAMPLE for a Reflective one), read from pass 1 on where the path ends on a lamp.
template <bool ENV>
__device__ inline bool shade_hit_emissive(const DScene& sc, const EnvTab& env, const EmTab& em, uint32_t maxdepth, uint64_t seed, uint32_t npaths,
                                          uint32_t path, uint32_t pixel, uint32_t sample, uint32_t pass, uint32_t tf, float t, V4 ro, V4 rd,
                                          V4 direct, uint16_t* __restrict__ mstack, float4* __restrict__ dstack, float* __restrict__ wbuf,
                                          float4* __restrict__ scol, RayV& nr) {
    const uint32_t tri = tf & 0x3FFFFFFFu, face = tf >> 30;
    const V4 black = mk(0.f / 255.f, 0.f / 255.f, 0.f / 255.f);
    V4 c;
    uint32_t npushed = pass;
    if (tri == 0) {
        if (ENV) c = env_lookup(env, rd);
        else c = mk(128.f / 255.f, 180.f / 255.f, 255.f / 255.f);  // raytrace.rs:1264
    } else if (face & 2u) {
        c = black;  // edge faces are Solid black, raytrace.rs:452-457
    } else {
        const float4 p1 = sc.tplane[2 * tri + 1];  // triangles only: the caller refuses analytic spheres
        const uint32_t mat = __float_as_uint(p1.w);
        const float4 m0 = sc.mats[2 * mat], m1 = sc.mats[2 * mat + 1];
        const uint32_t kind = __float_as_uint(m1.y);
        if (kind == RTMI_SOLID) {
            c = mk(m0.x, m0.y, m0.z);
            const uint32_t e = em.lampidx[tri];
            if (e != 0u && pass != 0u) {  // strategy A: the bounce's own chance against the sample's
                const float pbp = wbuf[path];
                if (pbp >= 0.f) {
                    const float pe = em_pdf(em, e, t * t, rd);
                    c = vmul(c, pbp / (pbp + pe));
                }
            }
        } else {
            mstack[(size_t)pass * npaths + path] = (uint16_t)mat;
            npushed = pass + 1;
            c = black;  // project_ray at depth 0, raytrace.rs:1261-1263
            if (maxdepth - pass - 1u != 0u) {
                const V4 point = vadd(vmul(rd, t), ro);  // Ray::at, raytrace.rs:227-229
                V4 norm = mk(p1.x, p1.y, p1.z);
                if (face & 1u) norm = vmul(norm, -1.f);  // raytrace.rs:441-449
                const V4 rv = random_vec(seed, pixel, sample, pass + 1u);
                float wb = RTMI_EMISSIVE_NO_SAMPLE;
                if (kind == RTMI_MATTE) {
                    nr = make_ray(vadd(point, vmul(rv, 0.001f)), vadd(norm, rv));  // lambertian_ray, :292-297
                    wb = bounce_pdf(norm, nr.dir, rv);
                } else {
                    const float ddot = fabsf(vdot(rd, norm));  // reflect_ray, :278-290
                    const V4 dir_p = vmul(norm, ddot);
                    const V4 dir_o = vadd(rd, dir_p);
                    const V4 reflect = vadd(dir_p, dir_o);
                    const V4 rvf = vmul(rv, m1.x);
                    const V4 reflect_dir = vunit(vadd(reflect, rvf));
                    nr = make_ray(vadd(point, vmul(reflect_dir, 0.001f)), vunit(vadd(reflect, rvf)));
                    direct = V4{0.f, 0.f, 0.f, 0.f};
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

// k_shade_envlight's loop with the shadow ray's own hit record for its occlusion byte: the candidate counts when its first hit is
// the lamp it was drawn on, on a non-edge face
template <bool ENV>
__global__ void __launch_bounds__(256) k_shade_emissive(DScene sc, DView v, uint64_t seed, uint32_t pix0, uint32_t npaths, int pass, EnvTab env,
                                                        EmTab em, const float4* __restrict__ qo, const float4* __restrict__ qd,
                                                        const uint32_t* __restrict__ qpath, const uint32_t* __restrict__ hit_tf,
                                                        const float* __restrict__ hit_t, const uint32_t* __restrict__ slot,
                                                        const float4* __restrict__ lq_d, const float4* __restrict__ lw,
                                                        const uint32_t* __restrict__ shit_tf, const float* __restrict__ shit_t,
                                                        float4* __restrict__ qo_n, float4* __restrict__ qd_n, uint32_t* __restrict__ qpath_n,
                                                        uint16_t* __restrict__ mstack, float4* __restrict__ dstack, float* __restrict__ wbuf,
                                                        float4* __restrict__ scol, DCtrl* __restrict__ ctrl) {
    __shared__ uint32_t s_cnt[4], s_base;
    const uint32_t count = min(ctrl->count[pass], npaths);
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
            const float4 o4 = qo[i], d4 = qd[i];  // (with ENV a miss looks the environment up in its ray's direction)
            V4 direct{0.f, 0.f, 0.f, 0.f};
            if ((tf & 0x3FFFFFFFu) != 0u && !((tf >> 30) & 2u)) {
                t = hit_t[i];
                // (the exhausted pass has no candidates: k_emissive_rays is not launched for it and the slots are stale)
                const uint32_t q = v.maxdepth - (uint32_t)pass - 1u != 0u ? slot[i] : RTMI_SHADOW_NONE;
                if (q != RTMI_SHADOW_NONE && q < npaths) {
                    const uint32_t stf = shit_tf[q], stri = stf & 0x3FFFFFFFu;
                    const float4 l4 = lw[q];
                    const uint32_t e = __float_as_uint(l4.z);
                    if (stri != 0u && !((stf >> 30) & 2u) && em.lampidx[stri] == e) {
                        const float st = shit_t[q];
                        const float4 w4 = lq_d[q];
                        const V4 omega{w4.x, w4.y, w4.z, w4.w};
                        const float pe = em_pdf(em, e, st * st, omega), pet = em_pdf(em, e, l4.y, omega);
                        const float wB = pe / (l4.x + pe);
                        const float4 r4 = em.lamp[(size_t)RTMI_EMISSIVE_REC * (e - 1u) + 4];
                        direct = vmul(mk(r4.x, r4.y, r4.z), (l4.x / pet) * wB);
                    }
                }
            }
            uint32_t prow, pcol, sample;
            path_pixel<Samp::PASS>(v, pix0, path, prow, pcol, sample, nullptr);
            push = shade_hit_emissive<ENV>(sc, env, em, v.maxdepth, seed, npaths, path, prow * v.width + pcol, sample, (uint32_t)pass, tf, t,
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
