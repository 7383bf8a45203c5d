// lit_rays_kernel.hpp -- the text of lit.hpp's candidate kernel, included there once per sampling mode (no include guard) with
//   RTMI_LIT_KERNEL      the kernel's name
//   RTMI_LIT_KEYS_PARAM  the mode's own last parameter (empty, or `, const uint32_t* __restrict__ keys`)
//   RTMI_LIT_RAYS_KEY    the statements that set `pixel` and `sample`, the RNG key of the path of queue entry i
// so that every mode's kernel is compiled from the same lines and k_lit_rays keeps the machine code it had (a shared device
// function does not: the grid built-ins and the argument loads are scheduled differently around an inlined body).
// With RTMI_LIT_SURFACES_KERNEL defined (the kernels of scenes with surface features, lit.hpp; RTMI_LIT_KEYS_PARAM then ends with
// `, SmoothTab sm, TexTab tex, NmapTab nm`) the candidate has two normals: ns, the hit's shading normal, gives c; n, the geometric
// one, gives the origin's offset and the second liveness test.  Without it the three hooks below expand to the text the kernel had.
#ifdef RTMI_LIT_SURFACES_KERNEL
#define RTMI_LIT_SHADING_NORMAL_DECL V4 ns{};
#define RTMI_LIT_SHADING_NORMAL ns = lit_shading_normal(sm, tex, nm, tri, tf >> 30, point, V4{d4.x, d4.y, d4.z, d4.w}, n);
#define RTMI_LIT_N ns
#define RTMI_LIT_LIVE c > 0.f && vdot(n, dir[l]) > 0.f
#else
#define RTMI_LIT_SHADING_NORMAL_DECL
#define RTMI_LIT_SHADING_NORMAL
#define RTMI_LIT_N n
#define RTMI_LIT_LIVE c > 0.f
#endif
__global__ void __launch_bounds__(256) RTMI_LIT_KERNEL(DScene sc, DView v, uint64_t seed, uint32_t pix0, uint32_t npaths, int pass, LitArgs la,
                                                  const float4* __restrict__ qo, const float4* __restrict__ qd,
                                                  const uint32_t* __restrict__ qpath, const uint32_t* __restrict__ hit_tf,
                                                  const float* __restrict__ hit_t, const DCtrl* __restrict__ ctrl,
                                                  float4* __restrict__ lq_o, float4* __restrict__ lq_d, float* __restrict__ lq_tmax,
                                                  float4* __restrict__ lw, uint32_t* __restrict__ slot, DCtrl* __restrict__ sctrl RTMI_LIT_KEYS_PARAM) {
    __shared__ uint32_t s_cnt[4], s_base;
    const uint32_t count = min(ctrl->count[pass], npaths);
    const uint32_t stride = gridDim.x * blockDim.x;
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint32_t bound = (count + 255u) & ~255u;  // whole blocks stay converged for the ballots and the barriers
    const uint32_t nl = min(la.nlights, (uint32_t)RTMI_LIT_LIGHTS);
    // (launched for the passes whose Matte hits bounce, maxdepth - pass - 1 != 0: an exhausted level gets no sample)
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < bound; i += stride) {
        bool cand = false;
        V4 point{}, n{};
        uint32_t pixel = 0, sample = 0;
        RTMI_LIT_SHADING_NORMAL_DECL
        if (i < count) {
            const uint32_t tf = hit_tf[i], tri = tf & 0x3FFFFFFFu;
            if (tri != 0u && !((tf >> 30) & 2u)) {
                const float4 p1 = sc.tplane[2 * tri + 1];
                const float4 m1 = sc.mats[2 * __float_as_uint(p1.w) + 1];
                if (__float_as_uint(m1.y) == RTMI_MATTE) {
                    cand = true;
                    const float t = hit_t[i];
                    const float4 o4 = qo[i], d4 = qd[i];
                    point = vadd(vmul(V4{d4.x, d4.y, d4.z, d4.w}, t), V4{o4.x, o4.y, o4.z, o4.w});
                    n = mk(p1.x, p1.y, p1.z);
                    if ((tf >> 30) & 1u) n = vmul(n, -1.f);
                    RTMI_LIT_RAYS_KEY
                    RTMI_LIT_SHADING_NORMAL
                }
            }
        }
        bool live[RTMI_LIT_LIGHTS];
        V4 o[RTMI_LIT_LIGHTS], dir[RTMI_LIT_LIGHTS];
        float r[RTMI_LIT_LIGHTS], g[RTMI_LIT_LIGHTS];
        uint32_t place[RTMI_LIT_LIGHTS];  // the lane's place among the wave's live candidates
        uint32_t wtotal = 0;
        const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
        for (uint32_t l = 0; l < RTMI_LIT_LIGHTS; l++) {
            live[l] = false;
            o[l] = V4{}; dir[l] = V4{};
            r[l] = 0.f; g[l] = 0.f;
            place[l] = 0;
            if (l < nl) {
                if (cand) {
                    const LitLight& L = la.li[l];
                    uint32_t w[4];
                    rng_block(seed, pixel, sample, 0xC0000000u | (l << 16) | (uint32_t)pass, w);
                    const V4 adj{L.orig.x + u32_to_unit_f32(w[0]) * L.len2, L.orig.y + u32_to_unit_f32(w[1]) * L.len2,
                                 L.orig.z + u32_to_unit_f32(w[2]) * L.len2, 0.f};
                    const V4 vv = vsub(adj, point);
                    const float d2 = vdot(vv, vv);
                    r[l] = sqrtf(d2);
                    dir[l] = vmul(vv, 1.f / r[l]);
                    o[l] = vadd(point, vmul(n, L.bias * (u32_to_unit_f32(w[3]) + 1.f)));
                    const float c = vdot(RTMI_LIT_N, dir[l]);
                    live[l] = RTMI_LIT_LIVE;  // false for the light behind the surface, for a NaN and for the light at the point
                    g[l] = la.inverse_square ? c / d2 : c;
                }
                const unsigned long long mask = __ballot(live[l]);
                place[l] = wtotal + (uint32_t)__popcll(mask & below);
                wtotal += (uint32_t)__popcll(mask);
            }
        }
        if (lane == 0) s_cnt[wv] = wtotal;
        __syncthreads();
        if (threadIdx.x == 0) {
            const uint32_t total = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
            s_base = total ? atomicAdd(&sctrl->count[pass + 1], total) : 0u;
        }
        __syncthreads();
        uint32_t base = s_base;
        for (uint32_t k = 0; k < wv; k++) base += s_cnt[k];
#pragma unroll
        for (uint32_t l = 0; l < RTMI_LIT_LIGHTS; l++) {
            if (l < nl) {
                if (live[l]) {
                    const LitLight& L = la.li[l];
                    const uint32_t q = base + place[l];
                    store_stream(&lq_o[q], make_float4(o[l].x, o[l].y, o[l].z, o[l].w));
                    store_stream(&lq_d[q], make_float4(dir[l].x, dir[l].y, dir[l].z, dir[l].w));
                    store_stream(&lq_tmax[q], L.unbounded ? INFINITY : r[l]);
                    store_stream(&lw[q], make_float4(L.col[0] * g[l], L.col[1] * g[l], L.col[2] * g[l], 0.f));
                    store_stream(&slot[(size_t)l * npaths + i], q);
                } else if (i < count) {
                    store_stream(&slot[(size_t)l * npaths + i], RTMI_SHADOW_NONE);
                }
            }
        }
        __syncthreads();  // s_cnt / s_base are rewritten by the next iteration
    }
}
#undef RTMI_LIT_SHADING_NORMAL_DECL
#undef RTMI_LIT_SHADING_NORMAL
#undef RTMI_LIT_N
#undef RTMI_LIT_LIVE
