// hybrid.hpp — the hybrid bounce pass (DESIGN.md 4.1 "Hybrid pass"): the BVH of bvh_fast.hpp PROPOSES each ray's closest hit,
// the reference's octree only has to CONFIRM it, and only rays whose confirmation fails are walked exactly.  Included by
// rtmi_device.hip between trace_oct.hpp and bvh_fast.hpp.
//
// For a ray that holds the sign certificate (ray_sign_certified, trace_oct.hpp) every triangle has a nonzero den and a finite
// t.  Let (t*, T*) be the closest hit over ALL triangles (Triangle::intersects, strict `<`): what k_hybrid_bvh computes.
//   * nothing passes              -> the octree walk scans a subset of the triangles and finds nothing either: a miss is final;
//   * every hit the octree walk can take has t >= t*, and so has every per-box best its skip rule (raytrace.rs:965) compares;
//   * a chain of present children root = B0 > B1 > ... > Bk = leaf, each of which collides (tmin < tmax, the SELECT step's
//     arithmetic) with tmin < t*, is entered box by box: children are visited in ascending tmin, a child is refused only when
//     tmin >= best, and every child at or before Bi in that order has tmin <= tmin(Bi) < t* <= best;
//   * if the leaf's list holds T*, the running best ends at t*; if no other triangle passes with a t that compares equal to
//     t* (the tie flag of k_hybrid_bvh), the triangle it holds is T*, and t bits, face bits and index are the BVH's: both
//     evaluate them with the same expressions.
// The chain is found by a guided descent along the hit point P* = d t* + o: at every inner box the octant of P*, that child's
// slab alone, at the leaf a comparison of indices.  No plane record is read.  Whatever fails -- a refused certificate, a tie,
// an absent child, a slab that does not collide or begins at or behind t*, a list without T* -- sends the ray to the pass's
// fallback list, which k_trace_oct_list (trace_oct.hpp) walks exactly.
//
// Launches of a pass (launch_trace, rtmi_device.hip): k_hybrid_bvh, k_oct_verify, k_trace_oct_list.
// DCtrl::hyb (always counted: a handful of atomics per wave): 0 rays offered, 1 certificate refusals, 2 BVH misses, 3 ties,
// 4..6 descents failed at an absent child / a child that does not collide / a child with tmin >= t*, 7 lists without T*,
// 8 rays on fallback lists, 9 violations (a counting launch's referee, k_hybrid_referee: a confirmed record that differs from
// the exact walk's in any bit; must stay 0), 10 descents that left the tree's arrays or depth (must stay 0), 11 confirmed hits.
#pragma once

namespace rtmi {

// The band of the certificate k_hybrid_bvh evaluates: only finiteness is needed (RTMI_DEVDEFS=-DHYB_KAPPA=CERT_KAPPA builds the
// comparison of DESIGN.md 4.1)
#ifndef HYB_KAPPA
#define HYB_KAPPA CERT_KAPPA_PRIMARY
#endif
// The origin bound.  Triangle::intersects decides on the ROUNDED point P = fl(d t + o), the BVH's slab test on the line itself:
// a component of P is off the line by at most 2^-24 (|d_k t| + |P_k|) <= 2^-24 (|o_k| + 2 |P_k|), and a slab end (lo - o) * inv
// carries 2^-23 (|o_k| + |lo_k|) of rounding in space -- together below 2^-22 (2 |o|_1 + |P|_1).  Every clip box (bvh_clip_box) is
// wider than the region its record accepts by eps_i >= 2e-5 (|c_i|_1 + r_i + 1), and an accepted P has |P|_1 <= 2 (|c_i|_1 + r_i).
// With |o|_1 <= 16 (m + 1), m = the smallest |c_i|_1 + r_i of the scene, the line passes every accepted P within
// 2^-22 (32 (m + 1) + 2 (|c_i|_1 + r_i)) <= 0.41 eps_i: inside the box with more than half the margin left for what it covered
// before (the rounding of the edge tests), and entering it before t.  A ray with a farther origin is refused like one without the
// certificate.  (The ray-independent margin is what the block cull's boxes grow by K |o|_1 for, trace_oct.hpp.)
#define HYB_OMAX_K 16.f
inline float hybrid_origin_max(float m) { return HYB_OMAX_K * (m + 1.f); }
__host__ __device__ inline bool hybrid_origin_ok(float4 o, float omax) {  // (a NaN gives false)
    return (fabsf(o.x) + fabsf(o.y)) + fabsf(o.z) <= omax;
}

#define HYB_PENDING 0xFFFFFFFFu  // hit_tf of a ray that is on the fallback list (no triangle: indices are < 2^26)
enum : int { HV_OK = 0, HV_ABSENT = 1, HV_NOCOLLIDE = 2, HV_TMIN = 3, HV_NOTRI = 4, HV_BOUNDS = 5 };

// collides() of the child in octant `oct` of the inner box with centre (cx, cy, cz) whose children have half edge hc, as the
// SELECT step of oct_walk writes it (trace_oct.hpp: the child's centre is the builder's cx + (+-hc), the slab pair is (a - b,
// a + b) with b = |inv_dir| hc) for a ray without a zero direction component: bit for bit BoundingBox::collides
// (raytrace.rs:860-907) of that child.  ix, iy, iz = 1 / d as make_rayk keeps them.
__host__ __device__ inline bool hybrid_child_slab(float cx, float cy, float cz, float hc, uint32_t oct, float ox, float oy, float oz,
                                                  float ix, float iy, float iz, float& tmin_o) {
    const float px = (oct & 1u) ? cx + hc : cx + (-hc);
    const float py = (oct & 2u) ? cy + hc : cy + (-hc);
    const float pz = (oct & 4u) ? cz + hc : cz + (-hc);
    const float bx = fabsf(ix) * hc, by = fabsf(iy) * hc, bz = fabsf(iz) * hc;
    const float ax = (px - ox) * ix, ay = (py - oy) * iy, az = (pz - oz) * iz;
    const float nx = ax - bx, ny = ay - by, nz = az - bz;
    const float fx = ax + bx, fy = ay + by, fz = az + bz;
    // (fmaxf / fminf as the reference's f32::max / f32::min: a NaN operand is ignored)
    const float tmin = fmaxf(fmaxf(nx, ny), nz), tmax = fminf(fminf(fx, fy), fz);
    tmin_o = tmin;
    return tmin < tmax;
}

// The guided descent and the list scan for the proposed hit (t, tri) of ray (o, d); HV_OK: the octree walk returns that hit.
// The caller has made sure that the ray holds the certificate.
__host__ __device__ inline int hybrid_verify(const uint4* __restrict__ fnodes, const uint4* __restrict__ oblocks,
                                             const uint32_t* __restrict__ wlinks, uint32_t nfn, uint32_t noblocks, uint32_t olevels,
                                             float root_half, float4 o, float4 d, float t, uint32_t tri) {
    const float ix = 1.f / d.x, iy = 1.f / d.y, iz = 1.f / d.z;  // make_rayk
    const float px = d.x * t + o.x, py = d.y * t + o.y, pz = d.z * t + o.z;
    uint32_t fnode = 0u, lblock = 0u;
    uint32_t lvl = 0u;
    for (;;) {
        if (lvl >= olevels || fnode >= nfn) return HV_BOUNDS;
        const uint4 q0 = fnodes[2u * fnode], q1 = fnodes[2u * fnode + 1u];
#ifdef __HIP_DEVICE_COMPILE__
        const float cx = __uint_as_float(q0.x), cy = __uint_as_float(q0.y), cz = __uint_as_float(q0.z);
#else
        float cx, cy, cz;
        memcpy(&cx, &q0.x, 4); memcpy(&cy, &q0.y, 4); memcpy(&cz, &q0.z, 4);
#endif
        const float hc = ldexpf(root_half, -(int)(lvl + 1u));  // half edge of the children (depth lvl + 1), as the SELECT step
        const uint32_t oct = (px > cx ? 1u : 0u) | (py > cy ? 2u : 0u) | (pz > cz ? 4u : 0u);
        const uint32_t bit = 1u << oct;
        if (!(q0.w & bit)) return HV_ABSENT;
        float tmin;
        if (!hybrid_child_slab(cx, cy, cz, hc, oct, o.x, o.y, o.z, ix, iy, iz, tmin)) return HV_NOCOLLIDE;
        if (!(tmin < t)) return HV_TMIN;
        const uint32_t leafmask = (q0.w >> 8) & 0xFFu;
        if (leafmask & bit) {
            if (q0.w & FN_WIDE) lblock = wlinks[(size_t)q1.y * 8u + oct];
            else lblock = q1.y + (((oct < 4u ? q1.z : q1.w) >> ((oct & 3u) * 8u)) & 0xFFu);
            break;
        }
        fnode = q1.x + (uint32_t)__builtin_popcount((q0.w & ~leafmask & 0xFFu) & (bit - 1u));
        lvl++;
    }
    // the leaf's list: it ends at the first index 0 or behind a full block whose fourth index has bit 31 set
    for (uint32_t b = lblock; b < noblocks; b++) {
        const uint4 blk = oblocks[b];
        if ((blk.x == tri) | (blk.y == tri) | (blk.z == tri) | ((blk.w & 0x7FFFFFFFu) == tri)) return HV_OK;  // (tri != 0)
        if (blk.w == 0u || (blk.w >> 31)) return HV_NOTRI;
    }
    return HV_BOUNDS;
}

// The tie rule of k_hybrid_bvh for one passing triangle (t, tri) against the lane's best (bt, btri; btri == 0: none yet):
// equal times (+0 == -0) of different triangles set the flag, a strictly smaller time clears it.  Returns the new flag.
__host__ __device__ inline bool hybrid_tie_flag(bool flag, float t, uint32_t tri, float bt, uint32_t btri) {
    const bool tie = (btri != 0u) & (t == bt) & (tri != btri);
    return (t < bt) ? false : (flag | tie);
}

#ifdef __HIPCC__
// Wave-compacted append of queue index `idx` to the fallback list of `pass` by the lanes with p (ballot, prefix sum, one
// atomic; every lane of the wave calls it).  A ray is appended at most once, so the list never outgrows the queue.
// Returns how many lanes appended.
__device__ inline uint32_t hybrid_append(bool p, uint32_t idx, uint32_t* __restrict__ fb, DCtrl* __restrict__ ctrl, int pass, int lane) {
    const unsigned long long mask = __ballot(p);
    if (!mask) return 0u;
    uint32_t qb = 0;
    if (lane == 0) qb = atomicAdd(&ctrl->fbcount[pass], (uint32_t)__popcll(mask));
    qb = (uint32_t)__builtin_amdgcn_readfirstlane((int)qb);
    if (p) fb[qb + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull))] = idx;
    return (uint32_t)__popcll(mask);
}

// One ray per lane over the queue of `pass`: a ray that k_hybrid_bvh left a hit for is confirmed against the octree or goes to
// the fallback list with HYB_PENDING in its record.  Misses and rays already on the list are left alone.
__global__ void __launch_bounds__(256) k_oct_verify(DScene sc, uint32_t nfn, const float4* __restrict__ qo, const float4* __restrict__ qd,
                                                    DCtrl* __restrict__ ctrl, int pass, uint32_t* __restrict__ hit_tf,
                                                    const float* __restrict__ hit_t, uint32_t* __restrict__ fb) {
    const uint32_t count = ctrl->count[pass];
    const int lane = threadIdx.x & 63;
    uint32_t nfail[5] = {0u, 0u, 0u, 0u, 0u}, nok = 0u, nfb = 0u;  // (wave-uniform)
    // (the trip count is the same for every lane of a wave: the appends below are wave operations)
    for (uint32_t base = blockIdx.x * blockDim.x + (threadIdx.x & ~63u); base < count; base += gridDim.x * blockDim.x) {
        const uint32_t i = base + (uint32_t)lane;
        int rc = HV_OK;
        bool hit = false;
        if (i < count) {
            const uint32_t tf = hit_tf[i];
            hit = tf != 0u && tf != HYB_PENDING;
            if (hit)
                rc = hybrid_verify(sc.fnodes, sc.oblocks, sc.wlinks, nfn, sc.noblocks, sc.olevels, sc.root_half, qo[i], qd[i], hit_t[i],
                                   tf & 0x3FFFFFFFu);
        }
        const bool bad = hit && rc != HV_OK;
        if (bad) hit_tf[i] = HYB_PENDING;
        nfb += hybrid_append(bad, i, fb, ctrl, pass, lane);
        nok += (uint32_t)__popcll(__ballot(hit && rc == HV_OK));
#pragma unroll
        for (int k = 0; k < 5; k++) nfail[k] += (uint32_t)__popcll(__ballot(bad && rc == k + 1));
    }
    if (lane == 0) {
        if (nfail[0]) atomicAdd(&ctrl->hyb[4], (unsigned long long)nfail[0]);
        if (nfail[1]) atomicAdd(&ctrl->hyb[5], (unsigned long long)nfail[1]);
        if (nfail[2]) atomicAdd(&ctrl->hyb[6], (unsigned long long)nfail[2]);
        if (nfail[3]) atomicAdd(&ctrl->hyb[7], (unsigned long long)nfail[3]);
        if (nfail[4]) atomicAdd(&ctrl->hyb[10], (unsigned long long)nfail[4]);
        if (nfb) atomicAdd(&ctrl->hyb[8], (unsigned long long)nfb);
        if (nok) atomicAdd(&ctrl->hyb[11], (unsigned long long)nok);
    }
}

// The referee of a counting launch: the exact walk's records (xtf, xt) against the hybrid's scratch records (htf, ht) for every
// ray the hybrid did not send to the fallback list.
__global__ void __launch_bounds__(256) k_hybrid_referee(DCtrl* __restrict__ ctrl, int pass, const uint32_t* __restrict__ xtf,
                                                        const float* __restrict__ xt, const uint32_t* __restrict__ htf,
                                                        const float* __restrict__ ht) {
    const uint32_t count = ctrl->count[pass];
    uint32_t bad = 0u;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < count; i += gridDim.x * blockDim.x) {
        if (htf[i] == HYB_PENDING) continue;
        bad += (htf[i] != xtf[i] || __float_as_uint(ht[i]) != __float_as_uint(xt[i])) ? 1u : 0u;
    }
    if (bad) atomicAdd(&ctrl->hyb[9], (unsigned long long)bad);
}
#endif

}  // namespace rtmi
