// rtmi_device.hip — HIP kernels (gfx950) and the C ABI of include/rtmi.h.
//
// Pipeline for one batch of N = pixels*spp paths ("wavefront" formulation of
// the reference's recursive project_ray, raytrace_lib/src/raytrace.rs:1256-1295):
//
//   k_gen     pixel_ray() for every (pixel, sample)        raytrace.rs:1374-1394
//   for pass k = 0 .. maxdepth-1 (remaining depth = maxdepth-k):
//     k_trace closest hit for every queued ray              raytrace.rs:909-1050, 400-439
//     k_shade color_ray(): terminal colour, or push the surface and emit
//             the bounce ray into the next queue, compacted with wave
//             ballot + prefix sum                           raytrace.rs:1199-1254, 278-301
//   k_accum   per pixel: ordered sum over samples * (1/spp) raytrace.rs:1414-1426
//
// The recursion `mix(c_1, mix(c_2, ...))` is evaluated inside-out when a path
// terminates (fold over the per-path surface stack), which is bit-identical to
// the nested calls; see DESIGN.md.
//
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off (strict IEEE f32:
// correctly rounded / and sqrtf are hipcc defaults, contraction is not).
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>  // types and prototypes only: the library is dlopen'ed when RTMI_FRAME_RCCL is asked for
#include <dlfcn.h>

#include <algorithm>
#include <array>
#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <tuple>
#include <unordered_map>
#include <vector>

#include "../../../include/rtmi.h"
#include "vec4.hpp"

// layouts the language bindings mirror (rust_raytrace_amd/_ffi.py, INTEGRATION.md ffi.rs; tests/test_host_cpu.py)
static_assert(sizeof(rtmi_stats_t) == 128 && sizeof(rtmi_tuning_t) == 48 && sizeof(rtmi_tile_t) == 16 && sizeof(rtmi_box_t) == 32 &&
              sizeof(rtmi_triangle_t) == 104 && sizeof(rtmi_viewport_t) == 64 && sizeof(rtmi_sphere_t) == 40 &&
              sizeof(rtmi_ray_record_t) == 72, "ABI struct layout changed");
static_assert(sizeof(rtmi_adaptive_t) == 32 && offsetof(rtmi_adaptive_t, samples) == 24, "ABI struct layout changed");
static_assert(sizeof(rtmi_denoise_t) == 24 && offsetof(rtmi_denoise_t, sigma_color) == 8, "ABI struct layout changed");
static_assert(sizeof(rtmi_ao_t) == 16 && offsetof(rtmi_ao_t, radius) == 8, "ABI struct layout changed");
static_assert(sizeof(rtmi_camera_t) == 16 && offsetof(rtmi_camera_t, lens_radius) == 8 && sizeof(rtmi_camera_out_t) == 3 * sizeof(void*), "ABI struct layout changed");
static_assert(sizeof(rtmi_bake_t) == 24 && offsetof(rtmi_bake_t, pixel0) == 12 && offsetof(rtmi_bake_t, bias) == 20 &&
              sizeof(rtmi_bake_out_t) == 4 * sizeof(void*) && offsetof(rtmi_bake_out_t, orig) == 2 * sizeof(void*), "ABI struct layout changed");
static_assert(sizeof(rtmi_light_t) == 28 && offsetof(rtmi_light_t, rays) == 16 && offsetof(rtmi_light_t, bias) == 24, "ABI struct layout changed");

namespace rtmi {

// ---------------------------------------------------------------- layout
// HBM-resident scene (see DESIGN.md "Data layout"):
//  nodes   : one 32-B record per BoundingBox, children of a box contiguous
//  refs    : u32 triangle indices of all leaves, leaf ranges contiguous
//  tplane  : 2 x float4 per triangle  (incenter.xyz, r2) (norm.xyz, material)
//  tedge   : 4 x float4 per triangle  (side_k.xyz, side_len_k) x3, (thr_k x3, 0)
//            thr_k = side_len_k * (1 - edge_thickness)      raytrace.rs:419
//  mats    : 2 x float4 per distinct surface (color.rgb, alpha) (scattering, kind, 0, 0)
struct DNode {
    float cx, cy, cz, half;
    uint32_t first, count, is_leaf, pad;
};

struct DScene {
    const DNode* nodes;
    const uint32_t* refs;
    const float4* tplane;
    const float4* tedge;
    const float4* mats;
    uint32_t nnodes, ntris, nmats, levels;
    // exact-octree form (trace_oct.hpp); null when the tree is not an exact octree
    const uint4* fnodes;
    const uint4* oblocks;
    const uint32_t* wlinks;  // 8 explicit first-block indices per FN_WIDE box
    // analytic spheres (a build-defined extension, rtmi_sphere_t): 2 x float4 each, (centre, radius) (surface id, 0, 0, 0)
    const float4* spheres;
    uint32_t nspheres;
    float root_half;
    uint32_t olevels;
    uint32_t noblocks;  // reference blocks in `oblocks`
    // packed block cull records, one uint4 per reference block (trace_oct.hpp, "Block cull"); null: the cull is off
    const uint4* ocull;
    // the sign certificate's direction table (trace_oct.hpp, ray_sign_certified); null exactly when ocull is
    const uint32_t* cert;
    // packed subtree cull records, one uint4 per `fnodes` record at the same index (trace_oct.hpp, "Node cull"); null: the
    // node cull is off (always when cert is)
    const uint4* fcull;
};
#define RTMI_FN_WIDE 0x10000u
// What build_ray_cert made: cells per face edge, distinct normals, list entries, the longest list, table bytes, seconds
struct CertStats {
    uint32_t g, normals;
    uint64_t entries;
    uint32_t longest;
    uint64_t bytes;
    double seconds;
};

#define RTMI_MAX_PASSES 32
#define RTMI_MAX_STREAMS 4  // interleaved sub-tiles of one tile, each on its own internal stream
#define RTMI_NHYB 12        // statistics of the hybrid passes (hybrid.hpp: what each entry counts)
#define RTMI_NDBG 52        // step statistics of the counting build (trace_oct.hpp: what each entry counts)
struct DCtrl {
    uint32_t count[RTMI_MAX_PASSES + 1];  // rays queued for pass k
    uint32_t head[RTMI_MAX_PASSES + 1];   // work-fetch cursor of pass k
    uint32_t xhead[RTMI_MAX_PASSES + 1][8];  // octree kernel: one cursor per XCD range of the queue
    // slow-path queue (rays with an exactly-zero direction component, trace_oct.hpp): entries pushed so far, and per
    // consumer launch k its range [slo[k], shi[k]) (k_slow_snapshot) and work-fetch cursor
    uint32_t scount;
    uint32_t slo[RTMI_MAX_PASSES + 1], shi[RTMI_MAX_PASSES + 1], shead[RTMI_MAX_PASSES + 1];
    unsigned long long rays;              // sum of count[] (the "Rays" statistic)
    unsigned long long counters[5];       // box_tests tri_tests full_tests nodes leaves
    unsigned long long dbg[RTMI_NDBG];    // step statistics of the counting build (tools/step_stats.py)
    // hybrid passes (hybrid.hpp): rays on the fallback list of pass k, the exact walk's cursors over it, the statistics
    uint32_t fbcount[RTMI_MAX_PASSES + 1];
    uint32_t fbhead[RTMI_MAX_PASSES + 1][8];
    unsigned long long hyb[RTMI_NHYB];
};

// The slow-path queue of one stream's batch.  A ray whose unit direction has an exactly-zero component skips that axis'
// slab in BoundingBox::collides (raytrace.rs:872, :882, :892: the origin is not checked against the slab), so it enters
// every box of the perpendicular plane: ~150 x the work of an ordinary ray (6 000 box + 36 000 triangle tests on the
// canonical scene), 14 ms for the one lane that traces it.  78 of the 268 M primary rays of config 3 are such rays (the
// two pixel rows and columns next to the camera axis, where `row + v_off` rounds to the axis), ~20 bounce rays per frame.
// Their work is nothing, their LATENCY is: a lane that meets one near the end of a launch holds the launch (and, in the
// primary pass, its whole wave) for up to 14 ms -- 10 % of a 1/8-frame tile.  Producers (k_path_primary, k_shade) put such
// rays here instead of the ordinary queue; k_path_slow traces their paths to the end on a side stream, one path per
// wave, concurrently with the following passes.  Same device functions, same image.
struct SlowQ {
    float4* o; float4* d; uint32_t* path; uint32_t* bounce;
    uint32_t cap;
};
#define RTMI_SLOW_CAP 16384u
__device__ inline bool has_zero_component(float x, float y, float z) { return (x == 0.f) | (y == 0.f) | (z == 0.f); }
// true when the ray was queued for the slow path (false: the queue is full, the caller keeps the ray)
__device__ inline bool slow_push(const SlowQ& q, DCtrl* ctrl, float4 o, float4 d, uint32_t path, uint32_t bounce) {
    const uint32_t slot = atomicAdd(&ctrl->scount, 1u);
    if (slot >= q.cap) return false;
    q.o[slot] = o; q.d[slot] = d; q.path[slot] = path; q.bounce[slot] = bounce;
    return true;
}
__global__ void k_slow_snapshot(DCtrl* ctrl, uint32_t k, uint32_t cap) {
    ctrl->slo[k] = k ? ctrl->shi[k - 1] : 0u;
    ctrl->shi[k] = min(ctrl->scount, cap);
}

// ---------------------------------------------------------------- ray for the hot loops
struct RayK {
    float ox, oy, oz, dx, dy, dz, ix, iy, iz;
    float ow, dw;  // lane 3 of orig / dir (normally +0)
    float qn, qd;  // lane-3 terms of norm.(incenter-orig) and norm.dir
};

__device__ inline RayK make_rayk(float4 o, float4 d) {
    RayK r;
    r.ox = o.x; r.oy = o.y; r.oz = o.z; r.ow = o.w;
    r.dx = d.x; r.dy = d.y; r.dz = d.z; r.dw = d.w;
    r.ix = 1.f / d.x; r.iy = 1.f / d.y; r.iz = 1.f / d.z;  // raytrace.rs:206-208
    r.qn = 0.f * (0.f - o.w);
    r.qd = 0.f * d.w;
    return r;
}

// BoundingBox::collides (raytrace.rs:860-907)
__device__ inline bool collides(float cx, float cy, float cz, float half, const RayK& r, float& tmin_o) {
    float tmin = -FLT_MAX, tmax = FLT_MAX;
    float a0 = (cx - r.ox) * r.ix, a1 = (cy - r.oy) * r.iy, a2 = (cz - r.oz) * r.iz;
    float b0 = r.ix * half, b1 = r.iy * half, b2 = r.iz * half;
    float t10 = a0 - b0, t20 = a0 + b0;
    float t11 = a1 - b1, t21 = a1 + b1;
    float t12 = a2 - b2, t22 = a2 + b2;
    if (r.dx != 0.f) {
        if (r.ix > 0.f) { tmin = t10; tmax = t20; } else { tmin = t20; tmax = t10; }
    }
    if (r.dy != 0.f) {
        if (r.iy > 0.f) { tmin = fmaxf(tmin, t11); tmax = fminf(tmax, t21); }
        else { tmin = fmaxf(tmin, t21); tmax = fminf(tmax, t11); }
    }
    if (r.dz != 0.f) {
        if (r.iz > 0.f) { tmin = fmaxf(tmin, t12); tmax = fminf(tmax, t22); }
        else { tmin = fmaxf(tmin, t22); tmax = fminf(tmax, t12); }
    }
    tmin_o = tmin;
    return tmin < tmax;
}

// Triangle::intersects (raytrace.rs:400-439).  Returns hit; face bits: 1 = back, 2 = edge.
template <bool COUNT>
__device__ inline bool tri_test(const DScene& sc, uint32_t tri, const RayK& r, float& t_o, uint32_t& face_o,
                                unsigned long long* cnt) {
    const float4 p0 = sc.tplane[2 * tri], p1 = sc.tplane[2 * tri + 1];
    float ax = p0.x - r.ox, ay = p0.y - r.oy, az = p0.z - r.oz;
    float num = (((0.f + p1.x * ax) + p1.y * ay) + p1.z * az) + r.qn;
    float den = (((0.f + p1.x * r.dx) + p1.y * r.dy) + p1.z * r.dz) + r.qd;
    float t = num / den;
    if (COUNT) cnt[1]++;
    if (t < 0.f) return false;
    float px = r.dx * t + r.ox, py = r.dy * t + r.oy, pz = r.dz * t + r.oz, pw = r.dw * t + r.ow;
    float ix = px - p0.x, iy = py - p0.y, iz = pz - p0.z;
    float l2 = ((ix * ix + iy * iy) + iz * iz) + pw * pw;
    if (l2 > p0.w) return false;
    if (COUNT) cnt[2]++;
    const float4 e0 = sc.tedge[4 * tri], e1 = sc.tedge[4 * tri + 1], e2 = sc.tedge[4 * tri + 2], e3 = sc.tedge[4 * tri + 3];
    float z = pw * 0.f;  // lane-3 product ip.w * side.w (side.w is +-0)
    float d0 = ((ix * e0.x + iy * e0.y) + iz * e0.z) + z;
    float d1 = ((ix * e1.x + iy * e1.y) + iz * e1.z) + z;
    float d2 = ((ix * e2.x + iy * e2.y) + iz * e2.z) + z;
    if (d0 > e0.w) return false;
    if (d1 > e1.w) return false;
    if (d2 > e2.w) return false;
    bool edge = (d0 > e3.x) | (d1 > e3.y) | (d2 > e3.z);
    t_o = t;
    face_o = (den > 0.f ? 1u : 0u) | (edge ? 2u : 0u);
    return true;
}

// ---------------------------------------------------------------- generic traversal (v1)
// Iterative form of BoundingBox::get_object_intersection_for_ray
// (raytrace.rs:909-1010).  One lane = one ray.  A frame is one inner box whose
// colliding children wait in sorted order:
//   w0 = index of its first child
//   w1 = order word: 3-bit child slots, next child in bits 0-2 | count << 24 |
//        has_hit << 28 | any_tmin_is_MAX << 29
//   w2 = t of the frame's best hit, w3 = triangle | face << 30
// Ancestors of the current frame live in LDS ([level][word][thread], so a
// lane always hits its own bank).  The children's tmin are not kept: the
// reference's skip rule `tmin < best_t` (raytrace.rs:965) is re-evaluated by
// running collides() again on the one child about to be visited, which
// returns the same float; since children are visited in ascending tmin and the
// best t never grows, the first skipped child ends the frame.
struct Frame { uint32_t first, w1; float t; uint32_t tri; };

#define F_COUNT(w) (((w) >> 24) & 15u)
#define F_HAS 0x10000000u
#define F_ANYMAX 0x20000000u

template <bool COUNT>
__device__ inline Frame expand(const DScene& sc, uint32_t first, uint32_t count, const RayK& r, unsigned long long* cnt) {
    float tm[8];
    bool anymax = false;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        tm[j] = INFINITY;
        if (j < (int)count) {
            const float4 g = *reinterpret_cast<const float4*>(&sc.nodes[first + j]);
            float tmin;
            if (COUNT) cnt[0]++;
            if (collides(g.x, g.y, g.z, g.w, r, tmin)) {
                tm[j] = tmin;
                anymax |= (tmin == FLT_MAX);
            }
        }
    }
    // stable ascending rank (insertion sort of raytrace.rs:941-947): child i
    // goes after every j < i with tm[j] <= tm[i] and every j > i with tm[j] < tm[i].
    uint32_t order = 0, nh = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        uint32_t rank = 0;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            if (j < i) rank += (tm[j] <= tm[i]) ? 1u : 0u;
            if (j > i) rank += (tm[j] < tm[i]) ? 1u : 0u;
        }
        if (tm[i] != INFINITY) { order |= (uint32_t)i << (3u * rank); nh++; }
    }
    Frame f;
    f.first = first;
    f.w1 = order | (nh << 24) | (anymax ? F_ANYMAX : 0u);
    f.t = 0.f;
    f.tri = 0;
    return f;
}

// get_box_min_time_intersection (raytrace.rs:1012-1050)
template <bool COUNT>
__device__ inline bool leaf_scan(const DScene& sc, uint32_t first, uint32_t count, const RayK& r, float& t_o,
                                 uint32_t& tf_o, unsigned long long* cnt) {
    bool have = false;
    float bt = 0.f;
    uint32_t btf = 0;
    if (COUNT) cnt[4]++;
    for (uint32_t i = 0; i < count; i++) {
        uint32_t tri = sc.refs[first + i];
        float t; uint32_t face;
        if (tri_test<COUNT>(sc, tri, r, t, face, cnt)) {
            if (!have || t < bt) { bt = t; btf = tri | (face << 30); }
            have = true;
        }
    }
    t_o = bt; tf_o = btf;
    return have;
}

__device__ inline void merge(Frame& f, bool have, float t, uint32_t tf) {
    // fold step of raytrace.rs:949-1007: first hit is taken, later ones replace iff strictly closer
    if (have) {
        if (!(f.w1 & F_HAS) || t < f.t) { f.t = t; f.tri = tf; }
        f.w1 |= F_HAS;
    }
}

template <bool COUNT>
__device__ inline bool traverse(const DScene& sc, const RayK& r, uint32_t* lds, int nthreads, int tid, float& t_o,
                                uint32_t& tf_o, unsigned long long* cnt) {
    const DNode root = sc.nodes[0];
    if (root.is_leaf) return leaf_scan<COUNT>(sc, root.first, root.count, r, t_o, tf_o, cnt);
    if (COUNT) cnt[3]++;
    Frame cur = expand<COUNT>(sc, root.first, root.count, r, cnt);
    int sp = 0;
    for (;;) {
        if (F_COUNT(cur.w1) == 0) {
            if (sp == 0) break;
            const bool have = (cur.w1 & F_HAS) != 0;
            const float ct = cur.t;
            const uint32_t ctf = cur.tri;
            sp--;
            uint32_t* fr = lds + (size_t)sp * 4 * nthreads + tid;
            cur.first = fr[0];
            cur.w1 = fr[nthreads];
            cur.t = __uint_as_float(fr[2 * nthreads]);
            cur.tri = fr[3 * nthreads];
            merge(cur, have, ct, ctf);
            continue;
        }
        const uint32_t c = cur.w1 & 7u;
        cur.w1 = ((cur.w1 & 0x00FFFFFFu) >> 3) | ((cur.w1 & 0xFF000000u) - (1u << 24));
        const DNode ch = sc.nodes[cur.first + c];
        if (cur.w1 & F_HAS) {
            float tmin;
            collides(ch.cx, ch.cy, ch.cz, ch.half, r, tmin);
            if (!(tmin < cur.t)) { cur.w1 &= ~(15u << 24); continue; }  // raytrace.rs:965
        } else if (cur.w1 & F_ANYMAX) {
            float tmin;
            collides(ch.cx, ch.cy, ch.cz, ch.half, r, tmin);
            if (tmin == FLT_MAX) continue;  // raytrace.rs:986
        }
        if (ch.is_leaf) {
            float t; uint32_t tf;
            bool have = leaf_scan<COUNT>(sc, ch.first, ch.count, r, t, tf, cnt);
            merge(cur, have, t, tf);
        } else {
            uint32_t* fr = lds + (size_t)sp * 4 * nthreads + tid;
            fr[0] = cur.first;
            fr[nthreads] = cur.w1;
            fr[2 * nthreads] = __float_as_uint(cur.t);
            fr[3 * nthreads] = cur.tri;
            sp++;
            if (COUNT) cnt[3]++;
            cur = expand<COUNT>(sc, ch.first, ch.count, r, cnt);
        }
    }
    t_o = cur.t; tf_o = cur.tri;
    return (cur.w1 & F_HAS) != 0;
}

// Persistent closest-hit kernel: each wave pulls 64 queued rays at a time.
template <bool COUNT>
__global__ void __launch_bounds__(256) k_trace(DScene sc, const float4* __restrict__ qo, const float4* __restrict__ qd,
                                               DCtrl* __restrict__ ctrl, int pass, uint32_t* __restrict__ hit_tf,
                                               float* __restrict__ hit_t) {
    extern __shared__ uint32_t lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const uint32_t count = ctrl->count[pass];
    uint32_t* head = &ctrl->head[pass];
    if (blockIdx.x == 0 && tid == 0) atomicAdd(&ctrl->rays, (unsigned long long)count);
    unsigned long long cnt[5] = {0, 0, 0, 0, 0};
    for (;;) {
        uint32_t base = 0;
        if (lane == 0) base = atomicAdd(head, 64u);
        base = __builtin_amdgcn_readfirstlane(base);
        if (base >= count) break;
        const uint32_t i = base + lane;
        if (i < count) {
            const RayK r = make_rayk(qo[i], qd[i]);
            float t = 0.f; uint32_t tf = 0;
            bool have = traverse<COUNT>(sc, r, lds, blockDim.x, tid, t, tf, cnt);
            hit_tf[i] = have ? tf : 0u;
            hit_t[i] = have ? t : 0.f;
        }
    }
    if (COUNT) {
#pragma unroll
        for (int k = 0; k < 5; k++)
            if (cnt[k]) atomicAdd(&ctrl->counters[k], cnt[k]);
    }
}

}  // namespace rtmi
#include "make_triangle.hpp"
#include "build_octree.hpp"
#include "shade.hpp"
#include "trace_oct.hpp"
#include "hybrid.hpp"
#include "bvh_fast.hpp"
#include "denoise.hpp"
#include "ao.hpp"
#include "light.hpp"
#include "preview.hpp"
#include "rays.hpp"
#include "bake.hpp"
#include "shadowed.hpp"
#include "envlight.hpp"
#include "lit.hpp"
#include "emissive.hpp"
namespace rtmi {


// ---------------------------------------------------------------- linear-list closest hit (root box is a leaf)
// build_trivial_bounding_box (raytrace.rs:847-856): every ray scans the same list, so the list is
// streamed ONCE per 256 rays through LDS in chunks of RTMI_LIN_CHUNK triangles (coalesced float4 gathers
// by the whole block, double-buffered against the tests) and every lane reads the records at a
// wave-uniform LDS address (broadcast).  Fold and test exactly as get_box_min_time_intersection /
// Triangle::intersects (raytrace.rs:1012-1050, 400-439).
// OCCL (k_occluded_linear, rtmi_occluded*): the any-hit form.  A ray whose fold accumulator is < its tmax after a chunk is
// answered 1 and tests no further chunk (the accumulator only falls from there; a NaN accumulator sticks and never passes
// `lt < tmax`); its lane keeps staging, which is the whole block's work, and a block whose 256 rays are all answered
// leaves the list.  A ray that never gets there scans the whole list and answers 0.
#define RTMI_LIN_CHUNK 64
template <bool COUNT, bool OCCL>
__device__ __forceinline__ void trace_linear(const DScene& sc, const float4* __restrict__ qo, const float4* __restrict__ qd,
                                             DCtrl* __restrict__ ctrl, int pass, uint32_t* __restrict__ hit_tf,
                                             float* __restrict__ hit_t, const float* __restrict__ tmax, uint8_t* __restrict__ occ) {
    constexpr int C = RTMI_LIN_CHUNK;
    __shared__ float4 rec[2][6][C];   // [buffer][plane0, plane1, edge0..3][triangle]
    __shared__ uint32_t rid[2][C];
    __shared__ uint32_t s_base;
    const int tid = threadIdx.x;
    const uint32_t count = ctrl->count[pass];
    if (blockIdx.x == 0 && tid == 0) atomicAdd(&ctrl->rays, (unsigned long long)count);
    const DNode root = sc.nodes[0];
    const uint32_t first = root.first, ntri = root.count;
    const uint32_t nchunks = (ntri + C - 1) / C;
    unsigned long long cnt[5] = {0, 0, 0, 0, 0};
    // staging: slot s of a chunk = float4 number (s / C) of triangle (s % C); 6*C slots, 256 threads
    auto stage_load = [&](uint32_t chunk, float4 (&v)[2], uint32_t (&id)[2]) {
#pragma unroll
        for (int k = 0; k < 2; k++) {
            const uint32_t s = tid + k * 256;
            v[k] = make_float4(0.f, 0.f, 0.f, 0.f);
            id[k] = 0;
            if (s < 6 * C) {
                const uint32_t j = chunk * C + (s % C), c = s / C;
                if (j < ntri) {
                    const uint32_t t = sc.refs[first + j];
                    id[k] = t;
                    v[k] = c < 2 ? sc.tplane[2 * t + c] : sc.tedge[4 * t + (c - 2)];
                }
            }
        }
    };
    auto stage_store = [&](int buf, const float4 (&v)[2], const uint32_t (&id)[2]) {
#pragma unroll
        for (int k = 0; k < 2; k++) {
            const uint32_t s = tid + k * 256;
            if (s < 6 * C) {
                rec[buf][s / C][s % C] = v[k];
                if (s < C) rid[buf][s] = id[k];
            }
        }
    };
    for (;;) {
        __syncthreads();
        if (tid == 0) s_base = atomicAdd(&ctrl->head[pass], 256u);
        __syncthreads();
        const uint32_t base = s_base;
        if (base >= count) break;
        const uint32_t i = base + tid;
        const bool active = i < count;
        const RayK r = active ? make_rayk(qo[i], qd[i]) : make_rayk(make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 1.f, 0.f));
        bool lhave = false;
        float lt = 0.f;
        uint32_t ltf = 0;
        const float tmx = OCCL ? (active ? (tmax ? tmax[i] : INFINITY) : 0.f) : 0.f;
        bool done = OCCL && !active;  // OCCL: this lane tests no more (answered, or it has no ray)
        float4 v[2];
        uint32_t id[2];
        if (nchunks) { stage_load(0, v, id); stage_store(0, v, id); }
        __syncthreads();
        for (uint32_t ch = 0; ch < nchunks; ch++) {
            const int buf = ch & 1;
            const bool next = ch + 1 < nchunks;
            if (next) stage_load(ch + 1, v, id);  // global gathers in flight while this chunk is tested
            const uint32_t n = (OCCL && done) ? 0u : min((uint32_t)C, ntri - ch * C);
            for (uint32_t j = 0; j < n; j++) {
                const float4 p0 = rec[buf][0][j], p1 = rec[buf][1][j];
                const float ax = p0.x - r.ox, ay = p0.y - r.oy, az = p0.z - r.oz;
                const float num = (((0.f + p1.x * ax) + p1.y * ay) + p1.z * az) + r.qn;
                const float den = (((0.f + p1.x * r.dx) + p1.y * r.dy) + p1.z * r.dz) + r.qd;
                const float t = num / den;
                if (!(t < 0.f)) {
                    const float px = r.dx * t + r.ox, py = r.dy * t + r.oy, pz = r.dz * t + r.oz, pw = r.dw * t + r.ow;
                    const float ix = px - p0.x, iy = py - p0.y, iz = pz - p0.z;
                    const float l2 = ((ix * ix + iy * iy) + iz * iz) + pw * pw;
                    if (!(l2 > p0.w)) {
                        if (COUNT && active) cnt[2]++;
                        const float4 e0 = rec[buf][2][j], e1 = rec[buf][3][j], e2 = rec[buf][4][j], e3 = rec[buf][5][j];
                        const float z = pw * 0.f;
                        const float d0 = ((ix * e0.x + iy * e0.y) + iz * e0.z) + z;
                        const float d1 = ((ix * e1.x + iy * e1.y) + iz * e1.z) + z;
                        const float d2 = ((ix * e2.x + iy * e2.y) + iz * e2.z) + z;
                        const bool inside = !(d0 > e0.w) & !(d1 > e1.w) & !(d2 > e2.w);
                        const bool edge = (d0 > e3.x) | (d1 > e3.y) | (d2 > e3.z);
                        const uint32_t face = (den > 0.f ? 1u : 0u) | (edge ? 2u : 0u);
                        const bool take = inside & (!lhave | (t < lt));
                        lt = take ? t : lt;
                        ltf = take ? (rid[buf][j] | (face << 30)) : ltf;
                        lhave = lhave | inside;
                    }
                }
            }
            if (COUNT && active) cnt[1] += n;
            if (next) stage_store(buf ^ 1, v, id);
            if (OCCL) {
                done = done | (lhave && lt < tmx);
                if (__syncthreads_count(!done) == 0) break;  // (the barrier of the other form, with the block's vote)
            } else __syncthreads();
        }
        if (active) {
            if (COUNT) cnt[4]++;
            if (OCCL) occ[i] = (lhave && lt < tmx) ? (uint8_t)1 : (uint8_t)0;
            else {
                hit_tf[i] = lhave ? ltf : 0u;
                hit_t[i] = lhave ? lt : 0.f;
            }
        }
    }
    if (COUNT) {
#pragma unroll
        for (int k = 0; k < 5; k++)
            if (cnt[k]) atomicAdd(&ctrl->counters[k], cnt[k]);
    }
}
template <bool COUNT>
__global__ void __launch_bounds__(256) k_trace_linear(DScene sc, const float4* __restrict__ qo, const float4* __restrict__ qd,
                                                      DCtrl* __restrict__ ctrl, int pass, uint32_t* __restrict__ hit_tf,
                                                      float* __restrict__ hit_t) {
    trace_linear<COUNT, false>(sc, qo, qd, ctrl, pass, hit_tf, hit_t, nullptr, nullptr);
}
template <bool COUNT>
__global__ void __launch_bounds__(256) k_occluded_linear(DScene sc, const float4* __restrict__ qo, const float4* __restrict__ qd,
                                                         DCtrl* __restrict__ ctrl, int pass, const float* __restrict__ tmax,
                                                         uint8_t* __restrict__ occ) {
    trace_linear<COUNT, true>(sc, qo, qd, ctrl, pass, nullptr, nullptr, tmax, occ);
}

// rtmi_occluded* from closest hits (generic tree, BVH mode, scenes with analytic spheres; the definition itself, and what the
// tests hold the any-hit kernels against): occ[i] = (tri != 0 && t < tmax[i]), tmax null = +inf
__global__ void __launch_bounds__(256) k_occl_from_hits(uint32_t n, const uint32_t* __restrict__ hit_tf, const float* __restrict__ hit_t,
                                                        const float* __restrict__ tmax, uint8_t* __restrict__ occ) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        occ[i] = ((hit_tf[i] & 0x3FFFFFFFu) != 0u && hit_t[i] < (tmax ? tmax[i] : INFINITY)) ? (uint8_t)1 : (uint8_t)0;
}

// ---------------------------------------------------------------- generation / shading (per-pass pipeline)
// pixel_ray / color_ray themselves are in shade.hpp (shared with the path kernels of trace_oct.hpp).
// S (shade.hpp): k_gen / k_shade are Samp::FRAME, k_gen_samples / k_shade_samples PASS, k_gen_list / k_shade_list LIST,
// k_gen_views / k_shade_views VIEWS (the view table is an argument of these two only), k_shade_rays RAYS (no k_gen: the rays
// are the caller's, rays.hpp has the kernel that stands in its place).  k_gen_camera (camera.hpp, included below) is a second
// PASS generator, for the built-in camera models; its passes are shaded by k_shade_samples.
#define RTMI_GEN_PARAMS uint64_t seed, uint32_t pix0, uint32_t npaths, float4* __restrict__ qo, float4* __restrict__ qd, \
                        uint32_t* __restrict__ qpath, DCtrl* __restrict__ ctrl
#define RTMI_GEN_ARGS v, seed, pix0, npaths, qo, qd, qpath, ctrl
template <Samp S>
__device__ __forceinline__ void gen_paths(const DView& v, RTMI_GEN_PARAMS, const uint32_t* __restrict__ list = nullptr,
                                          const ViewTab& vt = ViewTab{}) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t path = blockIdx.x * blockDim.x + threadIdx.x; path < npaths; path += stride) {
        uint32_t row, col, sample;
        path_pixel<S>(v, pix0, path, row, col, sample, list);
        const PixKey key = pixel_key<S>(v, row, vt);
        RayV r = pixel_ray<S>(v, key.row, col, key_seed<S>(key, vt, seed), key.row * v.width + col, sample, S == Samp::VIEWS ? &vt.cams[key.view] : nullptr);
        qo[path] = make_float4(r.orig.x, r.orig.y, r.orig.z, r.orig.w);
        qd[path] = make_float4(r.dir.x, r.dir.y, r.dir.z, r.dir.w);
        qpath[path] = path;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) ctrl->count[0] = npaths;
}
__global__ void __launch_bounds__(256) k_gen(DView v, RTMI_GEN_PARAMS) { gen_paths<Samp::FRAME>(RTMI_GEN_ARGS); }
__global__ void __launch_bounds__(256) k_gen_samples(DView v, RTMI_GEN_PARAMS) { gen_paths<Samp::PASS>(RTMI_GEN_ARGS); }
__global__ void __launch_bounds__(256) k_gen_list(DView v, RTMI_GEN_PARAMS, const uint32_t* __restrict__ list) { gen_paths<Samp::LIST>(RTMI_GEN_ARGS, list); }
__global__ void __launch_bounds__(256) k_gen_views(DView v, RTMI_GEN_PARAMS, ViewTab vt) { gen_paths<Samp::VIEWS>(RTMI_GEN_ARGS, nullptr, vt); }
}  // namespace rtmi
#include "camera.hpp"  // k_gen_camera: a PASS generator for the built-in camera models (rtmi_render_camera*)
namespace rtmi {

// color_ray + the tail of project_ray for every ray of pass `pass`.
#define RTMI_SHADE_PARAMS DScene sc, DView v, uint64_t seed, uint32_t pix0, uint32_t npaths, int pass,                  \
                          const float4* __restrict__ qo, const float4* __restrict__ qd,                                \
                          const uint32_t* __restrict__ qpath, const uint32_t* __restrict__ hit_tf,                     \
                          const float* __restrict__ hit_t, float4* __restrict__ qo_n, float4* __restrict__ qd_n,       \
                          uint32_t* __restrict__ qpath_n, uint16_t* __restrict__ mstack, float4* __restrict__ scol,    \
                          DCtrl* __restrict__ ctrl, SlowQ slow
#define RTMI_SHADE_ARGS sc, v, seed, pix0, npaths, pass, qo, qd, qpath, hit_tf, hit_t, qo_n, qd_n, qpath_n, mstack, scol, ctrl, slow
// L: the shading level (Shade, shade.hpp); the level's tables follow the mode's own argument.
template <Samp S, Shade L = Shade::PLAIN>
__device__ __forceinline__ void shade_pass(RTMI_SHADE_PARAMS, const uint32_t* __restrict__ list = nullptr, const ViewTab& vt = ViewTab{},
                                           const EnvTab* env = nullptr, const SmoothTab* sm = nullptr, const TexTab* tex = nullptr,
                                           float4* __restrict__ cstack = nullptr, const NmapTab* nm = nullptr) {
    __shared__ uint32_t s_cnt[4], s_base;
    const uint32_t count = ctrl->count[pass];
    const uint32_t stride = gridDim.x * blockDim.x;
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    // round the loop bound up so that whole BLOCKS stay converged for the ballot and the block-wide queue reservation
    const uint32_t bound = (count + 255u) & ~255u;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < bound; i += stride) {
        bool push = false;
        RayV nr;
        uint32_t path = 0;
        if (i < count) {
            // a miss (sky) or an edge face ends the path without looking at the ray: 2/3 of the primary rays never touch
            // their 36 bytes of origin / direction / hit time.  What a hit needs is requested together: the loads do not
            // depend on each other.
            path = qpath[i];
            const uint32_t tf = hit_tf[i];
            float t = 0.f;
            float4 o4 = make_float4(0.f, 0.f, 0.f, 0.f), d4 = make_float4(0.f, 0.f, 1.f, 0.f);
            if ((tf & 0x3FFFFFFFu) != 0u && !((tf >> 30) & 2u)) { t = hit_t[i]; o4 = qo[i]; d4 = qd[i]; }
            if constexpr (L >= Shade::ENV) {  // a miss looks the environment up in its ray's direction
                if ((tf & 0x3FFFFFFFu) == 0u) d4 = qd[i];
            }
            if constexpr (S == Samp::RAYS) {  // `list` = the batch's RNG keys (or null), pix0 = the key of its first group
                uint32_t pixel, sample;
                rays_key(v, pix0, path, list, pixel, sample);
                push = shade_hit<L>(sc, v.maxdepth, seed, npaths, path, pixel, sample, (uint32_t)pass, tf, t, V4{o4.x, o4.y, o4.z, o4.w},
                                                     V4{d4.x, d4.y, d4.z, d4.w}, mstack, scol, nr, nullptr, env, sm, tex, cstack, nm);
            } else {
            uint32_t prow, pcol, sample;
            path_pixel<S>(v, pix0, path, prow, pcol, sample, list);
            const PixKey key = pixel_key<S>(v, prow, vt);
            push = shade_hit<L>(sc, v.maxdepth, key_seed<S>(key, vt, seed), npaths, path, key.row * v.width + pcol, sample, (uint32_t)pass, tf, t,
                                                 V4{o4.x, o4.y, o4.z, o4.w}, V4{d4.x, d4.y, d4.z, d4.w}, mstack, scol, nr, nullptr, env, sm, tex, cstack, nm);
            }
            // a bounce ray with an exactly-zero direction component goes to the slow path (SlowQ), not to the next pass
            if (push && slow.cap && has_zero_component(nr.dir.x, nr.dir.y, nr.dir.z) &&
                slow_push(slow, ctrl, make_float4(nr.orig.x, nr.orig.y, nr.orig.z, nr.orig.w), make_float4(nr.dir.x, nr.dir.y, nr.dir.z, nr.dir.w),
                          path, (uint32_t)pass + 1u))
                push = false;
        }
        // compact surviving rays into the next queue: ballot + prefix sum per wave, ONE atomic per block of four waves.  (One
        // per wave made the queue counter the kernel's bottleneck: 1.7 M same-address atomics per frame at ~4.8 ns each were
        // half of its 16.7 ms.)
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
                const uint32_t slot = base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
                store_stream(&qo_n[slot], make_float4(nr.orig.x, nr.orig.y, nr.orig.z, nr.orig.w));
                store_stream(&qd_n[slot], make_float4(nr.dir.x, nr.dir.y, nr.dir.z, nr.dir.w));
                store_stream(&qpath_n[slot], path);
            }
        }
        __syncthreads();  // s_cnt / s_base are rewritten by the next iteration
    }
}
// The 30 shading kernels: one per sampling mode (k_shade, k_shade_samples, k_shade_list, k_shade_views, k_shade_rays) and shading
// level (no suffix, _glass, _env, _smooth, _tex, _nmap).  A level's kernels take, after the mode's own argument, the tables of the
// level and of every level below it (RTMI_TAIL_P_<level>), and hand them to shade_pass (RTMI_TAIL_A_<level>).  cstack: the colour
// stack, one float4 (colour.rgb, alpha) beside every mstack entry.  k_shade_rays (rtmi_render_rays*): v carries maxdepth, spp = the
// group size and dspp only; keys = the batch's RNG keys or null.
#define RTMI_TAIL_P_PLAIN
#define RTMI_TAIL_A_PLAIN
#define RTMI_TAIL_P_GLASS
#define RTMI_TAIL_A_GLASS
#define RTMI_TAIL_P_ENV , EnvTab env
#define RTMI_TAIL_A_ENV , &env
#define RTMI_TAIL_P_SMOOTH RTMI_TAIL_P_ENV, SmoothTab sm
#define RTMI_TAIL_A_SMOOTH RTMI_TAIL_A_ENV, &sm
#define RTMI_TAIL_P_TEX RTMI_TAIL_P_SMOOTH, TexTab tex, float4* __restrict__ cstack
#define RTMI_TAIL_A_TEX RTMI_TAIL_A_SMOOTH, &tex, cstack
#define RTMI_TAIL_P_NMAP RTMI_TAIL_P_TEX, NmapTab nm
#define RTMI_TAIL_A_NMAP RTMI_TAIL_A_TEX, &nm
#define RTMI_SHADE_KERNELS(sfx, LV)                                                                                                       \
    __global__ void __launch_bounds__(256) k_shade##sfx(RTMI_SHADE_PARAMS RTMI_TAIL_P_##LV) {                                             \
        shade_pass<Samp::FRAME, Shade::LV>(RTMI_SHADE_ARGS, nullptr, ViewTab{} RTMI_TAIL_A_##LV);                                         \
    }                                                                                                                                     \
    __global__ void __launch_bounds__(256) k_shade_samples##sfx(RTMI_SHADE_PARAMS RTMI_TAIL_P_##LV) {                                     \
        shade_pass<Samp::PASS, Shade::LV>(RTMI_SHADE_ARGS, nullptr, ViewTab{} RTMI_TAIL_A_##LV);                                          \
    }                                                                                                                                     \
    __global__ void __launch_bounds__(256) k_shade_list##sfx(RTMI_SHADE_PARAMS, const uint32_t* __restrict__ list RTMI_TAIL_P_##LV) {     \
        shade_pass<Samp::LIST, Shade::LV>(RTMI_SHADE_ARGS, list, ViewTab{} RTMI_TAIL_A_##LV);                                             \
    }                                                                                                                                     \
    __global__ void __launch_bounds__(256) k_shade_views##sfx(RTMI_SHADE_PARAMS, ViewTab vt RTMI_TAIL_P_##LV) {                           \
        shade_pass<Samp::VIEWS, Shade::LV>(RTMI_SHADE_ARGS, nullptr, vt RTMI_TAIL_A_##LV);                                                \
    }                                                                                                                                     \
    __global__ void __launch_bounds__(256) k_shade_rays##sfx(RTMI_SHADE_PARAMS, const uint32_t* __restrict__ keys RTMI_TAIL_P_##LV) {     \
        shade_pass<Samp::RAYS, Shade::LV>(RTMI_SHADE_ARGS, keys, ViewTab{} RTMI_TAIL_A_##LV);                                             \
    }
RTMI_SHADE_KERNELS(, PLAIN)
RTMI_SHADE_KERNELS(_glass, GLASS)   // RTMI_DIELECTRIC, DESIGN.md 4.22
RTMI_SHADE_KERNELS(_env, ENV)       // rtmi_scene_set_environment / rtmi_scene_set_sky, DESIGN.md 4.23
RTMI_SHADE_KERNELS(_smooth, SMOOTH) // rtmi_scene_set_normals, DESIGN.md 4.24
RTMI_SHADE_KERNELS(_tex, TEX)       // rtmi_scene_set_textures, DESIGN.md 4.25
RTMI_SHADE_KERNELS(_nmap, NMAP)     // rtmi_scene_set_normal_maps, DESIGN.md 4.26
// one mode's six kernels in level order, for launch_shade
#define RTMI_SHADE_ROW(k) k, k##_glass, k##_env, k##_smooth, k##_tex, k##_nmap

// rtmi_scene_set_sky: texel (i, j) of an n x n environment table from the inverse of env_lookup's map -- the direction of the
// texel's centre -- and a gradient sky with a sun disc, operation by operation as include/rtmi.h lists it.  One thread per texel.
struct SkyArgs { float4 up, sun_dir, zenith, horizon, ground, sun_color; float sun_cos; };
__global__ void __launch_bounds__(256) k_env_sky(float4* __restrict__ tab, uint32_t n, float fn, SkyArgs a) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n * n) return;
    const uint32_t j = k / n, i = k - j * n;
    auto v4 = [](float4 q) { return V4{q.x, q.y, q.z, q.w}; };
    float px = ((float)i + 0.5f) / fn * 2.f - 1.f, py = ((float)j + 0.5f) / fn * 2.f - 1.f;
    const float z = (1.f - fabsf(px)) - fabsf(py);
    if (z < 0.f) oct_fold(px, py);
    const V4 dir = vunit(mk(px, py, z));
    const float h = vdot(dir, vunit(v4(a.up)));
    V4 c = h < 0.f ? v4(a.ground) : mix_color(v4(a.horizon), v4(a.zenith), h);
    if (vdot(dir, vunit(v4(a.sun_dir))) >= a.sun_cos) c = vadd(c, v4(a.sun_color));
    tab[k] = make_float4(c.x, c.y, c.z, 0.f);
}

// walk_ray_set's per-pixel accumulation (raytrace.rs:1414-1426): acc = 0; acc += sample_i in sample order; * (1/spp).
// The sample colours of a pixel are consecutive in `scol` ([pixel][sample]), so one thread per pixel would read 16 B at a
// stride of spp * 16 B (round 2: 5.9 x the bytes fetched, 128-B lines evicted between a thread's iterations).  Instead a
// block takes RTMI_ACC_PIX consecutive pixels, streams their samples through LDS in chunks with fully coalesced float4
// loads, and thread (pixel j, channel c) adds its pixel's samples of the chunk in order, keeping the running sum in a
// register across chunks -- the same sequence of f32 additions per channel as the reference's Vec3 adds.  One float4 of
// padding per 64 keeps the 16 pixels that are summed at a time (spp = 64) on different LDS banks.
// `out` is the caller's tile buffer; the sub-tile `sub` of `nsub` holds every nsub-th ROW of that tile, so local row lr of
// the sub-tile is row lr * nsub + sub of the buffer.
#define RTMI_ACC_PIX 64
#define RTMI_ACC_CHUNK 1024
// Samp::FRAME: k_accum, the sum starts at 0.f and out = sum * inv.  PASS: k_accum_samples (progressive passes), the sum
// starts from accum when `resume`, is written back to accum, and out (when not NULL) = sum * inv.
// LIST: k_accum_list (adaptive passes), a PASS whose block's pixels are list[pix0 + pb + j], tile-local pixel indices (= their
// float4 in accum / sumsq / out); the per-lane sum of squares q = q + c * c continues in sumsq beside the sum, and
// counts[pixel] receives `ncount`, the pixel's samples after this pass.
template <Samp S>
__device__ __forceinline__ void accum_pixels(uint32_t npixels, uint32_t spp, const float4* __restrict__ scol, float* __restrict__ out,
                                             float* __restrict__ accum, bool resume, float inv, uint32_t pix0, uint32_t W,
                                             uint32_t nsub, uint32_t sub, FastDiv dW, const uint32_t* __restrict__ list = nullptr,
                                             float* __restrict__ sumsq = nullptr, uint32_t* __restrict__ counts = nullptr,
                                             uint32_t ncount = 0u) {
    __shared__ float4 stage[RTMI_ACC_CHUNK + RTMI_ACC_CHUNK / 64 + 1];
    const float* stage_f = reinterpret_cast<const float*>(stage);
    const uint32_t tid = threadIdx.x, j = tid >> 2, c = tid & 3u;
    for (uint32_t pb = blockIdx.x * RTMI_ACC_PIX; pb < npixels; pb += gridDim.x * RTMI_ACC_PIX) {
        const uint32_t npb = min((uint32_t)RTMI_ACC_PIX, npixels - pb);
        const uint32_t f0 = pb * spp, f1 = f0 + npb * spp;       // the block's samples: scol[f0 .. f1)
        const uint32_t my0 = f0 + j * spp, my1 = my0 + spp;      // this thread's pixel (when j < npb)
        size_t o = 0;                                            // PASS / LIST: this thread's float in accum / out
        float acc = 0.f, sq = 0.f;                               // sq: LIST only
        uint32_t lpix = 0;                                       // LIST: the tile-local pixel
        if (S == Samp::LIST) {
            if (j < npb) {
                lpix = list[pix0 + pb + j];
                o = (size_t)lpix * 4u + c;
                if (resume) { acc = accum[o]; sq = sumsq[o]; }
            }
        } else if (S == Samp::PASS && j < npb) {
            const uint32_t lp = pix0 + pb + j, lr = fdiv(lp, dW), col = lp - lr * W;
            o = (((size_t)lr * nsub + sub) * W + col) * 4u + c;
            if (resume) acc = accum[o];
        }
        for (uint32_t ch = f0; ch < f1; ch += RTMI_ACC_CHUNK) {
            const uint32_t n = min((uint32_t)RTMI_ACC_CHUNK, f1 - ch);
            __syncthreads();  // the previous chunk has been consumed
            for (uint32_t k = tid; k < n; k += 256u) stage[k + (k >> 6)] = scol[ch + k];
            __syncthreads();
            if (j < npb) {
                const uint32_t lo = max(my0, ch), hi = min(my1, ch + n);
                for (uint32_t s = lo; s < hi; s++) {
                    const uint32_t k = s - ch;
                    const float x = stage_f[(k + (k >> 6)) * 4u + c];
                    acc = acc + x;
                    if (S == Samp::LIST) sq = sq + x * x;
                }
            }
        }
        if (j < npb) {
            if (S != Samp::FRAME) {
                accum[o] = acc;
                if (S == Samp::LIST) {
                    sumsq[o] = sq;
                    if (c == 0u) counts[lpix] = ncount;
                }
                if (out) out[o] = acc * inv;
            } else {
                const uint32_t lp = pix0 + pb + j, lr = fdiv(lp, dW), col = lp - lr * W;
                const size_t orow = (size_t)lr * nsub + sub;
                out[(orow * W + col) * 4u + c] = acc * inv;
            }
        }
    }
}
__global__ void __launch_bounds__(256) k_accum(uint32_t npixels, uint32_t spp, const float4* __restrict__ scol,
                                               float* __restrict__ out, uint32_t pix0, uint32_t W, uint32_t nsub, uint32_t sub,
                                               FastDiv dW) {
    accum_pixels<Samp::FRAME>(npixels, spp, scol, out, nullptr, false, 1.f / (float)spp, pix0, W, nsub, sub, dW);
}
// Samples [sample0, sample0 + nsamples) of every pixel: continuing the running sum of samples [0, sample0) in accum performs
// the same f32 additions in the same order as k_accum over all samples, so the passes of a frame end in the same bits.
// `out` = the preview sum * (1/(sample0 + nsamples)); `accum` and `out` are the same tile layout and never overlap.
__global__ void __launch_bounds__(256) k_accum_samples(uint32_t npixels, uint32_t nsamples, uint32_t sample0, const float4* __restrict__ scol,
                                                       float* __restrict__ accum, float* __restrict__ out, uint32_t pix0, uint32_t W,
                                                       uint32_t nsub, uint32_t sub, FastDiv dW) {
    accum_pixels<Samp::PASS>(npixels, nsamples, scol, out, accum, sample0 != 0u, 1.f / (float)(sample0 + nsamples), pix0, W, nsub, sub, dW);
}
// Adaptive passes: samples [sample0, sample0 + nsamples) of the list's pixels pix0 .. pix0 + npixels - 1.  Every pixel of the
// list has had exactly sample0 samples, so the sum and the sum of squares continue in sample order from 0.f (sample0 == 0)
// and out = sum * (1/count) is k_accum's arithmetic at spp = count: the pixel of a uniform render at that many samples.
__global__ void __launch_bounds__(256) k_accum_list(uint32_t npixels, uint32_t nsamples, uint32_t sample0, const float4* __restrict__ scol,
                                                    float* __restrict__ accum, float* __restrict__ sumsq, uint32_t* __restrict__ counts,
                                                    float* __restrict__ out, const uint32_t* __restrict__ list, uint32_t pix0) {
    const uint32_t n = sample0 + nsamples;
    accum_pixels<Samp::LIST>(npixels, nsamples, scol, out, accum, sample0 != 0u, 1.f / (float)n, pix0, 0u, 0u, 0u, FastDiv{},
                             list, sumsq, counts, n);
}

// ---------------------------------------------------------------- first-hit feature buffers (rtmi_render_features*)
// k_features stands where k_shade and k_accum stand in a progressive pass whose only pass is the primary one: it turns the
// closest hits of the batch's primary rays (queue slot == path, a pixel's paths consecutive: [pixel][sample]) into per-pixel
// means of (albedo.rgb, coverage) and (normal.xyz, depth), and the hit id of each pixel's first sample.  There is no per-path
// intermediate in memory: 8 B per path are read, 36 B per pixel written.
// accum_pixels' scheme with 8 lanes per pixel: a block takes RTMI_FEAT_PIX consecutive pixels and walks their paths in
// chunks.  Staging: thread k of the chunk reads its path's hit_tf / hit_t (coalesced), gathers the features of that hit
// (hit_features, shade.hpp: once per path) and writes the 8 floats to LDS.  Summing: thread (pixel j, lane l) adds lane l of
// its pixel's samples in sample order from 0.f, carrying the sum across chunks: walk_ray_set's sequence of f32 additions.
// LDS banks: a ds_read_b32 is served per 32-lane half = 4 pixels x 8 lanes, on banks (entry * 8 + l) % 32, so the 4 pixels'
// entries must differ mod 4.  With nsamples % 4 == 0 they would all be equal (entry = j * nsamples + s); an entry is therefore
// stored rotated by its pixel inside its aligned group of four entries (which then belong to one pixel): conflict-free for
// nsamples = 4, 8, 16, 64, ...; other counts are left as they fall (nsamples % 4 == 2: two-way).
#define RTMI_FEAT_PIX 32
#define RTMI_FEAT_CHUNK 512  // paths per chunk: 16 KB of LDS
__device__ inline uint32_t feat_slot(uint32_t k, uint32_t rot) { return (k & ~3u) | ((k + rot) & 3u); }
// Sub-tile and stripe addressing of the outputs is accum_pixels<Samp::PASS>'s.  albedo / normal (float4 per pixel) and ids
// (uint32 per pixel) may each be NULL.  dS: n / nsamples.
// L: the shading level (Shade, shade.hpp) picks the gather.  Below SMOOTH it is hit_features, and glass and the environment do not
// show in a first hit.  From SMOOTH on it is the level's hit_features_* (the normal is the shading normal; TEX: the
// albedo is tex_colour's, 4.25; NMAP: the normal is the mapped one, 4.26), which needs the primary rays (qo, qd: queue slot ==
// path) beside the hit records, and the level's tables (sm may be an empty table).
#define RTMI_FEAT_PARAMS DScene sc, uint32_t npixels, uint32_t nsamples, const uint32_t* __restrict__ hit_tf,                          \
                         const float* __restrict__ hit_t, float* __restrict__ albedo, float* __restrict__ normal,                     \
                         uint32_t* __restrict__ ids, uint32_t pix0, uint32_t W, uint32_t nsub, uint32_t sub, FastDiv dW, FastDiv dS
#define RTMI_FEAT_ARGS sc, npixels, nsamples, hit_tf, hit_t, albedo, normal, ids, pix0, W, nsub, sub, dW, dS
template <Shade L>
__device__ __forceinline__ void features_pass(RTMI_FEAT_PARAMS, const float4* __restrict__ qo = nullptr, const float4* __restrict__ qd = nullptr,
                                              const SmoothTab* sm = nullptr, const TexTab* tex = nullptr, const NmapTab* nm = nullptr) {
    __shared__ float4 stage[2 * RTMI_FEAT_CHUNK];
    const float* stage_f = reinterpret_cast<const float*>(stage);
    const uint32_t tid = threadIdx.x, j = tid >> 3, l = tid & 7u;
    const uint32_t rot = (nsamples & 3u) == 0u ? 1u : 0u;
    const float inv = 1.f / (float)nsamples;
    for (uint32_t pb = blockIdx.x * RTMI_FEAT_PIX; pb < npixels; pb += gridDim.x * RTMI_FEAT_PIX) {
        const uint32_t npb = min((uint32_t)RTMI_FEAT_PIX, npixels - pb);
        const uint32_t f0 = pb * nsamples, nb = npb * nsamples;  // the block's paths: hit_*[f0 .. f0 + nb)
        const uint32_t my0 = j * nsamples, my1 = my0 + nsamples;  // this thread's pixel among them (when j < npb)
        float acc = 0.f;
        for (uint32_t r0 = 0; r0 < nb; r0 += RTMI_FEAT_CHUNK) {
            const uint32_t n = min((uint32_t)RTMI_FEAT_CHUNK, nb - r0);
            __syncthreads();  // the previous chunk has been consumed
            for (uint32_t k = tid; k < n; k += 256u) {
                HitFeat f;
                if constexpr (L < Shade::SMOOTH) {
                    f = hit_features(sc, hit_tf[f0 + r0 + k], hit_t[f0 + r0 + k]);
                } else {
                    const uint32_t tf = hit_tf[f0 + r0 + k];
                    float4 o4 = make_float4(0.f, 0.f, 0.f, 0.f), d4 = make_float4(0.f, 0.f, 1.f, 0.f);
                    if ((tf & 0x3FFFFFFFu) != 0u && !((tf >> 30) & 2u)) { o4 = qo[f0 + r0 + k]; d4 = qd[f0 + r0 + k]; }
                    const V4 ro{o4.x, o4.y, o4.z, o4.w}, rd{d4.x, d4.y, d4.z, d4.w};
                    if constexpr (L == Shade::SMOOTH) f = hit_features_smooth(sc, *sm, tf, hit_t[f0 + r0 + k], ro, rd);
                    else if constexpr (L == Shade::TEX) f = hit_features_tex(sc, *sm, *tex, tf, hit_t[f0 + r0 + k], ro, rd);
                    else f = hit_features_nmap(sc, *sm, *tex, *nm, tf, hit_t[f0 + r0 + k], ro, rd);
                }
                const uint32_t e = feat_slot(k, rot * fdiv(r0 + k, dS));
                stage[2u * e] = f.a;
                stage[2u * e + 1u] = f.n;
            }
            __syncthreads();
            if (j < npb) {
                const uint32_t lo = max(my0, r0), hi = min(my1, r0 + n);
                for (uint32_t s = lo; s < hi; s++) acc = acc + stage_f[feat_slot(s - r0, rot * j) * 8u + l];
            }
        }
        if (j < npb) {
            const uint32_t lp = pix0 + pb + j, lr = fdiv(lp, dW), col = lp - lr * W;
            const size_t o = ((size_t)lr * nsub + sub) * W + col;
            float* __restrict__ dst = l < 4u ? albedo : normal;
            if (dst) store_stream(&dst[o * 4u + (l & 3u)], acc * inv);
            if (ids && l == 0u) store_stream(&ids[o], hit_tf[f0 + my0]);
        }
    }
}
__global__ void __launch_bounds__(256) k_features(RTMI_FEAT_PARAMS) { features_pass<Shade::PLAIN>(RTMI_FEAT_ARGS); }
__global__ void __launch_bounds__(256) k_features_smooth(RTMI_FEAT_PARAMS, const float4* __restrict__ qo, const float4* __restrict__ qd, SmoothTab sm) {
    features_pass<Shade::SMOOTH>(RTMI_FEAT_ARGS, qo, qd, &sm);
}
__global__ void __launch_bounds__(256) k_features_tex(RTMI_FEAT_PARAMS, const float4* __restrict__ qo, const float4* __restrict__ qd, SmoothTab sm,
                                                      TexTab tex) {
    features_pass<Shade::TEX>(RTMI_FEAT_ARGS, qo, qd, &sm, &tex);
}
__global__ void __launch_bounds__(256) k_features_nmap(RTMI_FEAT_PARAMS, const float4* __restrict__ qo, const float4* __restrict__ qd, SmoothTab sm,
                                                       TexTab tex, NmapTab nm) {
    features_pass<Shade::NMAP>(RTMI_FEAT_ARGS, qo, qd, &sm, &tex, &nm);
}

// ---------------------------------------------------------------- adaptive sampling: the stop rule and the next list
// The stop rule of a pixel with n >= 2 samples, sum s and per-lane sum of squares q (rtmi.h, rtmi_render_adaptive):
// the worst channel's squared standard error of the mean against (abs_tol + rel_tol * brightest mean)^2.  f32 in this
// order, max(a, b) = a < b ? b : a, and any NaN means "not stopped" (abs_tol = NaN disables the rule).
__host__ __device__ inline float adapt_max(float a, float b) { return a < b ? b : a; }
__host__ __device__ inline bool adapt_stop(float4 s, float4 q, uint32_t n, float rel_tol, float abs_tol) {
    const float inv = 1.f / (float)n, dn1 = (float)(n - 1u);
    const float mr = s.x * inv, mg = s.y * inv, mb = s.z * inv;
    const float vr = (q.x - s.x * mr) / dn1, vg = (q.y - s.y * mg) / dn1, vb = (q.z - s.z * mb) / dn1;
    const float e = adapt_max(adapt_max(vr, vg), vb) / (float)n;
    const float L = adapt_max(adapt_max(mr, mg), mb);
    const float t = abs_tol + rel_tol * L;
    const bool nan = (mr != mr) | (mg != mg) | (mb != mb) | (vr != vr) | (vg != vg) | (vb != vb) | (e != e) | (t != t);
    return !nan && e <= t * t;
}
// Wave-wide inclusive prefix sum (wave64).
__device__ inline uint32_t wave_incl_scan(uint32_t v) {
    const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const uint32_t u = __shfl_up(v, d, 64);
        if (lane >= d) v += u;
    }
    return v;
}
// 256-thread block: exclusive prefix of v over the block's threads in thread order, and the block's total.  s_w: 4 words of LDS.
__device__ inline uint32_t block_excl_scan256(uint32_t v, uint32_t* s_w, uint32_t& total) {
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint32_t inc = wave_incl_scan(v);
    __syncthreads();  // s_w may still be read by a previous call
    if (lane == 63u) s_w[wv] = inc;
    __syncthreads();
    uint32_t base = 0;
    for (uint32_t k = 0; k < wv; k++) base += s_w[k];
    total = s_w[0] + s_w[1] + s_w[2] + s_w[3];
    return base + inc - v;
}
#define RTMI_ADAPT_BLOCK 256
// list[i] = i: the first pass of an adaptive call covers every pixel of the tile
__global__ void __launch_bounds__(256) k_adapt_init(uint32_t npix, uint32_t* __restrict__ list) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += stride) list[i] = i;
}
// Compaction of the active list in three launches that keep its ascending pixel order: (1) each block of 256 entries
// counts the pixels that go on, (2) one block turns the counts into offsets (and the total, which the host reads back), (3)
// each block writes its survivors at its offset in entry order.  (1) and (3) evaluate the same rule on the same bits.
__device__ inline bool adapt_goes_on(const uint32_t* __restrict__ list, uint32_t nlist, const float4* __restrict__ accum,
                                     const float4* __restrict__ sumsq, uint32_t n, float rel_tol, float abs_tol, uint32_t i,
                                     uint32_t& pixel) {
    if (i >= nlist) return false;
    pixel = list[i];
    return !adapt_stop(accum[pixel], sumsq[pixel], n, rel_tol, abs_tol);
}
__global__ void __launch_bounds__(RTMI_ADAPT_BLOCK) k_adapt_count(const uint32_t* __restrict__ list, uint32_t nlist,
                                                                  const float4* __restrict__ accum, const float4* __restrict__ sumsq,
                                                                  uint32_t n, float rel_tol, float abs_tol, uint32_t* __restrict__ bcnt) {
    __shared__ uint32_t s_w[4];
    uint32_t pixel = 0;
    const bool on = adapt_goes_on(list, nlist, accum, sumsq, n, rel_tol, abs_tol, blockIdx.x * RTMI_ADAPT_BLOCK + threadIdx.x, pixel);
    const unsigned long long mask = __ballot(on);
    if ((threadIdx.x & 63u) == 0u) s_w[threadIdx.x >> 6] = (uint32_t)__popcll(mask);
    __syncthreads();
    if (threadIdx.x == 0) bcnt[blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}
// one block: bcnt[0 .. nblk) -> exclusive offsets in place; bcnt[nblk] = the total
__global__ void __launch_bounds__(256) k_adapt_scan(uint32_t* __restrict__ bcnt, uint32_t nblk) {
    __shared__ uint32_t s_w[4];
    uint32_t carry = 0;
    for (uint32_t b0 = 0; b0 < nblk; b0 += 256u) {
        const uint32_t i = b0 + threadIdx.x;
        const uint32_t v = i < nblk ? bcnt[i] : 0u;
        uint32_t total;
        const uint32_t ex = block_excl_scan256(v, s_w, total);
        if (i < nblk) bcnt[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) bcnt[nblk] = carry;
}
__global__ void __launch_bounds__(RTMI_ADAPT_BLOCK) k_adapt_scatter(const uint32_t* __restrict__ list, uint32_t nlist,
                                                                    const float4* __restrict__ accum, const float4* __restrict__ sumsq,
                                                                    uint32_t n, float rel_tol, float abs_tol,
                                                                    const uint32_t* __restrict__ boff, uint32_t* __restrict__ next) {
    __shared__ uint32_t s_w[4];
    uint32_t pixel = 0;
    const bool on = adapt_goes_on(list, nlist, accum, sumsq, n, rel_tol, abs_tol, blockIdx.x * RTMI_ADAPT_BLOCK + threadIdx.x, pixel);
    uint32_t total;
    const uint32_t slot = block_excl_scan256(on ? 1u : 0u, s_w, total);
    if (on) next[boff[blockIdx.x] + slot] = pixel;
}

// write_png's quantisation (raytrace.rs:1468-1473): `as u8` truncates and saturates, NaN -> 0
__global__ void __launch_bounds__(256) k_quantize(uint64_t npixels, const float4* __restrict__ in, uint8_t* __restrict__ out) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < npixels; p += stride) {
        const float4 c = in[p];
        const float ch[3] = {c.x * 255.f, c.y * 255.f, c.z * 255.f};
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const float x = ch[k];
            out[p * 3 + k] = (x != x) ? 0 : (x <= 0.f ? 0 : (x >= 255.f ? 255 : (uint8_t)x));
        }
    }
}

// rtmi_render_frame_multi: bands of the n scenes, each padded to `mr` rows, lie one after the other in `stage`;
// image row `row` is local row (row / (S*n)) * S + row % S of band (row / S) % n.  `px` = bytes per pixel (16 or 3).
__global__ void __launch_bounds__(256) k_deinterleave(const uint8_t* __restrict__ stage, uint8_t* __restrict__ out, uint32_t W,
                                                      uint32_t H, uint32_t S, uint32_t n, uint32_t mr, uint32_t px) {
    const uint64_t npix = (uint64_t)W * H, stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < npix; p += stride) {
        const uint32_t row = (uint32_t)(p / W), col = (uint32_t)(p - (uint64_t)row * W);
        const uint32_t band = (row / S) % n, lr = (row / (S * n)) * S + row % S;
        const uint64_t src = (((uint64_t)band * mr + lr) * W + col) * px;
        if (px == 16) *reinterpret_cast<float4*>(out + p * 16) = *reinterpret_cast<const float4*>(stage + src);
        else { out[p * 3] = stage[src]; out[p * 3 + 1] = stage[src + 1]; out[p * 3 + 2] = stage[src + 2]; }
    }
}

// Analytic spheres (rtmi_sphere_t; a build-defined extension, see include/rtmi.h): every ray of the pass against the
// scene's flat sphere list, after the tree's closest hit.  4-lane Vec3 arithmetic in the operation order DESIGN.md 4.6 states.
__global__ void __launch_bounds__(256) k_trace_spheres(DScene sc, const float4* __restrict__ qo, const float4* __restrict__ qd,
                                                       const DCtrl* __restrict__ ctrl, int pass, uint32_t* __restrict__ hit_tf,
                                                       float* __restrict__ hit_t) {
    const uint32_t count = ctrl->count[pass];
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride) {
        const float4 o4 = qo[i], d4 = qd[i];
        const V4 ro{o4.x, o4.y, o4.z, o4.w}, rd{d4.x, d4.y, d4.z, d4.w};
        uint32_t tf = hit_tf[i];
        float bt = hit_t[i];
        bool have = tf != 0u;
        for (uint32_t k = 0; k < sc.nspheres; k++) {
            const float4 s0 = sc.spheres[2 * k];
            const V4 oc = vsub(ro, mk(s0.x, s0.y, s0.z));
            const float b = vdot(oc, rd);
            const float c = vlen2(oc) - s0.w * s0.w;
            const float disc = b * b - c;
            if (!(disc >= 0.f)) continue;
            const float sq = sqrtf(disc);
            const float t0 = (0.f - b) - sq, t1 = (0.f - b) + sq;
            float t; uint32_t face;
            if (t0 >= 0.f) { t = t0; face = 0u; }
            else if (t1 >= 0.f) { t = t1; face = 1u; }
            else continue;
            if (!have || t < bt) { bt = t; tf = (sc.ntris + k) | (face << 30); have = true; }
        }
        hit_tf[i] = tf;
        hit_t[i] = bt;
    }
}

// Explicit-ray entry (rtmi_trace): queue = the caller's rays
__global__ void k_set_count(DCtrl* ctrl, uint32_t n) { ctrl->count[0] = n; }

// ---------------------------------------------------------------- host side of the ABI
static thread_local std::string g_err;
static int fail(int code, const std::string& msg) { g_err = msg; return code; }

// HIP status -> ABI status: out of memory, "no device visible" and every other runtime failure are told apart
static int hip_code(hipError_t e) {
    // the failure is reported through the ABI's own channel (status + rtmi_last_error); what the runtime keeps pending for
    // the thread's next hipGetLastError() is dropped, so that the CALLER's next HIP call (PyTorch polls after every
    // operation) does not inherit this library's error
    (void)hipGetLastError();
    if (e == hipErrorOutOfMemory) return RTMI_ERR_OOM;
    if (e == hipErrorNoDevice || e == hipErrorInvalidDevice) return RTMI_ERR_NO_DEVICE;
    return RTMI_ERR_DEVICE;
}

#define HIPCHK(expr)                                                                                   \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess) return fail(hip_code(e_), std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

// No C++ exception crosses the ABI: bodies that allocate host memory run inside this guard.
#define RTMI_GUARD_BEGIN try {
#define RTMI_GUARD_END                                                                                 \
    } catch (const std::bad_alloc&) { return fail(RTMI_ERR_OOM, "host allocation failed");             \
    } catch (const std::exception& ex_) { return fail(RTMI_ERR_INVALID, std::string("internal error: ") + ex_.what()); \
    } catch (...) { return fail(RTMI_ERR_INVALID, "internal error"); }

template <typename T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    hipError_t ensure(size_t want) {
        if (want <= n) return hipSuccess;
        if (p) (void)hipFree(p);
        p = nullptr; n = 0;
        hipError_t e = hipMalloc((void**)&p, want * sizeof(T));
        if (e == hipSuccess) n = want;
        return e;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; n = 0; }
};

}  // namespace rtmi

using namespace rtmi;

// Per-stream workspace of one batch (queues, hit records, surface stacks, sample colours, control block).
struct Work {
    size_t cap = 0;
    uint32_t cap_depth = 0;
    DevBuf<float4> qo[2], qd[2], scol;
    DevBuf<uint32_t> qpath[2], hit_tf;
    DevBuf<float> hit_t;
    // hybrid passes (hybrid.hpp): the fallback list of the pass in flight, one entry per hit record, and the scratch hit
    // records a counting launch runs the hybrid into (allocated by the first such launch)
    DevBuf<uint32_t> fb, ref_tf;
    DevBuf<float> ref_t;
    DevBuf<uint16_t> mstack;
    DevBuf<float4> cstack;  // the colour stack of the k_shade*_tex kernels: allocated only for calls on a textured scene
    DevBuf<DCtrl> ctrl;
    // slow path (SlowQ): its queue, the side stream its consumer launches run on, "producer k done" / "slow path done" events
    DevBuf<float4> sqo, sqd;
    DevBuf<uint32_t> sqpath, sqbounce;
    hipStream_t sstream = nullptr;
    std::vector<hipEvent_t> sev;
    hipEvent_t sdone = nullptr, sgo = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};
    std::vector<hipEvent_t> pass_ev;  // start/stop of the trace kernel of every pass
    void release() {
        for (int k = 0; k < 2; k++) { qo[k].release(); qd[k].release(); qpath[k].release(); }
        scol.release(); hit_tf.release(); hit_t.release(); fb.release(); ref_tf.release(); ref_t.release(); mstack.release(); cstack.release(); ctrl.release();
        for (int k = 0; k < 2; k++) if (ev[k]) { (void)hipEventDestroy(ev[k]); ev[k] = nullptr; }
        for (hipEvent_t e : pass_ev) (void)hipEventDestroy(e);
        pass_ev.clear();
        sqo.release(); sqd.release(); sqpath.release(); sqbounce.release();
        for (hipEvent_t e : sev) (void)hipEventDestroy(e);
        sev.clear();
        if (sdone) { (void)hipEventDestroy(sdone); sdone = nullptr; }
        if (sgo) { (void)hipEventDestroy(sgo); sgo = nullptr; }
        if (sstream) { (void)hipStreamDestroy(sstream); sstream = nullptr; }
        cap = 0; cap_depth = 0;
    }
};

struct rtmi_scene {
    int device = 0;
    uint32_t options = 0;
    DScene d{};
    DevBuf<DNode> nodes;
    DevBuf<uint32_t> refs;
    DevBuf<float4> tplane, tedge, mats, spheres;
    std::vector<float4> hmats;  // the triangles' surface table (host copy): sphere surfaces are appended to it
    // a triangle / a triangle or a sphere is RTMI_DIELECTRIC: such a scene renders on the per-pass pipeline with k_shade*_glass
    bool tris_dielectric = false, has_dielectric = false;
    // rtmi_scene_set_environment / rtmi_scene_set_sky: the table (one float4 per texel) and what the k_shade*_env kernels get of
    // it.  A scene with one renders on the per-pass pipeline with those kernels, with or without glass.
    DevBuf<float4> env;
    EnvTab envtab{};
    bool has_env = false;
    // rtmi_render_envlight* / rtmi_scene_get_env_sampler: the sampler table of the environment (EnvSampler, envlight.hpp), built on
    // the first call that needs it (ensure_env_sampler) and dropped by whatever sets, replaces or clears the environment (env_set)
    DevBuf<uint32_t> envq, envex, envq_max;
    DevBuf<unsigned long long> envrows, envrowsum;
    EnvSampler envsamp{};
    bool envsamp_ok = false;
    // rtmi_scene_set_emitters: the lamps' triangles in triangle order and their corners (host copies, 9 floats per lamp).
    // rtmi_render_emissive* / rtmi_scene_get_emitter_sampler: the lamps' tables (EmTab, emissive.hpp), built on the first call that
    // needs them (ensure_emitters) and dropped by whatever sets or clears the marks.  No other call reads any of it.
    std::vector<uint32_t> em_tris;
    std::vector<float> em_corners;
    DevBuf<uint32_t> em_idx, em_list, em_q, em_max;
    DevBuf<float4> em_lamp, em_c;
    DevBuf<unsigned long long> em_cum;
    EmTab emtab{};
    bool emtab_ok = false;
    // rtmi_scene_set_normals: six float4 per triangle (SmoothTab, shade.hpp).  A scene with them renders on the per-pass pipeline
    // with the k_shade*_smooth kernels, which also know glass and the environment, and k_features_smooth.
    DevBuf<float4> smooth;
    SmoothTab smoothtab{};
    bool has_normals = false;
    // rtmi_scene_set_textures: five float4 per triangle, one uint4 per image and the texels of all images (TexTab, shade.hpp).  A
    // scene with them renders on the per-pass pipeline with the k_shade*_tex kernels, which also know glass, the environment and
    // vertex normals, and k_features_tex.
    DevBuf<float4> textri, texels;
    DevBuf<uint4> texhdr;
    TexTab textab{};
    uint32_t ntex = 0;
    bool has_tex = false;
    // rtmi_scene_set_normal_maps: one float4 per triangle (NmapTab, shade.hpp); the maps' texels are images of `texels`.  A scene
    // with them renders with the k_shade*_nmap kernels, which know everything the _tex ones do, and k_features_nmap.
    DevBuf<float4> nmaptri;
    NmapTab nmaptab{};
    bool has_nmap = false;
    std::vector<rtmi_triangle_t> htris;  // the records (host copy): the BVH is built from them
    DevBuf<uint4> fnodes, oblocks, ocull;  // (fnodes: the node records, then the node cull records)
    DevBuf<uint32_t> wlinks, cert;
    std::vector<uint32_t> leaf_box;  // OctForm::leafbox: leaf ids of k_trace_record -> box index
    // rtmi_trace_records / rtmi_primary_records: per-ray counters, leaf-list offsets and leaf ids of the last call
    DevBuf<uint32_t> rec_cnt, rec_ids;
    DevBuf<unsigned long long> rec_first;
    // RTMI_OPT_BVH: SAH BVH over the triangles' bounding spheres (bvh_fast.hpp)
    DevBuf<float4> bnodes;
    DevBuf<uint4> bleaves;
    uint32_t bvh_root = 0;
    size_t bvh_lds = 0;
    int bvh_blocks_per_cu = 8;
    bool bvh_ok = false;
    bool root_is_leaf = false; // build_trivial_bounding_box: one list for every ray -> k_trace_linear
    bool octree = false;       // the tree passed the exact-octree check
    std::string why_generic;   // reason when it did not
    int oct_blocks_per_cu = 8;   // what fits (occupancy query)
    uint32_t active_streams = 1; // sub-tiles of the render call in flight: their persistent kernels share the CUs
    size_t oct_lds = 0;
    // A tile is rendered as up to two interleaved sub-tiles, each with its own workspace on its own internal
    // stream, so that the small deep bounce passes of one overlap the bulk of the other.
    Work w[RTMI_MAX_STREAMS];
    hipStream_t istream[RTMI_MAX_STREAMS] = {};
    hipEvent_t fork_ev = nullptr, end_ev = nullptr, join_ev[RTMI_MAX_STREAMS] = {};
    DevBuf<float4> tile;
    DevBuf<float4> acc;              // rtmi_render_samples: the running per-pixel sums of the host variant
    DevBuf<float4> asq;              // rtmi_render_adaptive: the per-pixel sums of squares of the host variant
    DevBuf<uint32_t> acnt;           // rtmi_render_adaptive: the per-pixel sample counts of the host variant
    DevBuf<uint32_t> alist[2], ablk; // rtmi_render_adaptive*: active-pixel lists (ping-pong), per-block counts / offsets + total
    // rtmi_render_views*: the view table (grows only), the host copy it is uploaded from and the event recorded behind that
    // upload.  The next views call waits for the event before it rewrites the host copy, also when the call that uploaded
    // it failed before its final synchronisation.
    DevBuf<VCam> vcams;
    std::vector<VCam> hvcams;
    hipEvent_t vcams_ev = nullptr;
    DevBuf<uint8_t> qbytes;
    // rtmi_denoise*: the ping-pong image of calls of more than one iteration (grows only), and the four images (colour,
    // albedo, normal, result) of the host variants.  No render call reads or writes them.
    DevBuf<float4> dn_scratch, dn_host;
    uint32_t dn_lds_max_step = DN_LDS_MAX_STEP;  // tap spacings up to this one stage through LDS (RTMI_DENOISE_LDS_STEP=0|1|2)
    // rtmi_denoise_var*: one colour and two variance ping-pong images (grows only); the images of the host variants and of
    // rtmi_render_adaptive_denoised, and the latter's count map.  No render call and no rtmi_denoise call reads or writes them.
    DevBuf<float4> dnv_scratch, dnv_host;
    DevBuf<uint32_t> dnv_cnt;
    uint32_t dnv_lds_max_step = DN_LDS_MAX_STEP;  // as dn_lds_max_step, for the variance-guided filter (RTMI_DENOISE_VAR_LDS_STEP=0|1|2)
    DevBuf<float> occ_tmax;          // rtmi_occluded (host variant): the limits and the answers on the device
    DevBuf<uint8_t> occ_out;
    // rtmi_render_ao*: per stream, the AO ray queue of a batch (origins, directions, limits), each path's first queue entry
    // and the answer bytes (grow only); the image of the host variant.  No other call reads or writes them.
    struct AoBuf {
        DevBuf<float4> qo, qd;
        DevBuf<float> tmax;
        DevBuf<uint32_t> slot;
        DevBuf<uint8_t> occ;
        void release() { qo.release(); qd.release(); tmax.release(); slot.release(); occ.release(); }
    } ao[RTMI_MAX_STREAMS];
    DevBuf<float> ao_out;
    // rtmi_render_light*: per stream, the shadow-ray queue of a batch (origins, directions, limits, n . dir of the live rays),
    // each candidate's queue entry and the answer bytes (grow only); the two planes of the host variant.  No other call reads
    // or writes them.
    struct LightBuf {
        DevBuf<float4> qo, qd;
        DevBuf<float> tmax, c;
        DevBuf<uint32_t> slot;
        DevBuf<uint8_t> occ;
        void release() { qo.release(); qd.release(); tmax.release(); c.release(); slot.release(); occ.release(); }
    } light[RTMI_MAX_STREAMS];
    DevBuf<float> light_out;
    // rtmi_render_preview*: per stream, the one secondary-ray queue of a batch (origins, directions, limits, n . dir of the
    // lights' live rays, the answer bytes), each path's first AO entry, each light candidate's entry and each path's albedo (grow
    // only); the seven outputs of the host variant.  No other call reads or writes them.
    struct PreviewBuf {
        DevBuf<float4> qo, qd, alb;
        DevBuf<float> tmax, c;
        DevBuf<uint32_t> aslot, lslot;
        DevBuf<uint8_t> occ;
        void release() { qo.release(); qd.release(); alb.release(); tmax.release(); c.release(); aslot.release(); lslot.release(); occ.release(); }
    } pv[RTMI_MAX_STREAMS];
    DevBuf<float4> pv_out4;
    DevBuf<float> pv_out1;
    // rtmi_render_shadowed*: per stream, the shadow-ray queue of ONE pass of a batch (origins, directions, limits), each path
    // queue entry's shadow queue entry, the answer bytes and each path's mask of shadowed levels (grow only), and what the
    // walks need beside the path queues: `walk` holds the second control block (shadow queue j counts in count[j + 1]), hit
    // records of its own for scenes whose walk is a closest-hit launch, and the walks' event pairs; nothing else of it is
    // allocated.  No other call reads or writes them.
    struct ShadowBuf {
        DevBuf<float4> qo, qd;
        DevBuf<float> tmax;
        DevBuf<uint32_t> slot, mask;
        DevBuf<uint8_t> occ;
        // rtmi_render_envlight*, which runs the same pass structure: L * wgt per shadow queue entry, the direct stack
        // ([pass][path]) and each path's balance weight.  Allocated by that call only.
        DevBuf<float4> lw, dstack;
        DevBuf<float> wb;
        // rtmi_render_lit*, the same pass structure with up to nlights shadow rays per path and pass: qo, qd, tmax, lw and occ then
        // hold paths * nlights entries, slot paths * nlights words ([light][path]); dstack as above.  Sized by that call only.
        // rtmi_render_rays_lit* and rtmi_bake_lit* run the same passes on stream 0's buffers (ensure_lit_rays sizes them); the bake's
        // element candidates use them before its gather paths do, their shadow queue counted in walk's count[RTMI_MAX_PASSES].
        Work walk;
        void release() { qo.release(); qd.release(); tmax.release(); slot.release(); mask.release(); occ.release(); lw.release(); dstack.release(); wb.release(); walk.release(); }
    } shadow[RTMI_MAX_STREAMS];
    DevBuf<uint8_t> mstage, mframe;  // rtmi_render_frame_multi, root scene: received bands / the frame
    hipStream_t mstream = nullptr;   // rtmi_render_frame_multi: this scene's band stream
    std::vector<ncclComm_t> comms;   // root scene, RTMI_FRAME_RCCL: one communicator per scene of the last device list
    std::vector<int> comm_devices;
    int peer_root = -1;              // root device the peer-access state below refers to (-1: not asked yet)
    int peer_ok = 0;                 // 1 = this device reaches peer_root directly (enabled once), 0 = the runtime refused
    std::string peer_msg;            // the runtime's reason when it refused
    int num_cu = 256;
    int trace_block = 256;
    size_t trace_lds = 0;
    // tuning knobs, read from the environment ONCE at scene creation (getenv is not free and not thread-safe
    // against setenv): waves per CU of the octree kernel, refill thresholds, XCD mode, streams, batch size
    rtmi_tuning_t tune{};
    bool verbose = false;
    int vote[4] = {3, 2, 3, 2};  // SELECT : LEAF vote weights of the walk, primary rays / bounce rays (experiments: RTMI_VOTE="a,b,c,d")
    int lit_from_hits = 1;       // rtmi_render_lit* walks its shadow rays with the closest-hit launch on an octree (RTMI_LIT_FROM_HITS=0: the any-hit kernel, for comparison)
    int occl_from_hits = 0;      // rtmi_occluded* runs the closest-hit launch + k_occl_from_hits everywhere (RTMI_OCCLUDED_ANYHIT=0, for comparison)
    int block_cull = 1;          // k_trace_oct skips reference blocks by their cull records (RTMI_BLOCK_CULL=0: off, no records)
    int block_cull_n = 4;        // cull records a LEAF step of k_trace_oct reads, 2..4 (experiments: RTMI_BLOCK_CULL_N)
    CertStats cert_stats{};      // the sign certificate's table (rtmi_debug_cert_stats)
    int hybrid = 1;              // bounce passes propose hits with the BVH and confirm them against the octree (RTMI_HYBRID=0: off; hybrid.hpp)
    float hybrid_omax = 0.f;     // the largest |o|_1 of a ray a hybrid pass proposes a hit for (hybrid_origin_max, hybrid.hpp)
    uint32_t nfn = 0;            // inner records of the octree form (the bound of k_oct_verify's descent)
    int node_cull = 1;           // k_trace_oct skips subtrees by their node cull records (RTMI_NODE_CULL=0: off, no records)
    uint64_t node_cull_records = 0;  // node cull records built (0: none) and the seconds that took (rtmi_debug_node_cull_stats)
    double node_cull_seconds = 0.0;
    int primary_node_cull = 1;   // k_path_primary skips subtrees by the node cull records too (RTMI_PRIMARY_NODE_CULL=0: off)
    int packet_cull = 1;         // k_path_primary culls leaf triangles per pixel packet (RTMI_PACKET_CULL=0: off, for comparison)
    // k_path_primary traces the mirror reflections of its primary rays itself when a wave has at least this many
    // (RTMI_MIRROR_INPLACE=n; 0: off, everything above 64: never)
    int mirror_inplace = 32;
    unsigned long long vprev[RTMI_MAX_STREAMS][13] = {};  // verbose per-pass deltas (per handle: no shared statics)
};

// RCCL for RTMI_FRAME_RCCL, loaded on first use: no link-time dependency, and in a process that already holds PyTorch's
// RCCL (same SONAME librccl.so.1) dlopen hands back that copy instead of mapping a second one.
struct Rccl {
    void* lib = nullptr;
    decltype(&ncclCommInitAll) CommInitAll = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclGroupStart) GroupStart = nullptr;
    decltype(&ncclGroupEnd) GroupEnd = nullptr;
    decltype(&ncclGather) Gather = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
    bool ok = false;
};
static Rccl* rccl_api() {
    static Rccl api;
    static std::once_flag once;
    std::call_once(once, [] {
        for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
            api.lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
            if (api.lib) break;
        }
        if (!api.lib) return;
        api.CommInitAll = (decltype(api.CommInitAll))dlsym(api.lib, "ncclCommInitAll");
        api.CommDestroy = (decltype(api.CommDestroy))dlsym(api.lib, "ncclCommDestroy");
        api.GroupStart = (decltype(api.GroupStart))dlsym(api.lib, "ncclGroupStart");
        api.GroupEnd = (decltype(api.GroupEnd))dlsym(api.lib, "ncclGroupEnd");
        api.Gather = (decltype(api.Gather))dlsym(api.lib, "ncclGather");
        api.GetErrorString = (decltype(api.GetErrorString))dlsym(api.lib, "ncclGetErrorString");
        api.ok = api.CommInitAll && api.CommDestroy && api.GroupStart && api.GroupEnd && api.Gather && api.GetErrorString;
    });
    return api.ok ? &api : nullptr;
}

// Build the BVH (bvh_fast.hpp) of the opt-in fast mode and of the hybrid passes from the scene's triangle records.
static int upload_bvh(rtmi_scene* s) {
    s->bvh_ok = false;
    BvhBuild bb;
    if (s->htris.size() >= (1u << 26) || !bvh_build(s->htris.data(), s->htris.size(), bb)) return RTMI_OK;  // no BVH: RTMI_OPT_BVH is then ignored, no hybrid passes
    if (bb.wide.empty()) bb.wide.resize(8, make_float4(0.f, 0.f, 0.f, 0.f));
    auto up = [&](auto& buf, const auto& host) -> hipError_t {
        hipError_t e = buf.ensure(std::max<size_t>(host.size(), 1));
        if (e != hipSuccess || host.empty()) return e;
        return hipMemcpy(buf.p, host.data(), host.size() * sizeof(host[0]), hipMemcpyHostToDevice);
    };
    hipError_t be = up(s->bnodes, bb.wide);
    if (be == hipSuccess) be = up(s->bleaves, bb.leaves);
    if (be != hipSuccess) return fail(hip_code(be), std::string("scene upload (BVH): ") + hipGetErrorString(be));
    s->bvh_root = bb.root_link;
    {
        float m = FLT_MAX;  // the smallest |c|_1 + r over the triangles (the sentinel aside)
        for (size_t i = 1; i < s->htris.size(); i++) {
            const rtmi_triangle_t& t = s->htris[i];
            m = std::min(m, ((std::fabs(t.incenter[0]) + std::fabs(t.incenter[1])) + std::fabs(t.incenter[2])) + std::sqrt(t.bounding_r2));
        }
        s->hybrid_omax = hybrid_origin_max(m);
    }
    s->bvh_lds = (size_t)(3 * bb.depth + 2) * 64 * 4;  // an INNER step leaves at most 3 links waiting per level
    int nb = 0;
    if (s->bvh_lds <= 64 * 1024 &&
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_trace_bvh<false>, 64, s->bvh_lds) == hipSuccess && nb > 0) {
        s->bvh_blocks_per_cu = nb;
        s->bvh_ok = true;
    } else (void)hipGetLastError();
    return RTMI_OK;
}

static size_t env_size(const char* name, size_t dflt) {
    const char* s = getenv(name);
    if (!s || !*s) return dflt;
    char* end = nullptr;
    unsigned long long v = strtoull(s, &end, 10);
    return (end && *end == '\0' && (v > 0 || dflt == 0)) ? (size_t)v : dflt;
}

// Checks the flattened tree of rtmi_scene_create (every box reachable from an earlier one, 1..8 children after their
// parent, leaf ranges and triangle indices in bounds); fills the depth of every box and the largest depth of an inner box.
// Returns "" or what is wrong.
static std::string validate_tree(const rtmi_box_t* boxes, uint64_t nboxes, const uint32_t* tri_refs, uint64_t nrefs, uint64_t ntris,
                                 std::vector<uint32_t>& depth, uint32_t& max_inner_depth) {
    depth.assign(nboxes, 0xFFFFFFFFu);
    depth[0] = 0;
    max_inner_depth = 0;
    for (uint64_t i = 0; i < nboxes; i++) {
        const rtmi_box_t& b = boxes[i];
        if (depth[i] == 0xFFFFFFFFu) return "box " + std::to_string(i) + " is not reachable from an earlier box";
        if (b.is_leaf) {
            if ((uint64_t)b.first + b.count > nrefs) return "leaf triangle range out of bounds";
            for (uint32_t k = 0; k < b.count; k++)
                if (tri_refs[b.first + k] >= ntris) return "triangle index out of range";
        } else {
            // the reference's boxmap has 8 slots (raytrace.rs:929): more children would panic there
            if (b.count < 1 || b.count > 8) return "inner box must have 1..8 children";
            if (b.first <= i || (uint64_t)b.first + b.count > nboxes) return "child range must follow its parent";
            for (uint32_t k = 0; k < b.count; k++) {
                if (depth[b.first + k] != 0xFFFFFFFFu) return "box has two parents";
                depth[b.first + k] = depth[i] + 1;
            }
            max_inner_depth = std::max(max_inner_depth, depth[i]);
        }
    }
    return "";
}

// The exact-octree form of a validated tree (trace_oct.hpp, "Records"): fnodes, oblocks, wlinks.  Host only.
struct OctForm {
    std::vector<uint4> fn;     // 2 records per inner box
    std::vector<uint4> ob;     // reference blocks, each DISTINCT leaf list once
    std::vector<uint32_t> wl;  // explicit block indices of FN_WIDE boxes
    std::vector<uint32_t> leafbox;  // 8 per inner record: box index of its leaf child in each octant (~0u: none); the
                                    // records of k_trace_record name a leaf (record << 3) | octant
    uint64_t nwide = 0;        // FN_WIDE boxes
    std::string why;           // empty: the tree is an exact octree
};

// FNV-1a over a leaf's reference sequence (the dedup table's hash; equality is checked on the whole sequence)
struct RefListHash {
    size_t operator()(const std::vector<uint32_t>& v) const {
        uint64_t h = 1469598103934665603ull;
        for (uint32_t x : v) { h ^= x; h *= 1099511628211ull; }
        return (size_t)h;
    }
};

// Every child must be the builder's octant of its parent, bit for bit (orig + (+-newlen2), newlen2 = len2 / 2,
// raytrace.rs:816-824), stored in octant order.  Inner boxes get a 32-B record (centre, child masks, links); leaves only
// their reference blocks.  Leaves that list the same triangles in the same order share ONE run of blocks (the builder
// lists a triangle in every box its plane crosses, so neighbouring leaves often carry the same list): a list's identity
// is its first block, which is what the walk's one-entry leaf memo compares.  Order matters: the leaf fold takes the
// first of equal hit times, so only identical sequences are shared.
static void build_oct_form(const rtmi_box_t* boxes, uint64_t nboxes, const uint32_t* tri_refs, uint64_t ntris,
                           const std::vector<uint32_t>& depth, OctForm& f) {
    auto fb = [](float v) { uint32_t u; memcpy(&u, &v, 4); return u; };
    std::vector<uint4>& hfn = f.fn;
    std::vector<uint4>& hob = f.ob;
    std::vector<uint32_t>& hwl = f.wl;
    std::string& why = f.why;
    bool ok = !boxes[0].is_leaf;  // a one-leaf tree is the linear list (k_trace_linear)
    if (!ok) why = "the root box is a leaf";
    // record index of every inner box (in box order, root = 0) / first reference block of every leaf
    std::vector<uint32_t> slot(nboxes, 0);
    uint64_t ninner = 0;
    const float root_len2 = boxes[0].len2;
    std::unordered_map<std::vector<uint32_t>, uint32_t, RefListHash> seen;  // leaf list -> its first block
    std::vector<uint32_t> list;
    for (uint64_t i = 0; i < nboxes && ok; i++) {
        const rtmi_box_t& b = boxes[i];
        if (fb(b.len2) != fb(ldexpf(root_len2, -(int)depth[i])) || !(b.len2 > 0.f) || !std::isfinite(b.len2)) { ok = false; why = "box half-length is not root/2^depth"; break; }
        if (b.is_leaf) {
            for (uint32_t k = 0; k < b.count; k++)
                if (tri_refs[b.first + k] == 0) { ok = false; why = "a leaf lists the sentinel triangle 0"; }
            if (!ok) break;
            list.assign(tri_refs + b.first, tri_refs + b.first + b.count);
            auto it = seen.find(list);
            if (it != seen.end()) { slot[i] = it->second | 0x80000000u; continue; }
            if (hob.size() >= (1ull << 31)) { ok = false; why = "more than 2^31 reference blocks"; break; }
            slot[i] = (uint32_t)hob.size() | 0x80000000u;
            seen.emplace(list, (uint32_t)hob.size());
            // blocks of 4 indices; the list ends at the first 0, or after a block whose 4th index carries
            // bit 31 (a full last block: no extra all-zero block, triangle indices are < 2^30)
            for (uint32_t k = 0; k < std::max<uint32_t>(b.count, 1u); k += 4) {
                uint32_t v[4] = {0, 0, 0, 0};
                for (uint32_t j = 0; j < 4; j++)
                    if (k + j < b.count) v[j] = tri_refs[b.first + k + j];
                if (k + 4 == b.count) v[3] |= 0x80000000u;
                hob.push_back(make_uint4(v[0], v[1], v[2], v[3]));
            }
        } else {
            slot[i] = (uint32_t)ninner++;
        }
    }
    if (ok) {
        hfn.assign(2 * ninner, make_uint4(0, 0, 0, 0));
        f.leafbox.assign(8 * ninner, 0xFFFFFFFFu);
        for (uint64_t i = 0; i < nboxes && ok; i++) {
            const rtmi_box_t& b = boxes[i];
            if (b.is_leaf) continue;
            const float h = b.len2 / 2.f;
            uint32_t mask = 0, leafmask = 0, first_block[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            uint32_t base_inner = 0, base_block = 0xFFFFFFFFu;
            bool have_inner = false;
            int prev = -1;
            for (uint32_t k = 0; k < b.count && ok; k++) {
                const rtmi_box_t& c = boxes[b.first + k];
                int oct = 0;
                for (int a = 0; a < 3; a++) {
                    const float lo = b.orig[a] + (-1.f * h), hi = b.orig[a] + h;
                    if (fb(lo) == fb(hi)) { ok = false; why = "degenerate box"; break; }
                    if (fb(c.orig[a]) == fb(hi)) oct |= 1 << a;
                    else if (fb(c.orig[a]) != fb(lo)) { ok = false; why = "child centre is not an octant centre of its parent"; break; }
                }
                if (ok && oct <= prev) { ok = false; why = "children are not in octant order"; }
                prev = oct;
                mask |= 1u << oct;
                // children follow each other in box order, so the inner ones have consecutive records: one base + a
                // popcount.  Leaf children point at shared lists anywhere in `hob`: base = the smallest first block among
                // them + a byte offset per octant (new lists of one box are placed consecutively, in box order)
                if (c.is_leaf) {
                    leafmask |= 1u << oct;
                    f.leafbox[8 * (size_t)slot[i] + oct] = (uint32_t)(b.first + k);
                    first_block[oct & 7] = slot[b.first + k] & 0x7FFFFFFFu;
                    base_block = std::min(base_block, first_block[oct & 7]);
                } else if (!have_inner) { base_inner = slot[b.first + k]; have_inner = true; }
            }
            if (!leafmask) base_block = 0;
            uint32_t w = mask | (leafmask << 8), offlo = 0, offhi = 0, q1y = base_block;
            bool wide = false;
            for (int o = 0; o < 8; o++)
                if ((leafmask >> o) & 1u) wide |= first_block[o] - base_block > 255u;
            if (wide) {
                w |= RTMI_FN_WIDE;
                q1y = (uint32_t)(hwl.size() / 8);
                hwl.insert(hwl.end(), first_block, first_block + 8);
                f.nwide++;
            } else {
                for (int o = 0; o < 8; o++) {
                    const uint32_t off = ((leafmask >> o) & 1u) ? first_block[o] - base_block : 0u;
                    if (o < 4) offlo |= off << (8 * o); else offhi |= off << (8 * (o - 4));
                }
            }
            uint4* rec = &hfn[2 * (size_t)slot[i]];
            rec[0] = make_uint4(fb(b.orig[0]), fb(b.orig[1]), fb(b.orig[2]), w);
            rec[1] = make_uint4(base_inner, q1y, offlo, offhi);
        }
    }
    // k_trace_oct addresses its records with 32-bit byte offsets (ld_off32): 32 B per inner box and per triangle plane
    // record, 64 B per triangle edge record, 16 B per reference block; its stack keeps an inner box's record index in 22 bits
    if (ok && (ninner >= (1ull << 22) || ntris >= (1ull << 26) || hob.size() >= (1ull << 28))) { ok = false; why = "more than 2^22 inner boxes, or an array of the octree form would exceed 4 GiB"; }
    if (!ok) { hfn.clear(); hob.clear(); hwl.clear(); f.leafbox.clear(); f.nwide = 0; }
}

// The block cull records of `nb` reference blocks (trace_oct.hpp, "Block cull").  hp: the plane records
// (incenter.xyz, r2) (norm.xyz, material) of `ntris` triangles.  Boxes in double, rounded outward to f32 / int8.
static void build_block_cull(const uint4* blocks, size_t nb, const float4* hp, uint64_t ntris, std::vector<uint4>& out) {
    auto fb = [](float v) { uint32_t u; memcpy(&u, &v, 4); return u; };
    auto down = [](double v) { float f = (float)v; return (double)f > v ? std::nextafterf(f, -INFINITY) : f; };
    auto up = [](double v) { float f = (float)v; return (double)f < v ? std::nextafterf(f, INFINITY) : f; };
    auto in_range = [](double v) { return std::isfinite(v) && v >= 1e-15 && v <= 1e15; };
    const double K = 1e-5;
    out.assign(2 * nb, make_uint4(0u, 0u, 0u, 0u));
    for (size_t b = 0; b < nb; b++) {
        const uint4 blk = blocks[b];
        const uint32_t ids[4] = {blk.x, blk.y, blk.z, blk.w & 0x7FFFFFFFu};
        double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        int nlo[3] = {127, 127, 127}, nhi[3] = {-127, -127, -127};
        uint32_t flags = (blk.w == 0u || (blk.w >> 31)) ? BC_END : 0u;
        bool any = false;
        for (int k = 0; k < 4; k++) {
            if (ids[k] == 0u) continue;  // padding behind the list's end
            if (ids[k] >= ntris) { flags |= BC_NEVER; continue; }
            any = true;
            const float4 p0 = hp[2 * (size_t)ids[k]], p1 = hp[2 * (size_t)ids[k] + 1];
            const double c[3] = {p0.x, p0.y, p0.z}, n[3] = {p1.x, p1.y, p1.z};
            const double c1 = (std::fabs(c[0]) + std::fabs(c[1])) + std::fabs(c[2]);
            const double nn = std::sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
            if (!in_range(c1) || !in_range(nn) || !in_range((double)p0.w)) { flags |= BC_NEVER; continue; }
            const double rho = std::sqrt((double)p0.w);
            const double pad = rho * (1.0 + K) + K * (c1 + rho);
            for (int a = 0; a < 3; a++) {
                lo[a] = std::min(lo[a], c[a] - pad);
                hi[a] = std::max(hi[a], c[a] + pad);
                const double u = 127.0 * (n[a] / nn);
                nlo[a] = std::min(nlo[a], std::max(-127, (int)std::floor(u - 1e-6)));
                nhi[a] = std::max(nhi[a], std::min(127, (int)std::ceil(u + 1e-6)));
            }
        }
        float flo[3], fhi[3];
        for (int a = 0; a < 3; a++) {
            // no real reference (or none in range): the empty box
            flo[a] = any && !(flags & BC_NEVER) ? down(lo[a]) : FLT_MAX;
            fhi[a] = any && !(flags & BC_NEVER) ? up(hi[a]) : -FLT_MAX;
        }
        auto b8 = [](int v) { return (uint32_t)(uint8_t)(int8_t)v; };
        out[2 * b] = make_uint4(fb(flo[0]), fb(flo[1]), fb(flo[2]), fb(fhi[0]));
        out[2 * b + 1] = make_uint4(fb(fhi[1]), fb(fhi[2]), b8(nlo[0]) | (b8(nlo[1]) << 8) | (b8(nlo[2]) << 16) | (b8(nhi[0]) << 24),
                                    b8(nhi[1]) | (b8(nhi[2]) << 8) | (flags << 16));
    }
}

// The packed 16-B records (trace_oct.hpp, "Packed cull record") from the 32-B ones: bf16 ends, lo toward -inf, hi toward +inf
static void pack_block_cull(const std::vector<uint4>& recs, std::vector<uint4>& out) {
    auto down = [](uint32_t u) -> uint32_t {  // bf16 <= the f32 with bits u
        if (!(u >> 31)) return u >> 16;
        return (u & 0xFFFFu) ? (u >> 16) + 1u : u >> 16;  // negative: the magnitude grows (up to -inf)
    };
    auto up = [](uint32_t u) -> uint32_t {  // bf16 >= the f32 with bits u
        if (u >> 31) return u >> 16;
        return (u & 0xFFFFu) ? (u >> 16) + 1u : u >> 16;
    };
    const size_t nb = recs.size() / 2;
    out.assign(nb, make_uint4(0u, 0u, 0u, 0u));
    for (size_t b = 0; b < nb; b++) {
        const uint4 c0 = recs[2 * b], c1 = recs[2 * b + 1];
        const uint32_t flags = c1.w >> 16;
        uint32_t lo[3] = {down(c0.x), down(c0.y), down(c0.z)}, hi[3] = {up(c0.w), up(c1.x), up(c1.y)};
        if (flags & BC_NEVER)
            for (int a = 0; a < 3; a++) { lo[a] = 0xFF80u; hi[a] = 0x7F80u; }  // [-inf, +inf]: no half-line misses it
        out[b] = make_uint4(lo[0] | (lo[1] << 16), lo[2] | (hi[0] << 16), hi[1] | (hi[2] << 16), flags);
    }
}

// The node cull records (trace_oct.hpp, "Node cull"): per inner record of `fn` (2 uint4 each) the union of the
// f32 boxes of `recs` (build_block_cull: 2 uint4 per block of the `nb` blocks) over every block of every leaf list below it,
// as a 32-B record of the same form (no normal box) -- pack_block_cull then rounds it outward like a block's.  A never-cull
// block below makes the node never-cull (packed: [-inf, +inf]); a subtree without a real reference keeps the empty box.
// Bottom-up: the inner children of a record have larger record indices (children follow their parent in box order).  A
// shared list is walked once per leaf that carries it.
static void build_node_cull(const std::vector<uint4>& fn, const std::vector<uint32_t>& wl, const std::vector<uint4>& recs, size_t nb,
                            std::vector<uint4>& out) {
    auto fb = [](float v) { uint32_t u; memcpy(&u, &v, 4); return u; };
    auto bf = [](uint32_t u) { float v; memcpy(&v, &u, 4); return v; };
    const size_t nrec = fn.size() / 2;
    struct Box { float lo[3], hi[3]; bool never; };
    std::vector<Box> box(nrec);
    for (size_t r = nrec; r-- > 0;) {
        const uint4 q0 = fn[2 * r], q1 = fn[2 * r + 1];
        const uint32_t present = q0.w & 0xFFu, leafmask = (q0.w >> 8) & 0xFFu;
        Box b{{FLT_MAX, FLT_MAX, FLT_MAX}, {-FLT_MAX, -FLT_MAX, -FLT_MAX}, false};
        auto join = [&](const float* lo, const float* hi) {
            for (int a = 0; a < 3; a++) { b.lo[a] = std::min(b.lo[a], lo[a]); b.hi[a] = std::max(b.hi[a], hi[a]); }
        };
        for (uint32_t oct = 0; oct < 8; oct++) {
            const uint32_t bit = 1u << oct;
            if (!(present & bit)) continue;
            if (leafmask & bit) {
                // the leaf's first block as oct_walk finds it, then its blocks up to the one that ends the list
                size_t k = (q0.w & RTMI_FN_WIDE) ? wl[(size_t)q1.y * 8u + oct] : q1.y + (((oct < 4u ? q1.z : q1.w) >> ((oct & 3u) * 8u)) & 0xFFu);
                for (; k < nb; k++) {
                    const uint4 c0 = recs[2 * k], c1 = recs[2 * k + 1];
                    const uint32_t flags = c1.w >> 16;
                    if (flags & BC_NEVER) b.never = true;
                    const float lo[3] = {bf(c0.x), bf(c0.y), bf(c0.z)}, hi[3] = {bf(c0.w), bf(c1.x), bf(c1.y)};
                    join(lo, hi);
                    if (flags & BC_END) break;
                }
            } else {
                const size_t c = q1.x + (size_t)__builtin_popcount((present & ~leafmask) & (bit - 1u));
                if (c <= r || c >= nrec) { b.never = true; continue; }  // (cannot happen in a form build_oct_form made)
                b.never |= box[c].never;
                join(box[c].lo, box[c].hi);
            }
        }
        box[r] = b;
    }
    out.assign(2 * nrec, make_uint4(0u, 0u, 0u, 0u));
    for (size_t r = 0; r < nrec; r++) {
        const Box& b = box[r];
        out[2 * r] = make_uint4(fb(b.lo[0]), fb(b.lo[1]), fb(b.lo[2]), fb(b.hi[0]));
        out[2 * r + 1] = make_uint4(fb(b.hi[1]), fb(b.hi[2]), 0u, (b.never ? BC_NEVER : 0u) << 16);
    }
}

// The direction table of the sign certificate (trace_oct.hpp, ray_sign_certified).  hp: the plane records of
// `ntris` triangles.  The distinct normals (bitwise; those with |n| outside [1e-15, 1e15] make their block never-cull and are
// left out) are binned by the cell of d / d_major = (1, a, b): cell (face, i, j) covers a in [-1 + 2 i / G, -1 + 2 (i + 1) / G]
// and b likewise, both grown by CELL_PAD (the kernel finds the cell in f32: its a, b and the product with G / 2 are off by
// less than 1e-6).  A unit normal u is listed when |u_m + u_a a + u_b b| <= 3.001 tau somewhere in the grown cell -- |d|_1 <=
// 3.001 there --, evaluated row by row in double.  False: more than `max_normals` distinct normals, or more than 2^32 list entries.
static bool build_ray_cert(const float4* hp, uint64_t ntris, uint32_t G, size_t max_normals, std::vector<uint32_t>& out, CertStats& st) {
    const auto t0 = std::chrono::steady_clock::now();
    const double CELL_PAD = 1e-5, T = 3.001 * CERT_TAU;
    struct Key { uint32_t x, y, z; bool operator<(const Key& o) const { return std::tie(x, y, z) < std::tie(o.x, o.y, o.z); } };
    std::map<Key, uint32_t> seen;
    std::vector<float4> nrm;
    for (uint64_t i = 1; i < ntris; i++) {
        const float4 p1 = hp[2 * i + 1];
        const double nn = std::sqrt(((double)p1.x * p1.x + (double)p1.y * p1.y) + (double)p1.z * p1.z);
        if (!(std::isfinite(nn) && nn >= 1e-15 && nn <= 1e15)) continue;
        Key k;
        memcpy(&k.x, &p1.x, 4); memcpy(&k.y, &p1.y, 4); memcpy(&k.z, &p1.z, 4);
        if (seen.emplace(k, (uint32_t)nrm.size()).second) nrm.push_back(make_float4(p1.x, p1.y, p1.z, (fabsf(p1.x) + fabsf(p1.y)) + fabsf(p1.z)));
    }
    st = CertStats{0u, (uint32_t)nrm.size(), 0u, 0u, 0u, 0.0};
    if (nrm.size() > max_normals) return false;
    const size_t ncell = (size_t)3 * G * G;
    std::vector<uint32_t> cnt(ncell + 1, 0u);
    // the columns [j0, j1] of row i on `face` that list normal u (j0 > j1: none)
    auto row = [&](const double* u, int face, uint32_t i, int& j0, int& j1) {
        const double um = u[face], ua = u[(face + 1) % 3], ub = u[(face + 2) % 3];
        const double a0 = -1.0 + 2.0 * i / G - CELL_PAD, a1 = -1.0 + 2.0 * (i + 1) / G + CELL_PAD;
        const double p0 = std::min(ua * a0, ua * a1), p1 = std::max(ua * a0, ua * a1);
        const double q0 = -T - um - p1, q1 = T - um - p0;  // u_b b must lie in [q0, q1]
        j0 = 0; j1 = (int)G - 1;
        if (ub == 0.0) { if (!(q0 <= 0.0 && 0.0 <= q1)) j1 = -1; return; }
        double b0 = std::min(q0 / ub, q1 / ub), b1 = std::max(q0 / ub, q1 / ub);
        if (b1 < -1.0 - CELL_PAD || b0 > 1.0 + CELL_PAD) { j1 = -1; return; }
        b0 = std::max(b0, -2.0); b1 = std::min(b1, 2.0);
        // (2 CELL_PAD: the cell's own growth and the roundings here, which are below 1e-13)
        j0 = std::max(0, (int)std::floor((b0 - 2.0 * CELL_PAD + 1.0) * 0.5 * G));
        j1 = std::min((int)G - 1, (int)std::floor((b1 + 2.0 * CELL_PAD + 1.0) * 0.5 * G));
    };
    std::vector<std::array<double, 3>> un(nrm.size());
    for (size_t k = 0; k < nrm.size(); k++) {
        const double x = nrm[k].x, y = nrm[k].y, z = nrm[k].z, nn = std::sqrt((x * x + y * y) + z * z);
        un[k] = {x / nn, y / nn, z / nn};
    }
    uint64_t total = 0;
    for (int fill = 0; fill < 2; fill++) {
        if (fill) {
            if (total >= (1ull << 32)) return false;
            uint32_t run = 0;
            for (size_t c = 0; c <= ncell; c++) { const uint32_t n = cnt[c]; cnt[c] = run; run += n; }
        }
        const bool wide = nrm.size() > 65536;
        const size_t idx_words = wide ? total : (total + 1) / 2;
        const size_t idx0 = 4 + ncell + 1, nrm0 = (idx0 + idx_words + 3) & ~(size_t)3;
        std::vector<uint32_t> cur;
        if (fill) {
            out.assign(nrm0 + 4 * nrm.size(), 0u);
            out[0] = G; out[1] = (uint32_t)idx0; out[2] = (uint32_t)nrm0; out[3] = wide ? 1u : 0u;
            memcpy(&out[4], cnt.data(), (ncell + 1) * 4);
            if (!nrm.empty()) memcpy(&out[nrm0], nrm.data(), nrm.size() * sizeof(float4));
            cur.assign(cnt.begin(), cnt.end() - 1);
        }
        uint16_t* const i16 = fill ? reinterpret_cast<uint16_t*>(&out[idx0]) : nullptr;
        for (size_t k = 0; k < nrm.size(); k++)
            for (int face = 0; face < 3; face++)
                for (uint32_t i = 0; i < G; i++) {
                    int j0, j1;
                    row(un[k].data(), face, i, j0, j1);
                    for (int j = j0; j <= j1; j++) {
                        const size_t c = ((size_t)face * G + i) * G + (size_t)j;
                        if (!fill) { cnt[c]++; total++; }
                        else if (wide) out[idx0 + cur[c]++] = (uint32_t)k;
                        else i16[cur[c]++] = (uint16_t)k;
                    }
                }
    }
    uint32_t longest = 0;
    for (size_t c = 0; c < ncell; c++) longest = std::max(longest, cnt[c + 1] - cnt[c]);
    st = CertStats{G, (uint32_t)nrm.size(), total, longest, (uint64_t)out.size() * 4,
                   std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count()};
    return true;
}

// LDS of an octree-walk launch: the counting build keeps 2 more memo words per lane (the list's plane and edge tests)
// and every launch room for the LDS header of k_path_primary (trace_oct.hpp, PrimHdr: its packet and pass-2 queue)
static_assert(sizeof(PrimHdr) % 16 == 0 && sizeof(PrimHdr) <= 112, "header slot in LDS");
static size_t oct_launch_lds(const rtmi_scene* s, bool count) { return s->oct_lds + (count ? 2 * 4 * 64 : 0) + 112; }

extern "C" {

const char* rtmi_last_error(void) { return g_err.c_str(); }

int rtmi_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int rtmi_scene_create(const rtmi_triangle_t* tris, uint64_t ntris, const rtmi_box_t* boxes, uint64_t nboxes,
                      const uint32_t* tri_refs, uint64_t nrefs, int device, rtmi_scene_t** out) {
    if (!out) return fail(RTMI_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!tris || ntris < 1) return fail(RTMI_ERR_INVALID, "need at least the sentinel triangle (index 0)");
    if (!boxes || nboxes < 1) return fail(RTMI_ERR_INVALID, "need at least the root box");
    if (nrefs > 0 && !tri_refs) return fail(RTMI_ERR_INVALID, "tri_refs is NULL");
    if (ntris >= (1ull << 30)) return fail(RTMI_ERR_UNSUPPORTED, "more than 2^30 triangles");
    if (nboxes >= (1ull << 32) || nrefs >= (1ull << 32)) return fail(RTMI_ERR_UNSUPPORTED, "tree too large for 32-bit indices");

    RTMI_GUARD_BEGIN
    // ---- validate the tree, compute inner depth (levels of the LDS stack)
    std::vector<uint32_t> depth;
    uint32_t max_inner_depth = 0;
    {
        const std::string bad = validate_tree(boxes, nboxes, tri_refs, nrefs, ntris, depth, max_inner_depth);
        if (!bad.empty()) return fail(RTMI_ERR_INVALID, bad);
    }
    const uint32_t levels = std::max<uint32_t>(1u, max_inner_depth);
    int block = 256;
    if ((size_t)levels * 16 * 256 > 40 * 1024) block = 64;
    if ((size_t)levels * 16 * block > 64 * 1024) return fail(RTMI_ERR_UNSUPPORTED, "octree deeper than the LDS stack allows");

    // ---- device records
    std::vector<DNode> hn(nboxes);
    for (uint64_t i = 0; i < nboxes; i++) {
        const rtmi_box_t& b = boxes[i];
        hn[i] = DNode{b.orig[0], b.orig[1], b.orig[2], b.len2, b.first, b.count, b.is_leaf ? 1u : 0u, 0u};
    }
    // ---- exact-octree form (trace_oct.hpp); empty when the tree is not one, `why` says why
    OctForm of;
    build_oct_form(boxes, nboxes, tri_refs, ntris, depth, of);
    std::vector<uint4>& hfn = of.fn;
    std::vector<uint4>& hob = of.ob;
    std::vector<uint32_t>& hwl = of.wl;
    std::string& why = of.why;

    std::map<std::tuple<uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t>, uint32_t> matmap;
    std::vector<float4> hm, hp(2 * ntris), he(4 * ntris);
    bool has_dielectric = false;
    auto bits = [](float f) { uint32_t u; memcpy(&u, &f, 4); return u; };
    auto fbits = [](uint32_t u) { float f; memcpy(&f, &u, 4); return f; };
    for (uint64_t i = 0; i < ntris; i++) {
        const rtmi_triangle_t& t = tris[i];
        if (t.surface_kind > RTMI_DIELECTRIC) return fail(RTMI_ERR_INVALID, "unknown surface kind");
        if (t.surface_kind == RTMI_DIELECTRIC) {  // scattering carries the index of refraction
            if (!(std::isfinite(t.scattering) && t.scattering > 0.f))
                return fail(RTMI_ERR_INVALID, "triangle " + std::to_string(i) + ": a dielectric's index of refraction (scattering) must be finite and > 0");
            has_dielectric = true;
        }
        // fields a kind does not carry do not distinguish materials
        const float alpha = t.surface_kind == RTMI_SOLID ? 0.f : t.alpha;
        const float scat = t.surface_kind >= RTMI_REFLECTIVE ? t.scattering : 0.f;
        auto key = std::make_tuple(t.surface_kind, bits(t.color[0]), bits(t.color[1]), bits(t.color[2]), bits(alpha), bits(scat));
        auto it = matmap.find(key);
        uint32_t mid;
        if (it == matmap.end()) {
            mid = (uint32_t)matmap.size();
            matmap.emplace(key, mid);
            hm.push_back(make_float4(t.color[0], t.color[1], t.color[2], alpha));
            hm.push_back(make_float4(scat, fbits(t.surface_kind), 0.f, 0.f));
        } else mid = it->second;
        hp[2 * i] = make_float4(t.incenter[0], t.incenter[1], t.incenter[2], t.bounding_r2);
        hp[2 * i + 1] = make_float4(t.norm[0], t.norm[1], t.norm[2], fbits(mid));
        const float om = 1.f - t.edge_thickness;  // raytrace.rs:419
        for (int k = 0; k < 3; k++) he[4 * i + k] = make_float4(t.sides[k][0], t.sides[k][1], t.sides[k][2], t.side_lens[k]);
        he[4 * i + 3] = make_float4(t.side_lens[0] * om, t.side_lens[1] * om, t.side_lens[2] * om, 0.f);
    }
    if (matmap.size() > 65535) return fail(RTMI_ERR_UNSUPPORTED, "more than 65535 distinct surfaces");

    int ndev = rtmi_device_count();
    if (ndev <= 0) return fail(RTMI_ERR_NO_DEVICE, "no HIP device visible: the MI355X kernels cannot run (there is no CPU fallback)");
    if (device < 0 || device >= ndev) return fail(RTMI_ERR_INVALID, "device index out of range");
    HIPCHK(hipSetDevice(device));

    std::vector<uint32_t> hrefs(tri_refs, tri_refs + nrefs);
    struct Owner {  // destroys a half-built scene on any early exit, exceptions included
        rtmi_scene* s;
        ~Owner() { if (s) rtmi_scene_destroy(s); }
    } own{new rtmi_scene()};
    rtmi_scene* s = own.s;
    s->device = device;
    s->tune.batch_paths = env_size("RTMI_BATCH_PATHS", (size_t)256 << 20);
    s->tune.streams = (uint32_t)std::min<size_t>(env_size("RTMI_STREAMS", 0), RTMI_MAX_STREAMS);
    s->tune.subtile_min_paths = (uint32_t)std::min<size_t>(env_size("RTMI_SUBTILE_MIN_PATHS", 32768), 0xFFFFFFFFu);
    s->tune.oct_waves_per_cu = (uint32_t)std::min<size_t>(env_size("RTMI_OCT_WAVES_PER_CU", 0), 32);
    s->tune.refill_min0 = (uint32_t)std::min<size_t>(env_size("RTMI_REFILL_MIN0", 64), 64);
    s->tune.refill_min = (uint32_t)std::min<size_t>(env_size("RTMI_REFILL_MIN", 16), 64);
    s->tune.xcd_aware = (uint32_t)(env_size("RTMI_XCD_AWARE", 0) % 3);
    s->tune.pipeline = (uint32_t)std::min<size_t>(env_size("RTMI_PIPELINE", 0), 3);
    if (s->tune.pipeline == 2u) s->tune.pipeline = 0u;  // the removed fused pipeline: automatic
    s->tune.slow_path_off = (uint32_t)std::min<size_t>(env_size("RTMI_SLOW_PATH_OFF", 0), 1);
    s->verbose = getenv("RTMI_VERBOSE") != nullptr;
    if (const char* v = getenv("RTMI_PACKET_CULL")) s->packet_cull = strcmp(v, "0") != 0;  // (env_size treats 0 as unset)
    if (const char* v = getenv("RTMI_BLOCK_CULL")) s->block_cull = strcmp(v, "0") != 0;
    s->block_cull_n = (int)std::min<size_t>(std::max<size_t>(env_size("RTMI_BLOCK_CULL_N", 4), 2), 4);
    if (const char* v = getenv("RTMI_NODE_CULL")) s->node_cull = strcmp(v, "0") != 0;
    if (const char* v = getenv("RTMI_HYBRID")) s->hybrid = strcmp(v, "0") != 0;
    if (const char* v = getenv("RTMI_PRIMARY_NODE_CULL")) s->primary_node_cull = strcmp(v, "0") != 0;
    if (const char* v = getenv("RTMI_OCCLUDED_ANYHIT")) s->occl_from_hits = strcmp(v, "0") == 0;
    if (const char* v = getenv("RTMI_LIT_FROM_HITS")) s->lit_from_hits = strcmp(v, "0") != 0;
    if (const char* v = getenv("RTMI_DENOISE_LDS_STEP")) s->dn_lds_max_step = std::min<uint32_t>((uint32_t)strtoul(v, nullptr, 10), DN_LDS_MAX_STEP);
    if (const char* v = getenv("RTMI_DENOISE_VAR_LDS_STEP")) s->dnv_lds_max_step = std::min<uint32_t>((uint32_t)strtoul(v, nullptr, 10), DN_LDS_MAX_STEP);
    if (const char* v = getenv("RTMI_MIRROR_INPLACE")) {
        char* end = nullptr;
        const unsigned long n = strtoul(v, &end, 10);
        if (*v && end && *end == '\0') s->mirror_inplace = (int)std::min<unsigned long>(n, 65);
    }
    if (const char* v = getenv("RTMI_VOTE")) {
        int q[4];
        if (sscanf(v, "%d,%d,%d,%d", &q[0], &q[1], &q[2], &q[3]) == 4 && q[0] > 0 && q[1] > 0 && q[2] > 0 && q[3] > 0) memcpy(s->vote, q, sizeof q);
    }
    s->trace_block = block;
    s->trace_lds = (size_t)levels * 16 * block;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) s->num_cu = prop.multiProcessorCount;
    auto up = [&](auto& buf, const auto& host) -> hipError_t {
        hipError_t e = buf.ensure(std::max<size_t>(host.size(), 1));
        if (e != hipSuccess) return e;
        if (host.empty()) return hipSuccess;
        return hipMemcpy(buf.p, host.data(), host.size() * sizeof(host[0]), hipMemcpyHostToDevice);
    };
    hipError_t e = up(s->nodes, hn);
    if (e == hipSuccess) e = up(s->refs, hrefs);
    if (e == hipSuccess) e = up(s->tplane, hp);
    if (e == hipSuccess) e = up(s->tedge, he);
    if (e == hipSuccess) e = up(s->mats, hm);
    s->octree = !hfn.empty();
    s->nfn = (uint32_t)(hfn.size() / 2);
    s->root_is_leaf = boxes[0].is_leaf != 0;
    s->why_generic = why;
    if (e == hipSuccess && s->octree) e = up(s->fnodes, hfn);
    if (e == hipSuccess && s->octree) {
        // 15 zero blocks behind the last one: the whole-list cull of k_path_primary (trace_oct.hpp) reads the 16 blocks
        // from any block of a list on without a bounds test (they end no earlier than the array; noblocks stays the count)
        std::vector<uint4> hobp(hob);
        hobp.resize(hob.size() + 15, make_uint4(0u, 0u, 0u, 0u));
        e = up(s->oblocks, hobp);
    }
    if (e == hipSuccess && s->octree) e = up(s->wlinks, hwl);
    bool cert_on = false, fcull_on = false;
    size_t fcull_at = 0;  // where the node cull records begin in `fnodes`
    const bool bcull = s->octree && s->block_cull && hob.size() < (1ull << 27);  // (32-bit byte offsets)
    if (e == hipSuccess && bcull) {
        // The table's size grows with (distinct normals) x G and a ray's list with (distinct normals) / G: it pays for scenes
        // of up to RTMI_CERT_MAX_NORMALS distinct normals (the canonical scene has 6 717).  A scene with more
        // keeps the 32-B records and their normal box.
        std::vector<uint32_t> hcert;
        std::vector<uint4> hoc, hpk;
        const uint32_t G = (uint32_t)std::min<size_t>(std::max<size_t>(env_size("RTMI_CERT_G", 1024), 8), 1024);
        build_block_cull(hob.data(), hob.size(), hp.data(), ntris, hoc);
        if (!build_ray_cert(hp.data(), ntris, G, env_size("RTMI_CERT_MAX_NORMALS", 8192), hcert, s->cert_stats)) {
            hoc.resize(hoc.size() + 2, make_uint4(0u, 0u, 0u, 0u));  // the LEAF step reads a block's record and the next one's
            e = up(s->ocull, hoc);
        } else {
            cert_on = true;
            pack_block_cull(hoc, hpk);
            hpk.resize(hpk.size() + 3, make_uint4(0u, 0u, 0u, 0u));  // the LEAF step reads a block's record and the next three
            e = up(s->ocull, hpk);
            if (e == hipSuccess) e = up(s->cert, hcert);
            if (s->verbose)
                fprintf(stderr, "rtmi: sign certificate: G %u, %u distinct normals, %llu list entries (%.1f per cell, longest %u), %.1f MB, %.3f s\n",
                        G, s->cert_stats.normals, (unsigned long long)s->cert_stats.entries, (double)s->cert_stats.entries / (3.0 * G * G),
                        s->cert_stats.longest, (double)s->cert_stats.bytes / 1e6, s->cert_stats.seconds);
            if (e == hipSuccess && s->node_cull) {
                // one packed record per inner record: the box of everything below it (only a certified ray may use it)
                const auto t0 = std::chrono::steady_clock::now();
                std::vector<uint4> hnc, hnk;
                build_node_cull(hfn, hwl, hoc, hob.size(), hnc);
                pack_block_cull(hnc, hnk);
                s->node_cull_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
                s->node_cull_records = hnk.size();
                // behind the node records, in their buffer: the primary kernels address them from `fnodes` (PrimHdr::foff)
                std::vector<uint4> hfk(hfn);
                hfk.insert(hfk.end(), hnk.begin(), hnk.end());
                e = up(s->fnodes, hfk);
                fcull_on = e == hipSuccess && !hnk.empty();
                fcull_at = hfn.size();
                if (s->verbose)
                    fprintf(stderr, "rtmi: node cull: %llu records, %.2f MB, %.3f s\n", (unsigned long long)hnk.size(), (double)hnk.size() * 16.0 / 1e6,
                            s->node_cull_seconds);
            }
        }
    }
    for (int k = 0; k < RTMI_MAX_STREAMS && e == hipSuccess; k++) {
        e = s->w[k].ctrl.ensure(1);
        // zeroed once here (each batch zeroes its own): rtmi_debug_counters_n also reads the blocks of streams no render used
        if (e == hipSuccess) e = hipMemset(s->w[k].ctrl.p, 0, sizeof(DCtrl));
        if (e == hipSuccess) e = hipStreamCreateWithFlags(&s->istream[k], hipStreamNonBlocking);
        if (e == hipSuccess) e = hipEventCreate(&s->w[k].ev[0]);
        if (e == hipSuccess) e = hipEventCreate(&s->w[k].ev[1]);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&s->join_ev[k], hipEventDisableTiming);
    }
    if (e == hipSuccess) e = hipEventCreate(&s->fork_ev);
    if (e == hipSuccess) e = hipEventCreate(&s->end_ev);
    if (e != hipSuccess) return fail(hip_code(e), std::string("scene upload: ") + hipGetErrorString(e));
    s->d = DScene{s->nodes.p, s->refs.p, s->tplane.p, s->tedge.p, s->mats.p,
                  (uint32_t)nboxes, (uint32_t)ntris, (uint32_t)matmap.size(), levels,
                  s->octree ? s->fnodes.p : nullptr, s->octree ? s->oblocks.p : nullptr, s->octree ? s->wlinks.p : nullptr, nullptr, 0u, boxes[0].len2, max_inner_depth + 1, (uint32_t)hob.size(), bcull ? s->ocull.p : nullptr, cert_on ? s->cert.p : nullptr,
                  fcull_on ? s->fnodes.p + fcull_at : nullptr};
    s->hmats = hm;
    s->tris_dielectric = s->has_dielectric = has_dielectric;
    s->leaf_box = std::move(of.leafbox);
    if (s->octree) {
        // 2 words per level per lane (frame stack) + 3 per lane (leaf memo: key, t, tri | face; trace_oct.hpp)
        s->oct_lds = ((size_t)std::max<uint32_t>(1u, max_inner_depth) * 2 + 3) * 4 * 64;
        if (oct_launch_lds(s, true) > 64 * 1024) { s->octree = false; s->why_generic = "octree deeper than the LDS stack allows"; }
        else {
            int nb = 0;
            if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_trace_oct<false, false>, 64, s->oct_lds) == hipSuccess && nb > 0)
                s->oct_blocks_per_cu = nb;
        }
    }
    s->htris.assign(tris, tris + ntris);
    {   // fast-mode BVH (cheap: binned SAH over the triangles' disc boxes); absent when a record is not finite
        const int rc = upload_bvh(s);
        if (rc != RTMI_OK) return rc;
    }
    own.s = nullptr;
    *out = s;
    return RTMI_OK;
    RTMI_GUARD_END
}

int rtmi_scene_destroy(rtmi_scene_t* s) {
    if (!s) return RTMI_OK;
    (void)hipSetDevice(s->device);
    s->nodes.release(); s->refs.release(); s->tplane.release(); s->tedge.release(); s->mats.release();
    s->fnodes.release(); s->oblocks.release(); s->ocull.release(); s->cert.release(); s->wlinks.release(); s->bnodes.release(); s->bleaves.release(); s->spheres.release(); s->env.release(); s->envq.release(); s->envex.release(); s->envq_max.release(); s->envrows.release(); s->envrowsum.release(); s->em_idx.release(); s->em_list.release(); s->em_q.release(); s->em_max.release(); s->em_lamp.release(); s->em_c.release(); s->em_cum.release(); s->smooth.release(); s->textri.release(); s->texels.release(); s->texhdr.release(); s->nmaptri.release();
    for (int k = 0; k < RTMI_MAX_STREAMS; k++) {
        s->w[k].release();
        if (s->istream[k]) (void)hipStreamDestroy(s->istream[k]);
        if (s->join_ev[k]) (void)hipEventDestroy(s->join_ev[k]);
    }
    if (s->fork_ev) (void)hipEventDestroy(s->fork_ev);
    if (s->end_ev) (void)hipEventDestroy(s->end_ev);
    s->rec_cnt.release(); s->rec_ids.release(); s->rec_first.release();
    s->tile.release(); s->acc.release(); s->asq.release(); s->acnt.release();
    s->alist[0].release(); s->alist[1].release(); s->ablk.release(); s->qbytes.release(); s->mstage.release(); s->mframe.release();
    s->vcams.release(); s->dn_scratch.release(); s->dn_host.release();
    s->dnv_scratch.release(); s->dnv_host.release(); s->dnv_cnt.release();
    s->occ_tmax.release(); s->occ_out.release();
    for (auto& a : s->ao) a.release();
    s->ao_out.release();
    for (auto& l : s->light) l.release();
    s->light_out.release();
    for (auto& b : s->pv) b.release();
    for (auto& b : s->shadow) b.release();
    s->pv_out4.release(); s->pv_out1.release();
    if (s->vcams_ev) (void)hipEventDestroy(s->vcams_ev);
    if (s->mstream) (void)hipStreamDestroy(s->mstream);
    if (!s->comms.empty()) { if (Rccl* r = rccl_api()) for (ncclComm_t c : s->comms) (void)r->CommDestroy(c); }
    delete s;
    return RTMI_OK;
}

int rtmi_scene_set_options(rtmi_scene_t* s, uint32_t options) {
    if (!s) return fail(RTMI_ERR_INVALID, "scene is NULL");
    s->options = options;
    return RTMI_OK;
}

int rtmi_scene_set_spheres(rtmi_scene_t* s, const rtmi_sphere_t* sp, uint64_t n) {
    if (!s) return fail(RTMI_ERR_INVALID, "scene is NULL");
    if (n && !sp) return fail(RTMI_ERR_INVALID, "spheres is NULL");
    if (n > 4096) return fail(RTMI_ERR_UNSUPPORTED, "more than 4096 analytic spheres (they are a flat list, not in the tree)");
    if ((uint64_t)s->d.ntris + n >= (1ull << 30)) return fail(RTMI_ERR_UNSUPPORTED, "hit index space exhausted");
    RTMI_GUARD_BEGIN
    auto fbits = [](uint32_t u) { float f; memcpy(&f, &u, 4); return f; };
    std::vector<float4> mats = s->hmats, rec(2 * n);
    bool has_dielectric = s->tris_dielectric;
    for (uint64_t i = 0; i < n; i++) {
        if (sp[i].surface_kind > RTMI_DIELECTRIC) return fail(RTMI_ERR_INVALID, "unknown surface kind");
        if (sp[i].surface_kind == RTMI_DIELECTRIC) {  // scattering carries the index of refraction
            if (!(std::isfinite(sp[i].scattering) && sp[i].scattering > 0.f))
                return fail(RTMI_ERR_INVALID, "sphere " + std::to_string(i) + ": a dielectric's index of refraction (scattering) must be finite and > 0");
            has_dielectric = true;
        }
        const float alpha = sp[i].surface_kind == RTMI_SOLID ? 0.f : sp[i].alpha;
        const float scat = sp[i].surface_kind >= RTMI_REFLECTIVE ? sp[i].scattering : 0.f;
        const uint32_t mid = (uint32_t)(mats.size() / 2);
        mats.push_back(make_float4(sp[i].color[0], sp[i].color[1], sp[i].color[2], alpha));
        mats.push_back(make_float4(scat, fbits(sp[i].surface_kind), 0.f, 0.f));
        rec[2 * i] = make_float4(sp[i].center[0], sp[i].center[1], sp[i].center[2], sp[i].radius);
        rec[2 * i + 1] = make_float4(fbits(mid), 0.f, 0.f, 0.f);
    }
    if (mats.size() / 2 > 65535) return fail(RTMI_ERR_UNSUPPORTED, "more than 65535 distinct surfaces");
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(hipDeviceSynchronize());  // no render of this scene is in flight (one call at a time per handle)
    HIPCHK(s->mats.ensure(std::max<size_t>(mats.size(), 1)));
    HIPCHK(hipMemcpy(s->mats.p, mats.data(), mats.size() * sizeof(float4), hipMemcpyHostToDevice));
    HIPCHK(s->spheres.ensure(std::max<size_t>(rec.size(), 1)));
    if (n) HIPCHK(hipMemcpy(s->spheres.p, rec.data(), rec.size() * sizeof(float4), hipMemcpyHostToDevice));
    s->d.mats = s->mats.p;
    s->d.nmats = (uint32_t)(mats.size() / 2);
    s->d.spheres = s->spheres.p;
    s->d.nspheres = (uint32_t)n;
    s->has_dielectric = has_dielectric;
    return RTMI_OK;
    RTMI_GUARD_END
}

void rtmi_environment_defaults(rtmi_environment_t* e) {
    if (!e) return;
    const float id[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
    memcpy(e->frame, id, sizeof id);
    e->flags = 0u;
}

void rtmi_sky_defaults(rtmi_sky_t* k) {
    if (!k) return;
    const rtmi_sky_t d = {{0.f, 1.f, 0.f},        {-0.5f, 0.7f, -0.5f},   0.995f,          {0.15f, 0.35f, 0.9f},
                          {0.85f, 0.9f, 1.f},     {0.25f, 0.22f, 0.2f},   {40.f, 36.f, 28.f}};
    *k = d;
}

// the table is in place (or gone): what the k_shade*_env kernels get of it
static void env_set(rtmi_scene_t* s, uint32_t n, const float* frame) {
    s->envtab.tab = n ? s->env.p : nullptr;
    s->envtab.n = n;
    s->envtab.fn = (float)n;
    if (n) {
        s->envtab.r0 = make_float4(frame[0], frame[1], frame[2], 0.f);
        s->envtab.r1 = make_float4(frame[3], frame[4], frame[5], 0.f);
        s->envtab.r2 = make_float4(frame[6], frame[7], frame[8], 0.f);
    }
    s->has_env = n != 0u;
    s->envsamp_ok = false;  // the sampler table is of the table that was
}

int rtmi_scene_set_environment(rtmi_scene_t* s, const float* rgb, uint32_t n, const rtmi_environment_t* env) {
    if (!s) return fail(RTMI_ERR_INVALID, "scene is NULL");
    rtmi_environment_t e;
    rtmi_environment_defaults(&e);
    if (env) e = *env;
    if (rgb && n) {
        if (n > 4096u) return fail(RTMI_ERR_INVALID, "environment: n must be 1 to 4096");
        if (e.flags != 0u) return fail(RTMI_ERR_INVALID, "environment: flags must be 0");
        for (int k = 0; k < 9; k++)
            if (!std::isfinite(e.frame[k])) return fail(RTMI_ERR_INVALID, "environment: frame entry " + std::to_string(k) + " is not finite");
    }
    RTMI_GUARD_BEGIN
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(hipDeviceSynchronize());  // no render of this scene is in flight: its streams are done with the old table
    if (!rgb || !n) {
        env_set(s, 0u, nullptr);
        s->env.release();
        return RTMI_OK;
    }
    const size_t nt = (size_t)n * n;
    std::vector<float4> tab(nt);
    for (size_t k = 0; k < nt; k++) tab[k] = make_float4(rgb[3 * k], rgb[3 * k + 1], rgb[3 * k + 2], 0.f);
    env_set(s, 0u, nullptr);  // (a failure below leaves the scene without an environment, not with a stale one)
    HIPCHK(s->env.ensure(nt));
    HIPCHK(hipMemcpy(s->env.p, tab.data(), nt * sizeof(float4), hipMemcpyHostToDevice));
    env_set(s, n, e.frame);
    return RTMI_OK;
    RTMI_GUARD_END
}

int rtmi_scene_set_sky(rtmi_scene_t* s, uint32_t n, const rtmi_sky_t* sky) {
    if (!s) return fail(RTMI_ERR_INVALID, "scene is NULL");
    if (n < 1u || n > 4096u) return fail(RTMI_ERR_INVALID, "sky: n must be 1 to 4096");
    rtmi_sky_t k;
    rtmi_sky_defaults(&k);
    if (sky) k = *sky;
    auto usable = [](const float* v) {
        return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]) && (v[0] != 0.f || v[1] != 0.f || v[2] != 0.f);
    };
    if (!usable(k.up)) return fail(RTMI_ERR_INVALID, "sky: up must be finite and not zero");
    if (!usable(k.sun_dir)) return fail(RTMI_ERR_INVALID, "sky: sun_dir must be finite and not zero");
    RTMI_GUARD_BEGIN
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(hipDeviceSynchronize());  // no render of this scene is in flight: its streams are done with the old table
    const size_t nt = (size_t)n * n;
    env_set(s, 0u, nullptr);
    HIPCHK(s->env.ensure(nt));
    auto f4 = [](const float* v) { return make_float4(v[0], v[1], v[2], 0.f); };
    const SkyArgs a{f4(k.up), f4(k.sun_dir), f4(k.zenith), f4(k.horizon), f4(k.ground), f4(k.sun_color), k.sun_cos};
    hipLaunchKernelGGL(k_env_sky, dim3((unsigned)((nt + 255u) / 256u)), dim3(256), 0, 0, s->env.p, n, (float)n, a);
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    rtmi_environment_t e;
    rtmi_environment_defaults(&e);
    env_set(s, n, e.frame);
    return RTMI_OK;
    RTMI_GUARD_END
}

int rtmi_scene_get_environment(rtmi_scene_t* s, float* rgb_out, uint32_t* n_out) {
    if (!s || !n_out) return fail(RTMI_ERR_INVALID, "NULL argument");
    *n_out = s->has_env ? s->envtab.n : 0u;
    if (!s->has_env || !rgb_out) return RTMI_OK;
    RTMI_GUARD_BEGIN
    const size_t nt = (size_t)s->envtab.n * s->envtab.n;
    std::vector<float4> tab(nt);
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(tab.data(), s->env.p, nt * sizeof(float4), hipMemcpyDeviceToHost));
    for (size_t k = 0; k < nt; k++) { rgb_out[3 * k] = tab[k].x; rgb_out[3 * k + 1] = tab[k].y; rgb_out[3 * k + 2] = tab[k].z; }
    return RTMI_OK;
    RTMI_GUARD_END
}

// the table is in place (or gone): what the k_shade*_smooth / k_features_smooth kernels get of it
static void smooth_set(rtmi_scene_t* s, uint32_t n) {
    s->smoothtab.tab = n ? s->smooth.p : nullptr;
    s->smoothtab.n = n;
    s->has_normals = n != 0u;
}

int rtmi_scene_set_normals(rtmi_scene_t* s, const float* corners9, const float* normals9, uint64_t n) {
    if (!s) return fail(RTMI_ERR_INVALID, "scene is NULL");
    const bool set = normals9 && n;
    if (set) {
        if (!corners9) return fail(RTMI_ERR_INVALID, "normals: corners is NULL");
        if (n != s->d.ntris) return fail(RTMI_ERR_INVALID, "normals: n must equal ntris");
        for (uint64_t k = 9; k < n * 9; k++) {  // (entry 0 is the sentinel's and is ignored)
            if (!std::isfinite(corners9[k])) return fail(RTMI_ERR_INVALID, "normals: a corner of triangle " + std::to_string(k / 9) + " is not finite");
            if (!std::isfinite(normals9[k])) return fail(RTMI_ERR_INVALID, "normals: a normal of triangle " + std::to_string(k / 9) + " is not finite");
        }
    }
    RTMI_GUARD_BEGIN
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(hipDeviceSynchronize());  // no render of this scene is in flight: its streams are done with the old table
    if (!set) {
        smooth_set(s, 0u);
        s->smooth.release();
        return RTMI_OK;
    }
    // the per-triangle part of the definition, once: f32, every step rounded (this file is compiled without contraction)
    std::vector<float4> tab((size_t)n * 6, make_float4(0.f, 0.f, 0.f, 0.f));
    for (uint64_t g = 1; g < n; g++) {
        const float *c = corners9 + 9 * g, *nn = normals9 + 9 * g;
        const V4 c0 = mk(c[0], c[1], c[2]), e1 = vsub(mk(c[3], c[4], c[5]), c0), e2 = vsub(mk(c[6], c[7], c[8]), c0);
        const float d00 = vdot(e1, e1), d01 = vdot(e1, e2), d11 = vdot(e2, e2), den = d00 * d11 - d01 * d01;
        float4* r = &tab[(size_t)g * 6];
        r[0] = make_float4(c0.x, c0.y, c0.z, d00);
        r[1] = make_float4(e1.x, e1.y, e1.z, d01);
        r[2] = make_float4(e2.x, e2.y, e2.z, d11);
        r[3] = make_float4(nn[0], nn[1], nn[2], den);
        r[4] = make_float4(nn[3], nn[4], nn[5], 0.f);
        r[5] = make_float4(nn[6], nn[7], nn[8], 0.f);
    }
    smooth_set(s, 0u);  // (a failure below leaves the scene without normals, not with stale ones)
    HIPCHK(s->smooth.ensure(tab.size()));
    HIPCHK(hipMemcpy(s->smooth.p, tab.data(), tab.size() * sizeof(float4), hipMemcpyHostToDevice));
    smooth_set(s, (uint32_t)n);
    return RTMI_OK;
    RTMI_GUARD_END
}

int rtmi_scene_get_normals(rtmi_scene_t* s, float* normals9_out, uint64_t* n_out) {
    if (!s || !n_out) return fail(RTMI_ERR_INVALID, "NULL argument");
    *n_out = s->has_normals ? s->smoothtab.n : 0u;
    if (!s->has_normals || !normals9_out) return RTMI_OK;
    RTMI_GUARD_BEGIN
    const size_t n = s->smoothtab.n;
    std::vector<float4> tab(n * 6);
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(tab.data(), s->smooth.p, tab.size() * sizeof(float4), hipMemcpyDeviceToHost));
    for (size_t g = 0; g < n; g++)
        for (int k = 0; k < 3; k++) {
            const float4 q = tab[g * 6 + 3 + k];
            normals9_out[9 * g + 3 * k] = q.x; normals9_out[9 * g + 3 * k + 1] = q.y; normals9_out[9 * g + 3 * k + 2] = q.z;
        }
    return RTMI_OK;
    RTMI_GUARD_END
}

// rtmi_smooth_normals (include/rtmi.h): host code, no HIP call.  The definition sums, per corner, the area-weighted face normals of
// the triangles that share the corner's position, in increasing triangle index.  Here the positions are hashed once (-0 as +0,
// which == does not tell apart; a NaN equals nothing and is left out) to the increasing list of the triangles that touch them, so
// a corner walks its own position's list only: the same additions in the same order, in about O(n).
int rtmi_smooth_normals(const float* corners9, const float* facenorm3, uint64_t n, float crease_cos, float* normals9_out) {
    if (!(crease_cos >= -1.f && crease_cos <= 1.f)) return fail(RTMI_ERR_INVALID, "smooth_normals: crease_cos must be in [-1, 1]");
    if (n == 0) return RTMI_OK;
    if (!corners9 || !facenorm3 || !normals9_out) return fail(RTMI_ERR_INVALID, "NULL argument");
    if (n > 0x3FFFFFFFull) return fail(RTMI_ERR_INVALID, "smooth_normals: too many triangles");
    RTMI_GUARD_BEGIN
    struct Key {
        uint32_t x, y, z;
        bool operator==(const Key& o) const { return x == o.x && y == o.y && z == o.z; }
    };
    struct KeyHash {
        size_t operator()(const Key& k) const {
            uint64_t h = k.x * 0x9E3779B97F4A7C15ull;
            h = (h ^ (h >> 29) ^ k.y) * 0xBF58476D1CE4E5B9ull;
            h = (h ^ (h >> 32) ^ k.z) * 0x94D049BB133111EBull;
            return (size_t)(h ^ (h >> 31));
        }
    };
    auto key_of = [](const float* p, Key& k) {
        if (p[0] != p[0] || p[1] != p[1] || p[2] != p[2]) return false;
        const float q[3] = {p[0] + 0.f, p[1] + 0.f, p[2] + 0.f};  // -0 + 0 = +0
        memcpy(&k, q, sizeof k);
        return true;
    };
    std::vector<V4> wg(n);
    std::unordered_map<Key, uint32_t, KeyHash> slot;
    slot.reserve((size_t)n * 3 / 2 + 16);
    std::vector<std::vector<uint32_t>> touch;
    for (uint64_t g = 0; g < n; g++) {
        const float* c = corners9 + 9 * g;
        const V4 a = vsub(mk(c[3], c[4], c[5]), mk(c[0], c[1], c[2])), b = vsub(mk(c[6], c[7], c[8]), mk(c[0], c[1], c[2]));
        const V4 x = mk(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x);
        wg[g] = vmul(mk(facenorm3[3 * g], facenorm3[3 * g + 1], facenorm3[3 * g + 2]), sqrtf(vdot(x, x)));
        for (int k = 0; k < 3; k++) {
            Key key;
            if (!key_of(c + 3 * k, key)) continue;
            auto it = slot.find(key);
            if (it == slot.end()) {
                it = slot.emplace(key, (uint32_t)touch.size()).first;
                touch.emplace_back();
            }
            std::vector<uint32_t>& l = touch[it->second];
            if (l.empty() || l.back() != (uint32_t)g) l.push_back((uint32_t)g);  // each g at most once per position
        }
    }
    for (uint64_t f = 0; f < n; f++) {
        const V4 nf = mk(facenorm3[3 * f], facenorm3[3 * f + 1], facenorm3[3 * f + 2]);
        for (int k = 0; k < 3; k++) {
            V4 s = mk(0.f, 0.f, 0.f);
            Key key;
            if (key_of(corners9 + 9 * f + 3 * k, key))
                for (uint32_t g : touch[slot.find(key)->second])
                    if (g == f || vdot(nf, mk(facenorm3[3 * g], facenorm3[3 * g + 1], facenorm3[3 * g + 2])) >= crease_cos) s = vadd(s, wg[g]);
            const V4 u = vunit(s);
            float* o = normals9_out + 9 * f + 3 * k;
            o[0] = u.x; o[1] = u.y; o[2] = u.z;
        }
    }
    return RTMI_OK;
    RTMI_GUARD_END
}

// the tables are in place (or gone): what the k_shade*_tex / k_features_tex kernels get of them
static void nmap_set(rtmi_scene_t* s, uint32_t n, float strength) {
    s->nmaptab.tri = n ? s->nmaptri.p : nullptr;
    s->nmaptab.n = n;
    s->nmaptab.strength = n ? strength : 0.f;
    s->has_nmap = n != 0u;
}
static void tex_set(rtmi_scene_t* s, uint32_t n, uint32_t ntex) {
    s->textab.tri = n ? s->textri.p : nullptr;
    s->textab.hdr = n ? s->texhdr.p : nullptr;
    s->textab.texels = n ? s->texels.p : nullptr;
    s->textab.n = n;
    s->ntex = n ? ntex : 0u;
    s->has_tex = n != 0u;
}

int rtmi_scene_set_textures(rtmi_scene_t* s, const rtmi_texture_t* tex, uint32_t ntex, const float* corners9, const float* uvs6,
                            const uint32_t* tex_of_tri, uint64_t n) {
    if (!s) return fail(RTMI_ERR_INVALID, "scene is NULL");
    const bool set = tex && ntex;
    uint64_t total = 0;
    if (set) {
        if (!corners9 || !uvs6 || !tex_of_tri) return fail(RTMI_ERR_INVALID, "textures: corners, uvs or tex_of_tri is NULL");
        if (n != s->d.ntris) return fail(RTMI_ERR_INVALID, "textures: n must equal ntris");
        if (ntex > 256u) return fail(RTMI_ERR_INVALID, "textures: more than 256 textures");
        for (uint32_t k = 0; k < ntex; k++) {
            const std::string name = "textures: texture " + std::to_string(k + 1);
            if (tex[k].flags != 0u) return fail(RTMI_ERR_INVALID, name + " has flags != 0");
            if (!tex[k].rgb) return fail(RTMI_ERR_INVALID, name + " has no texels (rgb is NULL)");
            if (tex[k].width < 1u || tex[k].width > 8192u || tex[k].height < 1u || tex[k].height > 8192u)
                return fail(RTMI_ERR_INVALID, name + ": width and height must be 1 to 8192");
            total += (uint64_t)tex[k].width * tex[k].height;
            if (total > (1ull << 26)) return fail(RTMI_ERR_INVALID, name + ": more than 2^26 texels in all");
        }
        for (uint64_t g = 1; g < n; g++) {  // (entry 0 is the sentinel's and is ignored)
            if (tex_of_tri[g] > ntex)
                return fail(RTMI_ERR_INVALID, "textures: tex_of_tri of triangle " + std::to_string(g) + " is above ntex");
            if (tex_of_tri[g] == 0u) continue;
            for (int k = 0; k < 9; k++)
                if (!std::isfinite(corners9[9 * g + k])) return fail(RTMI_ERR_INVALID, "textures: a corner of triangle " + std::to_string(g) + " is not finite");
            for (int k = 0; k < 6; k++)
                if (!std::isfinite(uvs6[6 * g + k])) return fail(RTMI_ERR_INVALID, "textures: a uv of triangle " + std::to_string(g) + " is not finite");
        }
    }
    RTMI_GUARD_BEGIN
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(hipDeviceSynchronize());  // no render of this scene is in flight: its streams are done with the old tables
    // the normal maps name images by number: set, replace or remove the images and they are gone
    nmap_set(s, 0u, 0.f);
    s->nmaptri.release();
    if (!set) {
        tex_set(s, 0u, 0u);
        s->textri.release(); s->texhdr.release(); s->texels.release();
        return RTMI_OK;
    }
    // the per-triangle part of the definition, by the statements of rtmi_scene_set_normals: f32, every step rounded
    std::vector<float4> tab((size_t)n * 5, make_float4(0.f, 0.f, 0.f, 0.f));
    for (uint64_t g = 1; g < n; g++) {
        const float *c = corners9 + 9 * g, *uv = uvs6 + 6 * g;
        const V4 c0 = mk(c[0], c[1], c[2]), e1 = vsub(mk(c[3], c[4], c[5]), c0), e2 = vsub(mk(c[6], c[7], c[8]), c0);
        const float d00 = vdot(e1, e1), d01 = vdot(e1, e2), d11 = vdot(e2, e2), den = d00 * d11 - d01 * d01;
        const uint32_t k = den == 0.f ? 0u : tex_of_tri[g];  // a degenerate triangle has no barycentric coordinates: no texture
        float kf;
        memcpy(&kf, &k, sizeof kf);
        float4* r = &tab[(size_t)g * 5];
        r[0] = make_float4(c0.x, c0.y, c0.z, d00);
        r[1] = make_float4(e1.x, e1.y, e1.z, d01);
        r[2] = make_float4(e2.x, e2.y, e2.z, d11);
        r[3] = make_float4(uv[0], uv[2], uv[4], den);
        r[4] = make_float4(uv[1], uv[3], uv[5], kf);
    }
    std::vector<uint4> hdr(ntex);
    std::vector<float4> texels((size_t)total);
    size_t off = 0;
    for (uint32_t k = 0; k < ntex; k++) {
        const size_t m = (size_t)tex[k].width * tex[k].height;
        hdr[k] = make_uint4((uint32_t)off, tex[k].width, tex[k].height, 0u);
        for (size_t i = 0; i < m; i++) texels[off + i] = make_float4(tex[k].rgb[3 * i], tex[k].rgb[3 * i + 1], tex[k].rgb[3 * i + 2], 0.f);
        off += m;
    }
    tex_set(s, 0u, 0u);  // (a failure below leaves the scene without textures, not with stale ones)
    HIPCHK(s->textri.ensure(tab.size()));
    HIPCHK(s->texhdr.ensure(hdr.size()));
    HIPCHK(s->texels.ensure(texels.size()));
    HIPCHK(hipMemcpy(s->textri.p, tab.data(), tab.size() * sizeof(float4), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(s->texhdr.p, hdr.data(), hdr.size() * sizeof(uint4), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(s->texels.p, texels.data(), texels.size() * sizeof(float4), hipMemcpyHostToDevice));
    tex_set(s, (uint32_t)n, ntex);
    return RTMI_OK;
    RTMI_GUARD_END
}

int rtmi_scene_get_uvs(rtmi_scene_t* s, float* uvs6_out, uint32_t* tex_of_tri_out, uint64_t* n_out) {
    if (!s || !n_out) return fail(RTMI_ERR_INVALID, "NULL argument");
    *n_out = s->has_tex ? s->textab.n : 0u;
    if (!s->has_tex || (!uvs6_out && !tex_of_tri_out)) return RTMI_OK;
    RTMI_GUARD_BEGIN
    const size_t n = s->textab.n;
    std::vector<float4> tab(n * 5);
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(tab.data(), s->textri.p, tab.size() * sizeof(float4), hipMemcpyDeviceToHost));
    for (size_t g = 0; g < n; g++) {
        const float4 qu = tab[g * 5 + 3], qv = tab[g * 5 + 4];
        if (uvs6_out) {
            float* o = uvs6_out + 6 * g;
            o[0] = qu.x; o[1] = qv.x; o[2] = qu.y; o[3] = qv.y; o[4] = qu.z; o[5] = qv.z;
        }
        if (tex_of_tri_out) memcpy(&tex_of_tri_out[g], &qv.w, sizeof(uint32_t));
    }
    return RTMI_OK;
    RTMI_GUARD_END
}

int rtmi_scene_get_texture(rtmi_scene_t* s, uint32_t k, float* rgb_out, uint32_t* w_out, uint32_t* h_out) {
    if (!s || !w_out || !h_out) return fail(RTMI_ERR_INVALID, "NULL argument");
    if (!s->has_tex || k < 1u || k > s->ntex) return fail(RTMI_ERR_INVALID, "get_texture: k must be 1 to the number of textures");
    RTMI_GUARD_BEGIN
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(hipDeviceSynchronize());
    uint4 h;
    HIPCHK(hipMemcpy(&h, s->texhdr.p + (k - 1u), sizeof h, hipMemcpyDeviceToHost));
    *w_out = h.y;
    *h_out = h.z;
    if (!rgb_out) return RTMI_OK;
    std::vector<float4> t((size_t)h.y * h.z);
    HIPCHK(hipMemcpy(t.data(), s->texels.p + h.x, t.size() * sizeof(float4), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < t.size(); i++) { rgb_out[3 * i] = t[i].x; rgb_out[3 * i + 1] = t[i].y; rgb_out[3 * i + 2] = t[i].z; }
    return RTMI_OK;
    RTMI_GUARD_END
}

// rtmi_project_uvs (include/rtmi.h): host code, no HIP call, no sentinel.  A box projection: the axis of the largest |facenorm|
// component is dropped and the other two, in cyclic order, become (u, v).
int rtmi_project_uvs(const float* corners9, const float* facenorm3, uint64_t n, const float lo[3], float scale, float* uvs6_out) {
    if (n == 0) return RTMI_OK;
    if (!corners9 || !facenorm3 || !lo || !uvs6_out) return fail(RTMI_ERR_INVALID, "NULL argument");
    for (uint64_t g = 0; g < n; g++) {
        const float ax = fabsf(facenorm3[3 * g]), ay = fabsf(facenorm3[3 * g + 1]), az = fabsf(facenorm3[3 * g + 2]);
        const int a = ax >= ay && ax >= az ? 0 : (ay >= az ? 1 : 2);
        const int j = (a + 1) % 3, k = (a + 2) % 3;
        for (int p = 0; p < 3; p++) {
            const float* c = corners9 + 9 * g + 3 * p;
            uvs6_out[6 * g + 2 * p] = (c[j] - lo[j]) * scale;
            uvs6_out[6 * g + 2 * p + 1] = (c[k] - lo[k]) * scale;
        }
    }
    return RTMI_OK;
}

void rtmi_normal_maps_defaults(rtmi_normal_maps_t* o) {
    if (!o) return;
    o->strength = 1.f;
    o->flags = 0u;
}

// rtmi_normal_map_frames (include/rtmi.h "NORMAL MAPS OF A SCENE"): the per-triangle part of the definition.  Host code, no HIP call,
// no sentinel.  frames4_out: (T.xyz, bits) per triangle, NmapTab's record.
int rtmi_normal_map_frames(const float* corners9, const float* uvs6, const float* facenorm3, const uint32_t* nmap_of_tri, uint64_t n,
                           float* frames4_out) {
    if (n == 0) return RTMI_OK;
    if (!corners9 || !uvs6 || !facenorm3 || !nmap_of_tri || !frames4_out) return fail(RTMI_ERR_INVALID, "NULL argument");
    for (uint64_t g = 0; g < n; g++) {
        float* out = frames4_out + 4 * g;
        out[0] = out[1] = out[2] = out[3] = 0.f;
        if (nmap_of_tri[g] == 0u) continue;
        const float *c = corners9 + 9 * g, *uv = uvs6 + 6 * g, *nn = facenorm3 + 3 * g;
        const V4 c0 = mk(c[0], c[1], c[2]), e1 = vsub(mk(c[3], c[4], c[5]), c0), e2 = vsub(mk(c[6], c[7], c[8]), c0);
        const float d00 = vdot(e1, e1), d01 = vdot(e1, e2), d11 = vdot(e2, e2), den = d00 * d11 - d01 * d01;
        const float du1 = uv[2] - uv[0], du2 = uv[4] - uv[0], dv1 = uv[3] - uv[1], dv2 = uv[5] - uv[1];
        const float det = du1 * dv2 - du2 * dv1;
        if (det == 0.f || den == 0.f) continue;  // no tangent frame: stored with map 0
        V4 T = vsub(vmul(e1, dv2), vmul(e2, dv1)), B = vsub(vmul(e2, du1), vmul(e1, du2));
        if (det < 0.f) { T = vmul(T, -1.f); B = vmul(B, -1.f); }
        const V4 ng = mk(nn[0], nn[1], nn[2]);
        const V4 x = mk(ng.y * T.z - ng.z * T.y, ng.z * T.x - ng.x * T.z, ng.x * T.y - ng.y * T.x);
        const bool neg = !(vdot(x, B) >= 0.f);
        const uint32_t bits = nmap_of_tri[g] | (neg ? 0x80000000u : 0u);
        out[0] = T.x; out[1] = T.y; out[2] = T.z;
        memcpy(&out[3], &bits, sizeof bits);
    }
    return RTMI_OK;
}

// rtmi_scene_set_normal_maps (include/rtmi.h "NORMAL MAPS OF A SCENE"): the per-triangle frame, once, on the host.  The uvs are
// read back from the texture table, where rtmi_scene_set_textures stored them.
int rtmi_scene_set_normal_maps(rtmi_scene_t* s, const float* corners9, const uint32_t* nmap_of_tri, uint64_t n, const rtmi_normal_maps_t* opt) {
    if (!s) return fail(RTMI_ERR_INVALID, "scene is NULL");
    const bool set = nmap_of_tri && n;
    rtmi_normal_maps_t o;
    rtmi_normal_maps_defaults(&o);
    if (opt) o = *opt;
    if (set) {
        if (!s->has_tex) return fail(RTMI_ERR_INVALID, "normal maps: the scene has no textures (a map is one of rtmi_scene_set_textures' images)");
        if (!corners9) return fail(RTMI_ERR_INVALID, "normal maps: corners is NULL");
        if (n != s->d.ntris) return fail(RTMI_ERR_INVALID, "normal maps: n must equal ntris");
        if (o.flags != 0u) return fail(RTMI_ERR_INVALID, "normal maps: flags != 0");
        if (!std::isfinite(o.strength)) return fail(RTMI_ERR_INVALID, "normal maps: strength is not finite");
        for (uint64_t g = 1; g < n; g++) {  // (entry 0 is the sentinel's and is ignored)
            if (nmap_of_tri[g] > s->ntex)
                return fail(RTMI_ERR_INVALID, "normal maps: nmap_of_tri of triangle " + std::to_string(g) + " is above ntex");
            if (nmap_of_tri[g] == 0u) continue;
            for (int k = 0; k < 9; k++)
                if (!std::isfinite(corners9[9 * g + k])) return fail(RTMI_ERR_INVALID, "normal maps: a corner of triangle " + std::to_string(g) + " is not finite");
        }
    }
    RTMI_GUARD_BEGIN
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(hipDeviceSynchronize());  // no render of this scene is in flight: its streams are done with the old table
    if (!set) {
        nmap_set(s, 0u, 0.f);
        s->nmaptri.release();
        return RTMI_OK;
    }
    std::vector<float4> ttab((size_t)n * 5);
    HIPCHK(hipMemcpy(ttab.data(), s->textri.p, ttab.size() * sizeof(float4), hipMemcpyDeviceToHost));
    std::vector<float4> tab((size_t)n, make_float4(0.f, 0.f, 0.f, 0.f));
    {
        std::vector<float> uvs((size_t)n * 6), fn((size_t)n * 3);
        for (uint64_t g = 0; g < n; g++) {
            const float4 qu = ttab[(size_t)g * 5 + 3], qv = ttab[(size_t)g * 5 + 4];
            float* o = &uvs[6 * g];
            o[0] = qu.x; o[1] = qv.x; o[2] = qu.y; o[3] = qv.y; o[4] = qu.z; o[5] = qv.z;
            memcpy(&fn[3 * g], s->htris[g].norm, 12);
        }
        // (entry 0, the sentinel's, stays zero)
        const int rc = rtmi_normal_map_frames(corners9 + 9, uvs.data() + 6, fn.data() + 3, nmap_of_tri + 1, n - 1, reinterpret_cast<float*>(tab.data() + 1));
        if (rc != RTMI_OK) return rc;
    }
    nmap_set(s, 0u, 0.f);  // (a failure below leaves the scene without maps, not with stale ones)
    HIPCHK(s->nmaptri.ensure(tab.size()));
    HIPCHK(hipMemcpy(s->nmaptri.p, tab.data(), tab.size() * sizeof(float4), hipMemcpyHostToDevice));
    nmap_set(s, (uint32_t)n, o.strength);
    return RTMI_OK;
    RTMI_GUARD_END
}

int rtmi_scene_get_normal_maps(rtmi_scene_t* s, uint32_t* nmap_of_tri_out, float* strength_out, uint64_t* n_out) {
    if (!s || !n_out) return fail(RTMI_ERR_INVALID, "NULL argument");
    *n_out = s->has_nmap ? s->nmaptab.n : 0u;
    if (strength_out) *strength_out = s->has_nmap ? s->nmaptab.strength : 0.f;
    if (!s->has_nmap || !nmap_of_tri_out) return RTMI_OK;
    RTMI_GUARD_BEGIN
    const size_t n = s->nmaptab.n;
    std::vector<float4> tab(n);
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(tab.data(), s->nmaptri.p, tab.size() * sizeof(float4), hipMemcpyDeviceToHost));
    for (size_t g = 0; g < n; g++) {
        uint32_t bits;
        memcpy(&bits, &tab[g].w, sizeof bits);
        nmap_of_tri_out[g] = bits & 0x7FFFFFFFu;
    }
    return RTMI_OK;
    RTMI_GUARD_END
}

// rtmi_normal_map_from_height (include/rtmi.h): host code, no HIP call.  Repeat-wrapped central differences of a height field.
int rtmi_normal_map_from_height(const float* height, uint32_t w, uint32_t h, float scale, float* rgb_out) {
    if ((uint64_t)w * h == 0) return RTMI_OK;
    if (!height || !rgb_out) return fail(RTMI_ERR_INVALID, "NULL argument");
    for (uint32_t j = 0; j < h; j++) {
        const size_t jm = (size_t)(j == 0 ? h - 1 : j - 1) * w, jp = (size_t)(j == h - 1 ? 0 : j + 1) * w, jj = (size_t)j * w;
        for (uint32_t i = 0; i < w; i++) {
            const uint32_t im = i == 0 ? w - 1 : i - 1, ip = i == w - 1 ? 0 : i + 1;
            const float dx = ((height[jj + ip] - height[jj + im]) * 0.5f) * scale;
            const float dy = ((height[jp + i] - height[jm + i]) * 0.5f) * scale;
            const V4 nn = vunit(mk(dx * -1.f, dy * -1.f, 1.f));
            float* o = rgb_out + 3 * (jj + i);
            o[0] = nn.x * 0.5f + 0.5f; o[1] = nn.y * 0.5f + 0.5f; o[2] = nn.z * 0.5f + 0.5f;
        }
    }
    return RTMI_OK;
}

int rtmi_scene_set_corners(rtmi_scene_t* s, const float* corners9, uint64_t n) {
    if (!s) return fail(RTMI_ERR_INVALID, "scene is NULL");
    if (!corners9) return fail(RTMI_ERR_INVALID, "corners is NULL");
    if (n != s->htris.size()) return fail(RTMI_ERR_INVALID, "one corner triple per triangle of the scene (the sentinel included)");
    RTMI_GUARD_BEGIN
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(hipDeviceSynchronize());  // no render of this scene is in flight (one call at a time per handle)
    // The BVH's boxes come from the records' own edge tests since the hybrid passes rely on them (bvh_clip_box, bvh_fast.hpp):
    // the corners no longer enter them, and the tree built at scene creation stays.
    return RTMI_OK;
    RTMI_GUARD_END
}

int rtmi_scene_get_tuning(rtmi_scene_t* s, rtmi_tuning_t* out) {
    if (!s || !out) return fail(RTMI_ERR_INVALID, "NULL argument");
    *out = s->tune;
    return RTMI_OK;
}

int rtmi_scene_set_tuning(rtmi_scene_t* s, const rtmi_tuning_t* in) {
    if (!s || !in) return fail(RTMI_ERR_INVALID, "NULL argument");
    if (in->batch_paths == 0 || in->streams > RTMI_MAX_STREAMS || in->oct_waves_per_cu > 32 || in->refill_min0 < 1 ||
        in->refill_min0 > 64 || in->refill_min < 1 || in->refill_min > 64 || in->xcd_aware > 2 || in->kernel > 2 || in->pipeline > 3 || in->slow_path_off > 1)
        return fail(RTMI_ERR_INVALID, "tuning value out of range");
    if (in->kernel == 2) return fail(RTMI_ERR_UNSUPPORTED, "tuning kernel = 2: the ray-pool kernel k_trace_pool was removed (0 and 1 select k_trace_oct)");
    if (in->pipeline == 2) return fail(RTMI_ERR_UNSUPPORTED, "tuning pipeline = 2: the fused bounce pipeline was removed (0, 1 or 3)");
    s->tune = *in;
    return RTMI_OK;
}

static int ensure_workspace(Work& w, size_t cap, uint32_t maxdepth) {
    if (cap <= w.cap && maxdepth <= w.cap_depth) return RTMI_OK;
    cap = std::max(cap, w.cap);
    maxdepth = std::max(maxdepth, w.cap_depth);
    for (int k = 0; k < 2; k++) {
        HIPCHK(w.qo[k].ensure(cap));
        HIPCHK(w.qd[k].ensure(cap));
        HIPCHK(w.qpath[k].ensure(cap));
    }
    HIPCHK(w.scol.ensure(cap));
    HIPCHK(w.hit_tf.ensure(cap));
    HIPCHK(w.hit_t.ensure(cap));
    HIPCHK(w.fb.ensure(cap));
    HIPCHK(w.mstack.ensure(cap * (size_t)maxdepth));
    HIPCHK(w.sqo.ensure(RTMI_SLOW_CAP)); HIPCHK(w.sqd.ensure(RTMI_SLOW_CAP));
    HIPCHK(w.sqpath.ensure(RTMI_SLOW_CAP)); HIPCHK(w.sqbounce.ensure(RTMI_SLOW_CAP));
    if (!w.sstream) {
        // highest priority: the persistent kernels of the ordinary passes never yield their wave slots, so the slow path's
        // blocks must be first in line whenever slots come free (the end of the producer launch), not behind the queued
        // blocks of the other streams' launches
        int lo = 0, hi = 0;
        if (hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess) { (void)hipGetLastError(); lo = hi = 0; }
        HIPCHK(hipStreamCreateWithPriority(&w.sstream, hipStreamNonBlocking, hi));
    }
    if (!w.sdone) HIPCHK(hipEventCreateWithFlags(&w.sdone, hipEventDisableTiming));
    if (!w.sgo) HIPCHK(hipEventCreateWithFlags(&w.sgo, hipEventDisableTiming));
    while (w.sev.size() < (size_t)std::max<uint32_t>(maxdepth, 2u)) {
        hipEvent_t e;
        HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        w.sev.push_back(e);
    }
    while (w.pass_ev.size() < 2 * (size_t)std::max<uint32_t>(maxdepth, 2u)) {
        hipEvent_t e;
        HIPCHK(hipEventCreate(&e));
        w.pass_ev.push_back(e);
    }
    w.cap = cap;
    w.cap_depth = maxdepth;
    return RTMI_OK;
}
// The colour stack of a call on a textured scene: one float4 beside every mstack entry of the workspace ensure_workspace has sized.
// Every other call leaves it unallocated.
static int ensure_cstack(const rtmi_scene* s, Work& w) {
    if (!s->has_tex) return RTMI_OK;
    HIPCHK(w.cstack.ensure(w.cap * (size_t)w.cap_depth));
    return RTMI_OK;
}

// Persistent grid of the octree walk kernels (trace_oct.hpp).  About 24 resident waves per CU in all is the optimum of
// this VALU-issue-bound walk (more only adds cache pressure): one stream launches what fits, two or more share the CUs with
// 16 each (two streams: 12 / 14 / 16 / 17 / 18 / 20 / 24 waves per launch = 929 / 962 / 980 / 985 / 971 / 965 / 955 Mrays/s;
// one stream: 16 / 20 / 24 = 808 / 882 / 931).
static dim3 oct_grid(const rtmi_scene* s) {
    const int per_cu = s->tune.oct_waves_per_cu ? (int)s->tune.oct_waves_per_cu
                                                 : s->active_streams > 1 ? std::min(s->oct_blocks_per_cu, 16) : s->oct_blocks_per_cu;
    return dim3((unsigned)(s->num_cu * per_cu));
}

// The octree walk kernels of trace_oct.hpp as [count][fast] of their <bool COUNT, bool FAST> templates.  A batch's path
// kernels follow its sampling mode (shade.hpp): k_path_primary / k_path_slow for Samp::FRAME, the *_samples kernels for
// PASS, the *_list kernels for LIST and the *_views kernels for VIEWS; these two take the list or the view table as one more
// argument and so have function types of their own.
#define RTMI_COUNT_FAST(k) {{k<false, false>, k<false, true>}, {k<true, false>, k<true, true>}}
typedef void (*WalkKernel)(DScene, OctArgs, DCtrl*, int, int);
typedef void (*ListWalkKernel)(DScene, OctArgs, DCtrl*, int, int, const uint32_t*);
static const WalkKernel trace_oct_variant[2][2] = RTMI_COUNT_FAST(k_trace_oct);
typedef void (*OcclWalkKernel)(DScene, OctArgs, DCtrl*, int, int, OcclArgs);
static const OcclWalkKernel occluded_oct_variant[2][2] = RTMI_COUNT_FAST(k_occluded_oct);
// (first index of the path kernels: 0 = primary, 1 = slow, 2 = primary with the node cull)
static const WalkKernel path_variant[3][2][2][2] = {  // [which][mode == Samp::PASS][count][fast]
    {RTMI_COUNT_FAST(k_path_primary), RTMI_COUNT_FAST(k_path_primary_samples)},
    {RTMI_COUNT_FAST(k_path_slow), RTMI_COUNT_FAST(k_path_slow_samples)},
    {RTMI_COUNT_FAST(k_path_primary_cull), RTMI_COUNT_FAST(k_path_primary_samples_cull)}};
static const ListWalkKernel path_list_variant[3][2][2] = {RTMI_COUNT_FAST(k_path_primary_list), RTMI_COUNT_FAST(k_path_slow_list),
                                                          RTMI_COUNT_FAST(k_path_primary_list_cull)};
typedef void (*ViewsWalkKernel)(DScene, OctArgs, DCtrl*, int, int, ViewTab);
static const ViewsWalkKernel path_views_variant[3][2][2] = {RTMI_COUNT_FAST(k_path_primary_views), RTMI_COUNT_FAST(k_path_slow_views),
                                                            RTMI_COUNT_FAST(k_path_primary_views_cull)};

static void launch_trace(rtmi_scene* s, Work& w, hipStream_t st, const float4* qo, const float4* qd, int pass, bool count, hipEvent_t stop) {
    // `stop` is recorded right after the closest-hit kernel, so that the event pair of the caller times exactly
    // the kernel rocprofv3 lists as k_trace_oct / k_trace_linear / k_trace (a hybrid pass: its three launches)
    // Hybrid pass (hybrid.hpp): an exact octree with a direction table, a usable BVH, none of the options that select another
    // walk, a workspace with a fallback list as long as its hit records.  A counting launch walks the octree as ever and then
    // runs the hybrid into scratch records for the referee.
    const bool hybrid = s->hybrid && s->octree && s->d.cert && s->bvh_ok && !s->root_is_leaf &&
                        !(s->options & (RTMI_OPT_GENERIC | RTMI_OPT_FAST | RTMI_OPT_BVH)) && w.fb.p && w.fb.n >= w.hit_tf.n;
    auto launch_hybrid = [&](uint32_t* tf, float* ht, int add_rays) {
        const dim3 grid((unsigned)(s->num_cu * s->bvh_blocks_per_cu)), block(64);
        hipLaunchKernelGGL(k_hybrid_bvh, grid, block, s->bvh_lds, st, s->d, s->bnodes.p, s->bleaves.p, s->bvh_root, qo, qd, w.ctrl.p, pass, tf, ht,
                           (int)(pass == 0 ? s->tune.refill_min0 : s->tune.refill_min), w.fb.p, add_rays, s->hybrid_omax);
        hipLaunchKernelGGL(k_oct_verify, dim3((unsigned)(s->num_cu * 8)), dim3(256), 0, st, s->d, s->nfn, qo, qd, w.ctrl.p, pass, tf, ht, w.fb.p);
        OctArgs a{};
        a.qo = qo; a.qd = qd; a.hit_tf = tf; a.hit_t = ht; a.pass = pass;
        a.vote_s = pass == 0 ? s->vote[0] : s->vote[2]; a.vote_l = pass == 0 ? s->vote[1] : s->vote[3];
        a.bcn = s->block_cull_n;
        hipLaunchKernelGGL(k_trace_oct_list, oct_grid(s), dim3(64), oct_launch_lds(s, false), st, s->d, a, w.ctrl.p,
                           (int)(pass == 0 ? s->tune.refill_min0 : s->tune.refill_min),
                           (int)(s->tune.xcd_aware % 3u), (const uint32_t*)w.fb.p);
    };
    if (hybrid && !count) {
        launch_hybrid(w.hit_tf.p, w.hit_t.p, 1);
    } else if ((s->options & RTMI_OPT_BVH) && s->bvh_ok) {
        const dim3 grid((unsigned)(s->num_cu * s->bvh_blocks_per_cu)), block(64);
        hipLaunchKernelGGL(count ? k_trace_bvh<true> : k_trace_bvh<false>, grid, block, s->bvh_lds, st, s->d, s->bnodes.p, s->bleaves.p,
                           s->bvh_root, qo, qd, w.ctrl.p, pass, w.hit_tf.p, w.hit_t.p, (int)(pass == 0 ? s->tune.refill_min0 : s->tune.refill_min));
    } else if (s->root_is_leaf && !(s->options & RTMI_OPT_GENERIC)) {
        hipLaunchKernelGGL(count ? k_trace_linear<true> : k_trace_linear<false>, dim3((unsigned)(s->num_cu * 8)), dim3(256), 0, st, s->d,
                           qo, qd, w.ctrl.p, pass, w.hit_tf.p, w.hit_t.p);
    } else if (s->octree && !(s->options & RTMI_OPT_GENERIC)) {
        const int refill = (int)(pass == 0 ? s->tune.refill_min0 : s->tune.refill_min);
        const int xcd = (int)(s->tune.xcd_aware % 3u);  // 1 = ranges by XCC_ID, 2 = by blockIdx % 8, 0 = one range
        OctArgs a{};
        a.qo = qo; a.qd = qd; a.hit_tf = w.hit_tf.p; a.hit_t = w.hit_t.p; a.pass = pass;
        a.vote_s = pass == 0 ? s->vote[0] : s->vote[2]; a.vote_l = pass == 0 ? s->vote[1] : s->vote[3];
        a.bcn = s->block_cull_n;
        hipLaunchKernelGGL(trace_oct_variant[count][(s->options & RTMI_OPT_FAST) != 0], oct_grid(s), dim3(64), oct_launch_lds(s, count), st,
                           s->d, a, w.ctrl.p, refill, xcd);
    } else {
        // persistent grid: enough blocks to fill every CU at the occupancy LDS allows
        const int per_cu = s->trace_block == 256 ? 4 : 16;
        const dim3 grid((unsigned)(s->num_cu * per_cu)), block((unsigned)s->trace_block);
        hipLaunchKernelGGL(count ? k_trace<true> : k_trace<false>, grid, block, s->trace_lds, st, s->d, qo, qd, w.ctrl.p, pass,
                           w.hit_tf.p, w.hit_t.p);
    }
    (void)hipEventRecord(stop, st);
    if (hybrid && count && w.ref_tf.ensure(w.hit_tf.n) == hipSuccess && w.ref_t.ensure(w.hit_tf.n) == hipSuccess) {
        // the referee of the counting build: the same pass once more through the hybrid, into scratch records, and every record
        // the hybrid stands by against the exact walk's (the queue's "Rays" were counted by the walk above, not again)
        launch_hybrid(w.ref_tf.p, w.ref_t.p, 0);
        hipLaunchKernelGGL(k_hybrid_referee, dim3((unsigned)(s->num_cu * 8)), dim3(256), 0, st, w.ctrl.p, pass, w.hit_tf.p, w.hit_t.p, w.ref_tf.p,
                           w.ref_t.p);
    }
    if (s->d.nspheres)  // analytic spheres: a flat list against every ray, after the tree (not part of the timed trace kernel)
        hipLaunchKernelGGL(k_trace_spheres, dim3((unsigned)(s->num_cu * 8)), dim3(256), 0, st, s->d, qo, qd, w.ctrl.p, pass, w.hit_tf.p, w.hit_t.p);
}
// rtmi_occluded*'s scene dispatch.  An exact octree and the linear list have any-hit kernels; everything else (generic tree,
// RTMI_OPT_GENERIC, BVH mode, analytic spheres) runs its closest-hit launch of rtmi_trace followed by an elementwise kernel.
static bool occluded_anyhit(const rtmi_scene* s) {
    const bool bvh = (s->options & RTMI_OPT_BVH) && s->bvh_ok, generic = (s->options & RTMI_OPT_GENERIC) != 0;
    return !bvh && !generic && s->d.nspheres == 0 && (s->root_is_leaf || s->octree) && !s->occl_from_hits;
}
// The any-hit walk of queue `pass` of the stream's control block (ctrl->count[pass] rays, set on the stream before this):
// rays qo / qd, limits tmax (null: +inf), one byte per ray to occ.  pass 0 with n rays: rtmi_occluded*.  pass 1: the AO rays
// of rtmi_render_ao*, the shadow rays of rtmi_render_light* or both kinds of rtmi_render_preview*, whose count exists on the device only (0 is a valid count); n is then an upper bound (the closest-hit fallback writes the
// workspace's hit records, sized for it).  `stop` is recorded right after the walk kernel.
// from_hits: the closest-hit launch also where an any-hit kernel exists (w then has hit records, and a fallback list for the
// hybrid pass); the answers are the same bytes.
static void launch_occluded(rtmi_scene* s, Work& w, hipStream_t st, uint64_t n, const float4* qo, const float4* qd, const float* tmax,
                            uint8_t* occ, int pass, hipEvent_t stop, bool from_hits = false) {
    const bool count = (s->options & RTMI_OPT_COUNTERS) != 0;
    if (from_hits || !occluded_anyhit(s)) {
        launch_trace(s, w, st, qo, qd, pass, count, stop);
        const unsigned grid = (unsigned)std::min<uint64_t>((n + 255) / 256, (uint64_t)s->num_cu * 8);
        if (pass == 0)
            hipLaunchKernelGGL(k_occl_from_hits, dim3(grid), dim3(256), 0, st, (uint32_t)n, w.hit_tf.p, w.hit_t.p, tmax, occ);
        else
            hipLaunchKernelGGL(k_ao_occl_from_hits, dim3(grid), dim3(256), 0, st, w.ctrl.p, pass, w.hit_tf.p, w.hit_t.p, tmax, occ);
    } else if (s->root_is_leaf) {
        hipLaunchKernelGGL(count ? k_occluded_linear<true> : k_occluded_linear<false>, dim3((unsigned)(s->num_cu * 8)), dim3(256), 0, st, s->d,
                           qo, qd, w.ctrl.p, pass, tmax, occ);
        (void)hipEventRecord(stop, st);
    } else {
        OctArgs a{};
        a.qo = qo; a.qd = qd; a.pass = pass;
        a.vote_s = s->vote[0]; a.vote_l = s->vote[1];
        hipLaunchKernelGGL(occluded_oct_variant[count][(s->options & RTMI_OPT_FAST) != 0], oct_grid(s), dim3(64), oct_launch_lds(s, count), st,
                           s->d, a, w.ctrl.p, (int)s->tune.refill_min0, (int)(s->tune.xcd_aware % 3u), OcclArgs{tmax, occ});
        (void)hipEventRecord(stop, st);
    }
}
// where a stream's zero-component rays go; cap 0 (tuning slow_path = 0... or the queue not allocated) keeps them in place
static const SlowQ SLOW_OFF{nullptr, nullptr, nullptr, nullptr, 0u};  // no slow path: nothing is set aside (cap = 0)
static SlowQ slow_queue(rtmi_scene* s, Work& w) {
    const bool on = s->tune.slow_path_off == 0u && w.sqo.p && w.sstream;
    return SlowQ{w.sqo.p, w.sqd.p, w.sqpath.p, w.sqbounce.p, on ? RTMI_SLOW_CAP : 0u};
}
// One launch of the path kernel of the batch's sampling mode: k_path_primary* (slow = false) or k_path_slow*
static void launch_path(rtmi_scene* s, Work& w, hipStream_t st, dim3 grid, const OctArgs& a, int refill, int xcd, bool slow,
                        bool count, Samp mode, const uint32_t* list, const ViewTab& vt) {
    const bool fast = (s->options & RTMI_OPT_FAST) != 0;
    // a scene with node cull records (and so with a direction table) gets the primary kernels that use them (trace_oct.hpp)
    const int k = slow ? 1 : (s->d.fcull && s->primary_node_cull ? 2 : 0);
    if (mode == Samp::VIEWS)
        hipLaunchKernelGGL(path_views_variant[k][count][fast], grid, dim3(64), oct_launch_lds(s, count), st, s->d, a, w.ctrl.p, refill, xcd, vt);
    else if (mode == Samp::LIST)
        hipLaunchKernelGGL(path_list_variant[k][count][fast], grid, dim3(64), oct_launch_lds(s, count), st, s->d, a, w.ctrl.p, refill, xcd, list);
    else
        hipLaunchKernelGGL(path_variant[k][mode == Samp::PASS][count][fast], grid, dim3(64), oct_launch_lds(s, count), st, s->d, a, w.ctrl.p, refill, xcd);
}
// k_path_primary: the batch's primary rays generated, traced and shaded; the bounce rays go to queue 1, which pass 1 traces.
// The mirror reflections it traces itself go on in queue 2 (ping-pong buffer 0, free until pass 1's k_shade appends to it).
// `stop` is recorded right after the kernel.
static void launch_primary(rtmi_scene* s, Work& w, hipStream_t st, OctArgs a, bool count, Samp mode, const uint32_t* list,
                           const ViewTab& vt, hipEvent_t stop) {
    a.bqo = w.qo[1].p; a.bqd = w.qd[1].p; a.bqpath = w.qpath[1].p;
    a.vote_s = s->vote[0]; a.vote_l = s->vote[1];
    a.pcull = s->packet_cull;
    a.b2qo = w.qo[0].p; a.b2qd = w.qd[0].p; a.b2qpath = w.qpath[0].p;
    a.minpl = s->mirror_inplace;
    launch_path(s, w, st, oct_grid(s), a, (int)s->tune.refill_min0, (int)(s->tune.xcd_aware % 3u), false, count, mode, list, vt);
    (void)hipEventRecord(stop, st);
}
// Consumer launch k of the slow path (k_path_slow), on the side stream: after the producer on `st` whose event is sev[k]
static void launch_slow(rtmi_scene* s, Work& w, hipStream_t st, OctArgs a, uint32_t k, bool count, Samp mode, const uint32_t* list,
                        const ViewTab& vt) {
    a.slow_k = k;
    a.vote_s = s->vote[2]; a.vote_l = s->vote[3];
    (void)hipStreamWaitEvent(w.sstream, w.sev[k], 0);
    hipLaunchKernelGGL(k_slow_snapshot, dim3(1), dim3(1), 0, w.sstream, w.ctrl.p, k, a.slow.cap);
    // The ordinary stream goes on only after the snapshot: its next persistent launch and the slow-path launch then become
    // ready together and the high-priority one gets its few wave slots first.  (Without this the next launch, already
    // queued in order, took every slot while the side stream was still resolving the event, and the slow paths started
    // a whole pass late.)
    (void)hipEventRecord(w.sgo, w.sstream);
    (void)hipStreamWaitEvent(st, w.sgo, 0);
    const dim3 sgrid((unsigned)std::max(s->num_cu / 2, 1));  // one path per wave at a time; a frame has ~100 such paths, a wave takes one after the other
    launch_path(s, w, w.sstream, sgrid, a, 1, 0, true, count, mode, list, vt);
}

// The work counters of a stream's control block as stats
static rtmi_stats_t ctrl_counters(const DCtrl& h) {
    rtmi_stats_t c{};
    c.rays = h.rays;
    c.box_tests = h.counters[0]; c.tri_tests = h.counters[1]; c.full_tests = h.counters[2];
    c.nodes = h.counters[3]; c.leaves = h.counters[4];
    c.slow_paths = std::min<uint32_t>(h.scount, RTMI_SLOW_CAP);
    return c;
}
// a += the work counters of b (rays, tests, nodes, leaves, slow paths)
static void add_counters(rtmi_stats_t& a, const rtmi_stats_t& b) {
    a.rays += b.rays; a.box_tests += b.box_tests; a.tri_tests += b.tri_tests; a.full_tests += b.full_tests;
    a.nodes += b.nodes; a.leaves += b.leaves; a.slow_paths += b.slow_paths;
}

int rtmi_render_device(rtmi_scene_t* s, const rtmi_viewport_t* vp, uint64_t seed, uint32_t row0, uint32_t nrows,
                       void* out_device, void* hip_stream, rtmi_stats_t* stats) {
    const rtmi_tile_t tile{row0, nrows, nrows ? nrows : 1u, 0u};
    return rtmi_render_tile_device(s, vp, seed, &tile, out_device, hip_stream, stats);
}

// One sub-tile = every nsub-th stripe of the caller's tile, rendered on its own stream with its own workspace.
struct SubTile {
    DView dv;          // row mapping of the sub-tile's local rows (tile_pixel)
    uint64_t npix = 0; // pixels of the sub-tile
    uint32_t base = 0;  // adaptive passes: the sub-tile's first entry of the active-pixel list
};
// An adaptive pass (rtmi_render_adaptive*): the n pixels of `list` (tile-local pixel indices, ascending), each with the same
// number of samples behind it; sumsq / counts continue beside the call's accum.
struct ListPass { const uint32_t* list; uint32_t n; float4* sumsq; uint32_t* counts; };
// The outputs of a features call (rtmi_render_features*): one float4 / float4 / uint32 per pixel of the tile, each may be null
struct FeatOut { float4* albedo; float4* normal; uint32_t* ids; };
// An ambient-occlusion call (rtmi_render_ao*): its parameters and its output, one f32 per pixel of the tile
struct AoCall { rtmi_ao_t p; float* out; };
// A direct-light call (rtmi_render_light*): its parameters and its two planes, one f32 per pixel of the tile, either may be null
struct LightCall { rtmi_light_t p; float* shadow; float* irradiance; };
// A preview call (rtmi_render_preview*): its parameters as the kernels take them, the entries a path may queue (Ka + sum K_l)
// and its outputs, each may be null (shadow / irradiance: nlights planes of `plane` floats)
struct PreviewCall {
    PvArgs a;
    uint32_t per_path;
    float4* color; FeatOut fo; float* ao; float* shadow; float* irradiance;
    size_t plane;
};
// A shadowed path-trace (rtmi_render_shadowed*): the light every surface hit of every bounce is tested against
// el != nullptr: an envlight path-trace (rtmi_render_envlight*), the same pass structure with k_envlight_rays and k_shade_envlight;
// p is then an unbounded light that is never read beyond its flags (no tmax)
// lit != nullptr: a lit path-trace (rtmi_render_lit*), the same pass structure with k_lit_rays and k_shade_lit and up to
// lit->nlights shadow rays per path and pass; p is then never read
// em != nullptr: an emissive path-trace (rtmi_render_emissive*), the same pass structure with k_emissive_rays and k_shade_emissive,
// whose walk is the scene's closest-hit launch into the shadow queue's own hit records; p is then never read
struct ShadowCall { rtmi_light_t p; const rtmi_envlight_t* el = nullptr; const LitArgs* lit = nullptr; const EmTab* em = nullptr; };
// A camera call (rtmi_render_camera*): the model k_gen_camera generates the rays of, and the guides of those rays (each may be null)
struct CameraCall { DCam cam; FeatOut fo; };
// One render_tile call: what it renders, and its plan (plan_tile)
struct TileCall {
    uint64_t seed;
    uint32_t sample0, spp, maxdepth, W;  // spp: samples per pixel of this call
    float4 *accum, *out;
    const ListPass* lp;
    const FeatOut* fo;  // a features call: the primary pass alone (maxdepth = 1, per-pass pipeline), k_features for k_shade + k_accum
    const AoCall* ao;   // an AO call: a features call's primary pass, then k_ao_rays, the any-hit walk of queue 1 and k_ao_resolve
    const LightCall* li;  // a direct-light call: likewise with k_light_rays and k_light_resolve
    const PreviewCall* pv;  // a preview call: the primary pass once, k_preview_rays, one walk of queue 1, k_preview_resolve
    const ShadowCall* sh;  // a shadowed path-trace: a progressive pass (accum) of the per-pass pipeline with k_shadow_rays, an any-hit walk and k_shade_shadowed per bounce pass
    const CameraCall* cam;  // a camera call: a progressive pass (accum) of the per-pass pipeline, or a features call (fo), with k_gen_camera for k_gen_samples; k_features after pass 0 when cam->fo asks
    ViewTab vt;  // VIEWS: the view table (cams == nullptr otherwise)
    Samp mode;  // LIST with lp, PASS with accum, fo, ao, li or pv, VIEWS with vt.cams, FRAME otherwise
    bool counting, path_kernels;
    uint32_t nsub;
    uint64_t pix_per_batch, max_npix;  // max_npix: pixels of the largest sub-tile
    SubTile sub[RTMI_MAX_STREAMS];
};
// What the batches of a call add up to: work counters, closest-hit launches and their times
struct TileSums {
    rtmi_stats_t counters{};
    float trace_ms = 0.f, primary_ms = 0.f, bounce_ms = 0.f;
    uint32_t launches = 0;
    uint64_t ao_hits = 0;  // AO calls: samples whose primary ray hit
};

// Checks of a render call's viewport and tile (nrows >= 1), before any HIP call
static int check_view(const rtmi_viewport_t* vp, const rtmi_tile_t* tile) {
    const uint32_t row0 = tile->row0, nrows = tile->nrows;
    if (vp->width == 0 || vp->height == 0) return fail(RTMI_ERR_INVALID, "empty viewport");
    if (tile->stripe_rows == 0) return fail(RTMI_ERR_INVALID, "stripe_rows must be >= 1");
    const uint64_t nstripes = ((uint64_t)nrows + tile->stripe_rows - 1) / tile->stripe_rows;
    const uint64_t last_row = (uint64_t)row0 + (nstripes - 1) * tile->stripe_step + ((uint64_t)nrows - 1 - (nstripes - 1) * tile->stripe_rows);
    if (last_row >= vp->height) return fail(RTMI_ERR_INVALID, "row range outside the viewport");
    if (nstripes > 1 && tile->stripe_step < tile->stripe_rows) return fail(RTMI_ERR_INVALID, "stripes overlap");
    if (vp->samples_per_pixel == 0) return fail(RTMI_ERR_INVALID, "samples_per_pixel must be >= 1");  // reference: 1/0 -> NaN image
    if (vp->maxdepth > RTMI_MAX_PASSES) return fail(RTMI_ERR_UNSUPPORTED, "maxdepth above 32");
    if ((uint64_t)vp->width * vp->height >= (1ull << 32)) return fail(RTMI_ERR_UNSUPPORTED, "more than 2^32 pixels");
    return RTMI_OK;
}

// The shading level of a scene (Shade, shade.hpp): THE place that reads the has_* flags to choose kernels.  Each feature's kernels
// know every earlier feature, so the level is the latest feature the scene has, and a table of a lower level that the scene lacks is
// passed empty (envtab.n = 0, smoothtab.n = 0).  Only Shade::PLAIN renders with the path kernels (plan_tile): k_path_slow has no
// arm for any level above it.
static Shade shade_level(const rtmi_scene* s) {
    if (s->has_nmap) return Shade::NMAP;  // (a scene with normal maps has textures)
    if (s->has_tex) return Shade::TEX;
    if (s->has_normals) return Shade::SMOOTH;
    if (s->has_env) return Shade::ENV;
    if (s->has_dielectric) return Shade::GLASS;
    return Shade::PLAIN;
}

// The shading launch of pass `pass` of a batch on workspace w, THE launch site of the 30 k_shade* kernels: the kernel of (mode,
// shade_level(s)) shades the rays (qo, qd) of queue pass & 1 -- pass 0 of explicit rays has them where the caller put them -- into
// the other queue and scol.  list, vt: the mode's own argument (LIST: the pixel list; RAYS: the batch's RNG keys or null; VIEWS:
// the view table).  The level's tables are appended here.  Every launch is a typed call: an argument list that does not fit its
// kernel does not compile.
static void launch_shade(rtmi_scene* s, Work& w, hipStream_t st, Samp mode, const DView& dv, uint64_t seed, uint32_t pix0, uint32_t npaths,
                         uint32_t pass, const float4* qo, const float4* qd, float4* scol, const SlowQ& slow, const uint32_t* list = nullptr,
                         const ViewTab& vt = ViewTab{}) {
    const int a = pass & 1, b = a ^ 1;
    const dim3 grid((unsigned)(s->num_cu * 8)), block(256);
    // a mode's six kernels in level order (RTMI_SHADE_ROW), then the mode's own argument
    auto row = [&](auto plain, auto glass, auto env, auto smooth, auto tex, auto nmap, auto... m) {
        auto go = [&](auto k, auto... tail) {
            hipLaunchKernelGGL(k, grid, block, 0, st, s->d, dv, seed, pix0, npaths, (int)pass, qo, qd, w.qpath[a].p, w.hit_tf.p, w.hit_t.p,
                               w.qo[b].p, w.qd[b].p, w.qpath[b].p, w.mstack.p, scol, w.ctrl.p, slow, m..., tail...);
        };
        switch (shade_level(s)) {
        case Shade::PLAIN: go(plain); break;
        case Shade::GLASS: go(glass); break;
        case Shade::ENV: go(env, s->envtab); break;
        case Shade::SMOOTH: go(smooth, s->envtab, s->smoothtab); break;
        case Shade::TEX: go(tex, s->envtab, s->smoothtab, s->textab, w.cstack.p); break;
        case Shade::NMAP: go(nmap, s->envtab, s->smoothtab, s->textab, w.cstack.p, s->nmaptab); break;
        }
    };
    switch (mode) {
    case Samp::FRAME: row(RTMI_SHADE_ROW(k_shade)); break;
    case Samp::PASS: row(RTMI_SHADE_ROW(k_shade_samples)); break;
    case Samp::LIST: row(RTMI_SHADE_ROW(k_shade_list), list); break;
    case Samp::VIEWS: row(RTMI_SHADE_ROW(k_shade_views), vt); break;
    case Samp::RAYS: row(RTMI_SHADE_ROW(k_shade_rays), list); break;
    }
}

// The feature kernel of the scene's level on the hit records of the primary queue (qo, qd): the queue is still intact at every site
// that calls this (the shading of pass 0 writes the OTHER queue).  Glass and the environment do not show in a first hit's features.
static void launch_features(rtmi_scene* s, dim3 grid, dim3 block, hipStream_t st, uint32_t npixels, uint32_t nsamples, const uint32_t* hit_tf,
                            const float* hit_t, float* albedo, float* normal, uint32_t* ids, uint32_t pix0, uint32_t W, uint32_t nsub, uint32_t sub,
                            const float4* qo, const float4* qd) {
    auto go = [&](auto k, auto... tail) {
        hipLaunchKernelGGL(k, grid, block, 0, st, s->d, npixels, nsamples, hit_tf, hit_t, albedo, normal, ids, pix0, W, nsub, sub,
                           make_fastdiv(W), make_fastdiv(nsamples), tail...);
    };
    switch (shade_level(s)) {
    case Shade::PLAIN:
    case Shade::GLASS:
    case Shade::ENV: go(k_features); break;
    case Shade::SMOOTH: go(k_features_smooth, qo, qd, s->smoothtab); break;
    case Shade::TEX: go(k_features_tex, qo, qd, s->smoothtab, s->textab); break;
    case Shade::NMAP: go(k_features_nmap, qo, qd, s->smoothtab, s->textab, s->nmaptab); break;
    }
}

// An envlight call walks its shadow rays with the scene's closest-hit launch on an octree: they leave a hit in every direction
// the map is bright in, most of them escape, and an escaping ray costs the any-hit octree walk (k_occluded_oct) a full
// traversal where the hybrid pass (hybrid.hpp) settles it in the BVH.  Measured on the canonical 2048 x 2048 frame: 39.4 ms of
// k_occluded_oct per 16 samples for 10 M shadow rays, against 26 ms of closest-hit launches for the 94 M path rays
// (profiles/envlight_kernel_stats_anyhit.csv).  The linear list keeps its any-hit kernel, which stops at the first hit.
static bool envlight_from_hits(const rtmi_scene* s, const TileCall& c) { return c.sh && c.sh->el && !s->root_is_leaf; }
// A lit call walks its shadow rays with the scene's closest-hit launch on an octree too, although they end at a lamp and four in
// ten of them meet an occluder, where the any-hit kernel stops: measured on the canonical 2048 x 2048 frame with lights A + B,
// 20.4 M shadow rays per 16 samples cost k_occluded_oct 59.9 ms and the hybrid pass 12.2 ms on top of the path rays' 26.3 ms
// (profiles/lit_kernel_stats_anyhit.csv against lit_kernel_stats.csv).  RTMI_LIT_FROM_HITS=0 brings the any-hit
// kernel back for that comparison; the answers are the same bytes.  The linear list keeps its any-hit kernel.
// The kernel set of a lit call: the *_surf kernels (lit.hpp) for a scene with a surface feature, today's for every other.  Levels
// PLAIN and ENV take the old set unless the scene has a dielectric, which Shade::ENV's kernels know and the old lit kernels do not.
static bool lit_surfaces(const rtmi_scene* s) { return shade_level(s) >= Shade::SMOOTH || s->has_dielectric; }
static bool lit_from_hits(const rtmi_scene* s, const TileCall& c) { return c.sh && c.sh->lit && s->lit_from_hits && !s->root_is_leaf; }

// The plan of a call: its streams, their sub-tiles and the batch size, with every stream's workspace sized for it.
static int plan_tile(rtmi_scene* s, const rtmi_viewport_t* vp, const rtmi_tile_t* tile, TileCall& c) {
    const uint32_t nrows = tile->nrows, spp = c.spp;
    const uint64_t npix = (uint64_t)nrows * c.W;
    // ---- the tile's rows dealt out to the streams one row at a time (sub-tile t = rows t, t + nsub, ... of the tile): equal
    //      shares whatever the tile's own striping is.  (Round 2 dealt out whole stripes: with the 16-row stripes of an
    //      8-rank tiling a stream's stripes repeat every 384 image rows, the teapot covers two such periods and the slowest
    //      stream of a rank carried up to 12 % more rays than the others.)
    // path kernels (pipeline 3; 0 = automatic): exact-octree scenes get pass 0 from k_path_primary, which generates, traces and
    // shades the primary rays in one kernel.  Everything else (pipeline 1, linear list, generic tree, BVH mode,
    // analytic spheres) starts with k_gen.  Both then run one closest-hit + one shading launch per bounce pass.
    c.path_kernels = !c.fo && !c.ao && !c.li && !c.pv && !c.sh && !c.cam && s->tune.pipeline != 1u && s->octree && !s->root_is_leaf &&
                     !(s->options & (RTMI_OPT_GENERIC | RTMI_OPT_BVH)) && s->d.nspheres == 0 && shade_level(s) == Shade::PLAIN;
    // streams = 0 (automatic): one stream for path-kernel tiles of 2^26 paths and more, three otherwise (the per-pass
    // pipelines -- BVH mode: 29.6 ms on three streams, 35.2 on one -- have elementwise kernels to hide).  Since k_shade stopped being
    // atomic-bound (round 3) there is little left for a second stream to hide: the full config-3 frame takes 366.9 ms on one
    // stream and 371.8 on three (the sub-tiles' persistent launches compete for the same wave slots); a 1/8 tile 52.1 vs 51.6.
    // adaptive passes: sized from the pass's own pixels, lp->n.  A refinement pass (fewer pixels than the tile) takes one
    // stream: on config 3 its few hundred thousand pixels ran 6 % faster over the whole call on one stream than on three,
    // and no slower at the other tolerances measured.
    const ListPass* lp = c.lp;
    const uint64_t npix_call = lp ? (uint64_t)lp->n : npix;
    // features calls (c.fo): one stream at any size.  Their elementwise kernels are 3 % of the call, and on three streams a
    // sub-tile's k_features waits for wave slots behind the other sub-tiles' persistent k_trace_oct launches (config 3's frame
    // of 2^28 paths: 108.0 and 111.0 ms on one stream in two jobs, 113.9 and 113.7 on three; 2^25 paths: 16.4 and 16.3 against
    // 17.5 and 17.3).
    // AO, direct-light and preview calls (c.ao, c.li, c.pv): as features calls.
    const uint32_t auto_streams = (c.fo || c.ao || c.li || c.pv || (c.path_kernels && npix_call * spp >= (1ull << 26)) || (lp && npix_call < npix)) ? 1u : 3u;
    uint32_t nsub = std::min<uint32_t>(s->tune.streams ? s->tune.streams : auto_streams, (uint32_t)RTMI_MAX_STREAMS);
    nsub = (uint32_t)std::min<uint64_t>(nsub, lp ? npix_call : nrows);
    if (npix_call * spp < s->tune.subtile_min_paths) nsub = 1;
    s->active_streams = c.nsub = nsub;
    for (uint32_t t = 0; t < nsub; t++) {
        DView& dv = c.sub[t].dv;
        dv.orig = mk(vp->orig[0], vp->orig[1], vp->orig[2]);
        dv.cam = mk(vp->cam[0], vp->cam[1], vp->cam[2]);
        dv.vu = mk(vp->vu[0], vp->vu[1], vp->vu[2]);
        dv.vv = mk(vp->vv[0], vp->vv[1], vp->vv[2]);
        dv.width = c.W; dv.height = vp->height; dv.maxdepth = c.maxdepth; dv.spp = spp;
        dv.row0 = tile->row0; dv.stripe_rows = tile->stripe_rows; dv.stripe_step = tile->stripe_step;
        view_set_sampling(dv, c.sample0, vp->samples_per_pixel);
        dv.sub_mul = lp ? 1u : nsub; dv.sub_off = lp ? 0u : t;  // list entries are tile-local pixel indices
        view_set_divisors(dv);
        if (lp) {  // a contiguous chunk of the list: neighbouring pixels stay in the same waves
            c.sub[t].base = (uint32_t)(npix_call * t / nsub);
            c.sub[t].npix = npix_call * (t + 1) / nsub - c.sub[t].base;
        } else {
            c.sub[t].npix = (uint64_t)((nrows - t + nsub - 1) / nsub) * c.W;
        }
    }

    // batch = whole pixels with all their samples; an AO call counts a path as its K AO rays (a direct-light call: its K
    // candidates, a preview call: its Ka + sum K_l entries), so that the ray queue of a batch stays within batch_paths entries
    // and below the walk's 2^31
    const size_t want_paths = (size_t)std::max<uint64_t>(s->tune.batch_paths, 1) / nsub;
    const uint64_t per_pix = (uint64_t)spp * (c.ao ? c.ao->p.rays : c.li ? c.li->p.rays : c.pv ? std::max(c.pv->per_path, 1u) : 1u);
    uint64_t pix_per_batch = std::max<uint64_t>(1, want_paths / per_pix);
    uint64_t max_sub_npix = 0;
    for (uint32_t t = 0; t < nsub; t++) max_sub_npix = std::max(max_sub_npix, c.sub[t].npix);
    // equal batches: a sub-tile a little larger than the budget (thirds of a frame whose stripes do not divide evenly)
    // would otherwise get a full batch and a sliver with five tiny passes of its own
    if (pix_per_batch < max_sub_npix) {
        const uint64_t nb = (max_sub_npix + pix_per_batch - 1) / pix_per_batch;
        pix_per_batch = max_sub_npix * 8 <= pix_per_batch * 9 ? max_sub_npix : (max_sub_npix + nb - 1) / nb;
    }
    pix_per_batch = std::min<uint64_t>(pix_per_batch, max_sub_npix);
    // (2^30: k_path_primary keeps a path's bounce and its certificate in the two bits above the path's index)
    if (pix_per_batch * per_pix >= (1ull << 30)) return fail(RTMI_ERR_UNSUPPORTED, "batch above 2^30 paths");
    c.pix_per_batch = pix_per_batch;
    c.max_npix = max_sub_npix;
    for (uint32_t t = 0; t < nsub; t++) {
        if (c.sub[t].npix == 0) continue;
        const size_t paths = (size_t)(std::min<uint64_t>(pix_per_batch, c.sub[t].npix) * spp);
        // an AO call on a scene without an any-hit kernel: the closest-hit launch of the AO rays writes the workspace's hit records
        // (a direct-light call likewise: its candidates bound its live rays)
        const size_t nao = c.ao ? paths * c.ao->p.rays : c.li ? paths * c.li->p.rays : c.pv ? paths * c.pv->per_path : 0;
        int rc = ensure_workspace(s->w[t], nao && !occluded_anyhit(s) ? nao : paths, c.maxdepth);
        if (rc != RTMI_OK) return rc;
        rc = ensure_cstack(s, s->w[t]);
        if (rc != RTMI_OK) return rc;
        if (c.ao) {
            rtmi_scene::AoBuf& a = s->ao[t];
            HIPCHK(a.qo.ensure(nao)); HIPCHK(a.qd.ensure(nao)); HIPCHK(a.occ.ensure(nao)); HIPCHK(a.slot.ensure(paths));
            if (!std::isinf(c.ao->p.radius)) HIPCHK(a.tmax.ensure(nao));
        }
        if (c.li) {
            rtmi_scene::LightBuf& l = s->light[t];
            HIPCHK(l.qo.ensure(nao)); HIPCHK(l.qd.ensure(nao)); HIPCHK(l.c.ensure(nao)); HIPCHK(l.occ.ensure(nao)); HIPCHK(l.slot.ensure(nao));
            if (!(c.li->p.flags & RTMI_LIGHT_UNBOUNDED)) HIPCHK(l.tmax.ensure(nao));
        }
        if (c.pv) {
            rtmi_scene::PreviewBuf& b = s->pv[t];
            HIPCHK(b.qo.ensure(nao)); HIPCHK(b.qd.ensure(nao)); HIPCHK(b.tmax.ensure(nao)); HIPCHK(b.c.ensure(nao)); HIPCHK(b.occ.ensure(nao));
            HIPCHK(b.alb.ensure(paths)); HIPCHK(b.aslot.ensure(paths)); HIPCHK(b.lslot.ensure(paths * (c.pv->per_path - c.pv->a.Ka)));
        }
        if (c.sh && c.sh->lit) {  // a pass tests at most nlights rays per path: every queue of the walk holds paths * nlights entries
            rtmi_scene::ShadowBuf& b = s->shadow[t];
            const size_t nq = paths * c.sh->lit->nlights;
            HIPCHK(b.qo.ensure(nq)); HIPCHK(b.qd.ensure(nq)); HIPCHK(b.tmax.ensure(nq)); HIPCHK(b.lw.ensure(nq)); HIPCHK(b.occ.ensure(nq));
            HIPCHK(b.slot.ensure(nq)); HIPCHK(b.dstack.ensure(paths * c.maxdepth));
            HIPCHK(b.walk.ctrl.ensure(1));
            if (nq && (!occluded_anyhit(s) || lit_from_hits(s, c))) { HIPCHK(b.walk.hit_tf.ensure(nq)); HIPCHK(b.walk.hit_t.ensure(nq)); }
            if (nq && lit_from_hits(s, c)) HIPCHK(b.walk.fb.ensure(b.walk.hit_tf.n));
            while (b.walk.pass_ev.size() < 2 * (size_t)c.maxdepth) {
                hipEvent_t e;
                HIPCHK(hipEventCreate(&e));
                b.walk.pass_ev.push_back(e);
            }
        } else if (c.sh && c.sh->em) {  // one candidate per path: the shadow queue, its hit records, weights, slots and the direct stack
            rtmi_scene::ShadowBuf& b = s->shadow[t];
            HIPCHK(b.qo.ensure(paths)); HIPCHK(b.qd.ensure(paths)); HIPCHK(b.slot.ensure(paths)); HIPCHK(b.lw.ensure(paths));
            HIPCHK(b.dstack.ensure(paths * c.maxdepth)); HIPCHK(b.wb.ensure(paths));
            HIPCHK(b.walk.ctrl.ensure(1)); HIPCHK(b.walk.hit_tf.ensure(paths)); HIPCHK(b.walk.hit_t.ensure(paths));
            if (!s->root_is_leaf) HIPCHK(b.walk.fb.ensure(b.walk.hit_tf.n));  // the hybrid pass's fallback list, as long as the hit records
            while (b.walk.pass_ev.size() < 2 * (size_t)c.maxdepth) {
                hipEvent_t e;
                HIPCHK(hipEventCreate(&e));
                b.walk.pass_ev.push_back(e);
            }
        } else if (c.sh) {  // a pass tests at most one ray per path
            rtmi_scene::ShadowBuf& b = s->shadow[t];
            HIPCHK(b.qo.ensure(paths)); HIPCHK(b.qd.ensure(paths)); HIPCHK(b.slot.ensure(paths)); HIPCHK(b.mask.ensure(paths)); HIPCHK(b.occ.ensure(paths));
            if (!(c.sh->p.flags & RTMI_LIGHT_UNBOUNDED)) HIPCHK(b.tmax.ensure(paths));
            if (c.sh->el) { HIPCHK(b.lw.ensure(paths)); HIPCHK(b.dstack.ensure(paths * c.maxdepth)); HIPCHK(b.wb.ensure(paths)); }
            HIPCHK(b.walk.ctrl.ensure(1));
            if (!occluded_anyhit(s) || envlight_from_hits(s, c)) { HIPCHK(b.walk.hit_tf.ensure(paths)); HIPCHK(b.walk.hit_t.ensure(paths)); }
            if (envlight_from_hits(s, c)) HIPCHK(b.walk.fb.ensure(b.walk.hit_tf.n));  // the hybrid pass's fallback list, as long as the hit records
            while (b.walk.pass_ev.size() < 2 * (size_t)c.maxdepth) {
                hipEvent_t e;
                HIPCHK(hipEventCreate(&e));
                b.walk.pass_ev.push_back(e);
            }
        }
    }
    return RTMI_OK;
}

// verbose with counters, per-pass pipeline: what pass `pass` of stream t cost per ray (this pass's share of the counters)
static int dump_pass_counters(rtmi_scene* s, Work& w, hipStream_t st, uint32_t t, uint32_t pass) {
    DCtrl h;
    HIPCHK(hipMemcpyAsync(&h, w.ctrl.p, sizeof(DCtrl), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    unsigned long long* prev = s->vprev[t], d[13];  // d: the pass's share of counters[0..4], dbg[0..7]
    if (pass == 0) memset(prev, 0, sizeof(s->vprev[t]));
    for (int k = 0; k < 13; k++) {
        const unsigned long long cur = k < 5 ? h.counters[k] : h.dbg[k - 5];
        d[k] = cur - prev[k];
        prev[k] = cur;
    }
    const double n = h.count[pass] ? (double)h.count[pass] : 1.0;
    fprintf(stderr, "[rtmi]   stream %u pass %u per ray: box %.1f tri %.1f full %.2f nodes %.1f leaves %.1f | S-steps %.1f (util %.2f) L-steps %.1f (util %.2f)\n",
            t, pass, d[0] / n, d[1] / n, d[2] / n, d[3] / n, d[4] / n, d[6] / n, (double)d[6] / (64.0 * (d[5] ? d[5] : 1)), d[8] / n,
            (double)d[8] / (64.0 * (d[7] ? d[7] : 1)));
    return RTMI_OK;
}

// Enqueues batch p0 of sub-tile t on its stream: the primary rays (k_path_primary, or k_gen), one closest-hit and one
// shading launch per bounce pass with the slow path beside them, and the accumulation.  No host dependency inside a batch:
// queue sizes live on the device.
static int enqueue_batch(rtmi_scene* s, const TileCall& c, uint32_t t, uint64_t p0) {
    Work& w = s->w[t];
    hipStream_t st = s->istream[t];
    const DView& dv = c.sub[t].dv;
    const uint32_t np = (uint32_t)std::min<uint64_t>(c.pix_per_batch, c.sub[t].npix - p0);
    const uint32_t npaths = np * c.spp;
    const uint32_t pix0 = c.sub[t].base + (uint32_t)p0;  // local pixel index inside the sub-tile (list entry: adaptive)
    const uint32_t* list = c.mode == Samp::LIST ? c.lp->list : nullptr;
    const dim3 ew_grid((unsigned)(s->num_cu * 8)), ew_block(256);
    HIPCHK(hipMemsetAsync(w.ctrl.p, 0, sizeof(DCtrl), st));
    HIPCHK(hipEventRecord(w.ev[0], st));
    // what both path kernels (trace_oct.hpp) read: the batch's paths, their surface stacks and sample colours, the slow-path queue
    OctArgs pa{};
    pa.v = dv; pa.seed = c.seed; pa.pix0 = pix0; pa.npaths = npaths;
    pa.mstack = w.mstack.p; pa.scol = w.scol.p; pa.slow = slow_queue(s, w);
    // the slow path: zero-component rays that k_path_primary and k_shade set aside, traced beside the following passes
    const SlowQ sq = c.path_kernels ? pa.slow : SLOW_OFF;
    auto slow_after = [&](uint32_t k) {  // after producer k: k_path_primary (0) or the shading of pass k
        if (sq.cap == 0u) return;
        (void)hipEventRecord(w.sev[k], st);
        launch_slow(s, w, st, pa, k, c.counting, c.mode, list, c.vt);
    };
    uint32_t pass0 = 0;  // first pass of the per-pass loop
    if (c.path_kernels) {
        HIPCHK(hipEventRecord(w.pass_ev[0], st));
        launch_primary(s, w, st, pa, c.counting, c.mode, list, c.vt, w.pass_ev[1]);
        HIPCHK(hipGetLastError());
        slow_after(0);
        pass0 = 1;
    } else if (list) {
        hipLaunchKernelGGL(k_gen_list, ew_grid, ew_block, 0, st, dv, c.seed, pix0, npaths, w.qo[0].p, w.qd[0].p, w.qpath[0].p, w.ctrl.p, list);
    } else if (c.mode == Samp::VIEWS) {
        hipLaunchKernelGGL(k_gen_views, ew_grid, ew_block, 0, st, dv, c.seed, pix0, npaths, w.qo[0].p, w.qd[0].p, w.qpath[0].p, w.ctrl.p, c.vt);
    } else if (c.cam) {
        hipLaunchKernelGGL(k_gen_camera, ew_grid, ew_block, 0, st, dv, c.cam->cam, c.seed, pix0, npaths, w.qo[0].p, w.qd[0].p, w.qpath[0].p, w.ctrl.p);
    } else {
        hipLaunchKernelGGL(c.mode == Samp::PASS ? k_gen_samples : k_gen, ew_grid, ew_block, 0, st, dv, c.seed, pix0, npaths, w.qo[0].p,
                           w.qd[0].p, w.qpath[0].p, w.ctrl.p);
    }
    HIPCHK(hipGetLastError());  // a refused launch is reported where it happens, not at the end of the batch
    if (c.fo) {  // the primary rays' closest hits, then their per-pixel feature means: nothing is shaded, nothing bounces
        HIPCHK(hipEventRecord(w.pass_ev[0], st));
        launch_trace(s, w, st, w.qo[0].p, w.qd[0].p, 0, c.counting, w.pass_ev[1]);
        HIPCHK(hipGetLastError());
        launch_features(s, ew_grid, ew_block, st, np, c.spp, w.hit_tf.p, w.hit_t.p, (float*)c.fo->albedo, (float*)c.fo->normal, c.fo->ids, pix0,
                        c.W, c.nsub, t, w.qo[0].p, w.qd[0].p);
        HIPCHK(hipEventRecord(w.ev[1], st));
        HIPCHK(hipGetLastError());
        return RTMI_OK;
    }
    if (c.ao) {  // the primary rays' closest hits, K AO rays per hit compacted into queue 1, their any-hit walk, the per-pixel counts
        const rtmi_ao_t& p = c.ao->p;
        rtmi_scene::AoBuf& a = s->ao[t];
        float* tmax = std::isinf(p.radius) ? nullptr : a.tmax.p;  // +inf: the walk's NULL tmax
        HIPCHK(hipEventRecord(w.pass_ev[0], st));
        launch_trace(s, w, st, w.qo[0].p, w.qd[0].p, 0, c.counting, w.pass_ev[1]);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(k_ao_rays, ew_grid, ew_block, 0, st, s->d, dv, c.seed, pix0, npaths, p.rays, make_fastdiv(p.rays), p.radius, p.bias,
                           w.qo[0].p, w.qd[0].p, w.hit_tf.p, w.hit_t.p, a.qo.p, a.qd.p, tmax, a.slot.p, w.ctrl.p);
        hipLaunchKernelGGL(k_ao_count, dim3(1), dim3(1), 0, st, w.ctrl.p, p.rays);
        HIPCHK(hipEventRecord(w.pass_ev[2], st));
        launch_occluded(s, w, st, (uint64_t)npaths * p.rays, a.qo.p, a.qd.p, tmax, a.occ.p, 1, w.pass_ev[3]);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(k_ao_resolve, ew_grid, ew_block, 0, st, np, c.spp, p.rays, make_fastdiv(p.rays), a.slot.p, a.occ.p, c.ao->out, pix0,
                           c.W, c.nsub, t, make_fastdiv(c.W));
        HIPCHK(hipEventRecord(w.ev[1], st));
        HIPCHK(hipGetLastError());
        return RTMI_OK;
    }
    if (c.li) {  // the primary rays' closest hits, the live shadow rays compacted into queue 1, their any-hit walk, the per-pixel folds
        const rtmi_light_t& p = c.li->p;
        rtmi_scene::LightBuf& l = s->light[t];
        float* tmax = (p.flags & RTMI_LIGHT_UNBOUNDED) ? nullptr : l.tmax.p;  // unbounded: the walk's NULL tmax
        HIPCHK(hipEventRecord(w.pass_ev[0], st));
        launch_trace(s, w, st, w.qo[0].p, w.qd[0].p, 0, c.counting, w.pass_ev[1]);
        HIPCHK(hipGetLastError());
        // ctrl->count[1] (zero since the batch's memset) is the compaction's counter and then the walk's ray count
        hipLaunchKernelGGL(k_light_rays, ew_grid, ew_block, 0, st, s->d, dv, c.seed, pix0, npaths, p.rays, make_fastdiv(p.rays),
                           mk(p.orig[0], p.orig[1], p.orig[2]), p.len2, p.bias, w.qo[0].p, w.qd[0].p, w.hit_tf.p, w.hit_t.p, l.qo.p, l.qd.p, tmax,
                           l.c.p, l.slot.p, w.ctrl.p);
        HIPCHK(hipEventRecord(w.pass_ev[2], st));
        launch_occluded(s, w, st, (uint64_t)npaths * p.rays, l.qo.p, l.qd.p, tmax, l.occ.p, 1, w.pass_ev[3]);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(k_light_resolve, ew_grid, ew_block, 0, st, np, c.spp * p.rays, l.slot.p, l.occ.p, l.c.p, c.li->shadow,
                           c.li->irradiance, pix0, c.W, c.nsub, t, make_fastdiv(c.W));
        HIPCHK(hipEventRecord(w.ev[1], st));
        HIPCHK(hipGetLastError());
        return RTMI_OK;
    }
    if (c.pv) {  // the primary rays' closest hits ONCE (and their feature means), the AO rays and every light's live rays in queue 1, one walk, the per-pixel folds
        const PreviewCall& p = *c.pv;
        rtmi_scene::PreviewBuf& b = s->pv[t];
        HIPCHK(hipEventRecord(w.pass_ev[0], st));
        launch_trace(s, w, st, w.qo[0].p, w.qd[0].p, 0, c.counting, w.pass_ev[1]);
        HIPCHK(hipGetLastError());
        // before the walk: its closest-hit fallback writes the workspace's hit records
        if (p.fo.albedo || p.fo.normal || p.fo.ids)
            launch_features(s, ew_grid, ew_block, st, np, c.spp, w.hit_tf.p, w.hit_t.p, (float*)p.fo.albedo, (float*)p.fo.normal, p.fo.ids, pix0,
                            c.W, c.nsub, t, w.qo[0].p, w.qd[0].p);
        // ctrl->count[1] (zero since the batch's memset) is the compaction's counter and then the walk's ray count
        hipLaunchKernelGGL(k_preview_rays, ew_grid, ew_block, 0, st, s->d, dv, c.seed, pix0, npaths, p.a, w.qo[0].p, w.qd[0].p, w.hit_tf.p,
                           w.hit_t.p, b.qo.p, b.qd.p, b.tmax.p, b.c.p, b.aslot.p, b.lslot.p, b.alb.p, w.ctrl.p);
        HIPCHK(hipGetLastError());
        if (p.per_path) {
            HIPCHK(hipEventRecord(w.pass_ev[2], st));
            launch_occluded(s, w, st, (uint64_t)npaths * p.per_path, b.qo.p, b.qd.p, b.tmax.p, b.occ.p, 1, w.pass_ev[3]);
            HIPCHK(hipGetLastError());
        }
        hipLaunchKernelGGL(k_preview_resolve, ew_grid, ew_block, 0, st, np, c.spp, npaths, p.a, b.alb.p, b.aslot.p, b.lslot.p, b.occ.p, b.c.p,
                           p.color, p.ao, p.shadow, p.irradiance, p.plane, pix0, c.W, c.nsub, t, make_fastdiv(c.W));
        HIPCHK(hipEventRecord(w.ev[1], st));
        HIPCHK(hipGetLastError());
        return RTMI_OK;
    }
    if (c.sh) {  // per pass: the closest hits of path queue j, its live shadow rays compacted into shadow queue j, their any-hit walk, the shading with the answers
        const rtmi_light_t& p = c.sh->p;
        rtmi_scene::ShadowBuf& sb = s->shadow[t];
        float* tmax = (p.flags & RTMI_LIGHT_UNBOUNDED) ? nullptr : sb.tmax.p;  // unbounded: the walk's NULL tmax
        HIPCHK(hipMemsetAsync(sb.walk.ctrl.p, 0, sizeof(DCtrl), st));
        for (uint32_t pass = 0; pass < c.maxdepth; pass++) {
            const int a = pass & 1, b = a ^ 1;
            HIPCHK(hipEventRecord(w.pass_ev[2 * pass], st));
            launch_trace(s, w, st, w.qo[a].p, w.qd[a].p, (int)pass, c.counting, w.pass_ev[2 * pass + 1]);
            HIPCHK(hipGetLastError());
            // sb.walk.ctrl->count[pass + 1] (zero since the memset above) is the compaction's counter and then the walk's ray count
            if (c.sh->lit) {
                const LitArgs& la = *c.sh->lit;
                if (c.maxdepth - pass - 1u != 0u && la.nlights != 0u) {
                    if (lit_surfaces(s))
                        hipLaunchKernelGGL(k_lit_rays_surf, ew_grid, ew_block, 0, st, s->d, dv, c.seed, pix0, npaths, (int)pass, la, w.qo[a].p,
                                           w.qd[a].p, w.qpath[a].p, w.hit_tf.p, w.hit_t.p, w.ctrl.p, sb.qo.p, sb.qd.p, sb.tmax.p, sb.lw.p, sb.slot.p,
                                           sb.walk.ctrl.p, s->smoothtab, s->textab, s->nmaptab);
                    else
                        hipLaunchKernelGGL(k_lit_rays, ew_grid, ew_block, 0, st, s->d, dv, c.seed, pix0, npaths, (int)pass, la, w.qo[a].p, w.qd[a].p,
                                           w.qpath[a].p, w.hit_tf.p, w.hit_t.p, w.ctrl.p, sb.qo.p, sb.qd.p, sb.tmax.p, sb.lw.p, sb.slot.p,
                                           sb.walk.ctrl.p);
                    HIPCHK(hipEventRecord(sb.walk.pass_ev[2 * pass], st));
                    launch_occluded(s, sb.walk, st, (uint64_t)npaths * la.nlights, sb.qo.p, sb.qd.p, sb.tmax.p, sb.occ.p, (int)pass + 1,
                                    sb.walk.pass_ev[2 * pass + 1], lit_from_hits(s, c));
                    HIPCHK(hipGetLastError());
                } else {  // no candidates (the exhausted level, or no lights): no walk, an empty event pair for collect_batch
                    HIPCHK(hipEventRecord(sb.walk.pass_ev[2 * pass], st));
                    HIPCHK(hipEventRecord(sb.walk.pass_ev[2 * pass + 1], st));
                }
                if (lit_surfaces(s))
                    hipLaunchKernelGGL(k_shade_lit_surf, ew_grid, ew_block, 0, st, s->d, dv, c.seed, pix0, npaths, (int)pass, s->envtab, la.nlights,
                                       w.qo[a].p, w.qd[a].p, w.qpath[a].p, w.hit_tf.p, w.hit_t.p, sb.slot.p, sb.occ.p, sb.lw.p, w.qo[b].p, w.qd[b].p,
                                       w.qpath[b].p, w.mstack.p, sb.dstack.p, w.scol.p, w.ctrl.p, s->smoothtab, s->textab, w.cstack.p, s->nmaptab);
                else
                    hipLaunchKernelGGL(s->has_env ? k_shade_lit<true> : k_shade_lit<false>, ew_grid, ew_block, 0, st, s->d, dv, c.seed, pix0, npaths,
                                       (int)pass, s->envtab, la.nlights, w.qo[a].p, w.qd[a].p, w.qpath[a].p, w.hit_tf.p, w.hit_t.p, sb.slot.p,
                                       sb.occ.p, sb.lw.p, w.qo[b].p, w.qd[b].p, w.qpath[b].p, w.mstack.p, sb.dstack.p, w.scol.p, w.ctrl.p);
                HIPCHK(hipGetLastError());
                continue;
            }
            if (c.sh->em) {
                if (c.maxdepth - pass - 1u != 0u) {
                    hipLaunchKernelGGL(k_emissive_rays, ew_grid, ew_block, 0, st, s->d, dv, c.seed, pix0, (int)pass, *c.sh->em, w.qo[a].p, w.qd[a].p,
                                       w.qpath[a].p, w.hit_tf.p, w.hit_t.p, w.ctrl.p, sb.qo.p, sb.qd.p, sb.lw.p, sb.slot.p, sb.walk.ctrl.p);
                    HIPCHK(hipEventRecord(sb.walk.pass_ev[2 * pass], st));
                    launch_trace(s, sb.walk, st, sb.qo.p, sb.qd.p, (int)pass + 1, c.counting, sb.walk.pass_ev[2 * pass + 1]);
                    HIPCHK(hipGetLastError());
                } else {  // the exhausted level gets no sample: no candidates, no walk (an empty event pair for collect_batch)
                    HIPCHK(hipEventRecord(sb.walk.pass_ev[2 * pass], st));
                    HIPCHK(hipEventRecord(sb.walk.pass_ev[2 * pass + 1], st));
                }
                hipLaunchKernelGGL(s->has_env ? k_shade_emissive<true> : k_shade_emissive<false>, ew_grid, ew_block, 0, st, s->d, dv, c.seed, pix0,
                                   npaths, (int)pass, s->envtab, *c.sh->em, w.qo[a].p, w.qd[a].p, w.qpath[a].p, w.hit_tf.p, w.hit_t.p, sb.slot.p,
                                   sb.qd.p, sb.lw.p, sb.walk.hit_tf.p, sb.walk.hit_t.p, w.qo[b].p, w.qd[b].p, w.qpath[b].p, w.mstack.p,
                                   sb.dstack.p, sb.wb.p, w.scol.p, w.ctrl.p);
                HIPCHK(hipGetLastError());
                continue;
            }
            if (c.sh->el) {
                if (c.maxdepth - pass - 1u != 0u) {
                    hipLaunchKernelGGL(k_envlight_rays, ew_grid, ew_block, 0, st, s->d, dv, c.seed, pix0, (int)pass, s->envtab, s->envsamp,
                                       c.sh->el->bias, w.qo[a].p, w.qd[a].p, w.qpath[a].p, w.hit_tf.p, w.hit_t.p, w.ctrl.p, sb.qo.p, sb.qd.p, sb.lw.p,
                                       sb.slot.p, sb.walk.ctrl.p);
                    HIPCHK(hipEventRecord(sb.walk.pass_ev[2 * pass], st));
                    launch_occluded(s, sb.walk, st, npaths, sb.qo.p, sb.qd.p, nullptr, sb.occ.p, (int)pass + 1, sb.walk.pass_ev[2 * pass + 1],
                                    envlight_from_hits(s, c));
                    HIPCHK(hipGetLastError());
                } else {  // the exhausted level gets no sample: no candidates, no walk (an empty event pair for collect_batch), and
                          // k_shade_envlight does not read the slots
                    HIPCHK(hipEventRecord(sb.walk.pass_ev[2 * pass], st));
                    HIPCHK(hipEventRecord(sb.walk.pass_ev[2 * pass + 1], st));
                }
                hipLaunchKernelGGL(k_shade_envlight, ew_grid, ew_block, 0, st, s->d, dv, c.seed, pix0, npaths, (int)pass, s->envtab, s->envsamp,
                                   w.qo[a].p, w.qd[a].p, w.qpath[a].p, w.hit_tf.p, w.hit_t.p, sb.slot.p, sb.occ.p, sb.lw.p, w.qo[b].p, w.qd[b].p,
                                   w.qpath[b].p, w.mstack.p, sb.dstack.p, sb.wb.p, w.scol.p, w.ctrl.p);
                HIPCHK(hipGetLastError());
                continue;
            }
            hipLaunchKernelGGL(k_shadow_rays, ew_grid, ew_block, 0, st, s->d, dv, c.seed, pix0, (int)pass, mk(p.orig[0], p.orig[1], p.orig[2]),
                               p.len2, p.bias, w.qo[a].p, w.qd[a].p, w.qpath[a].p, w.hit_tf.p, w.hit_t.p, w.ctrl.p, sb.qo.p, sb.qd.p, tmax,
                               sb.slot.p, sb.walk.ctrl.p);
            HIPCHK(hipEventRecord(sb.walk.pass_ev[2 * pass], st));
            launch_occluded(s, sb.walk, st, npaths, sb.qo.p, sb.qd.p, tmax, sb.occ.p, (int)pass + 1, sb.walk.pass_ev[2 * pass + 1]);
            HIPCHK(hipGetLastError());
            hipLaunchKernelGGL(k_shade_shadowed, ew_grid, ew_block, 0, st, s->d, dv, c.seed, pix0, npaths, (int)pass, w.qo[a].p, w.qd[a].p,
                               w.qpath[a].p, w.hit_tf.p, w.hit_t.p, sb.slot.p, sb.occ.p, w.qo[b].p, w.qd[b].p, w.qpath[b].p, w.mstack.p,
                               sb.mask.p, w.scol.p, w.ctrl.p);
            HIPCHK(hipGetLastError());
        }
        hipLaunchKernelGGL(k_accum_samples, ew_grid, ew_block, 0, st, np, c.spp, c.sample0, w.scol.p, (float*)c.accum, (float*)c.out,
                           pix0, c.W, c.nsub, t, make_fastdiv(c.W));
        HIPCHK(hipEventRecord(w.ev[1], st));
        HIPCHK(hipGetLastError());
        return RTMI_OK;
    }
    for (uint32_t pass = pass0; pass < c.maxdepth; pass++) {
        const int a = pass & 1;
        HIPCHK(hipEventRecord(w.pass_ev[2 * pass], st));
        launch_trace(s, w, st, w.qo[a].p, w.qd[a].p, (int)pass, c.counting, w.pass_ev[2 * pass + 1]);
        HIPCHK(hipGetLastError());
        if (pass == 0 && c.cam && (c.cam->fo.albedo || c.cam->fo.normal || c.cam->fo.ids))  // the guides, before pass 1 rewrites the hit records
            launch_features(s, ew_grid, ew_block, st, np, c.spp, w.hit_tf.p, w.hit_t.p, (float*)c.cam->fo.albedo, (float*)c.cam->fo.normal,
                            c.cam->fo.ids, pix0, c.W, c.nsub, t, w.qo[a].p, w.qd[a].p);
        if (c.counting && s->verbose && !c.path_kernels) {
            int rc = dump_pass_counters(s, w, st, t, pass);
            if (rc != RTMI_OK) return rc;
        }
        launch_shade(s, w, st, c.mode, dv, c.seed, pix0, npaths, pass, w.qo[a].p, w.qd[a].p, w.scol.p, sq, list, c.vt);
        HIPCHK(hipGetLastError());
        if (pass + 1 < c.maxdepth) {  // the last pass's shading emits no rays
            slow_after(pass);
            HIPCHK(hipGetLastError());
        }
    }
    if (sq.cap != 0u) {  // the sample colours of the slow paths must be there before k_accum
        HIPCHK(hipEventRecord(w.sdone, w.sstream));
        HIPCHK(hipStreamWaitEvent(st, w.sdone, 0));
    }
    switch (c.mode) {
    case Samp::FRAME:
    case Samp::VIEWS:  // the stacked tile: k_accum does not know about views
        hipLaunchKernelGGL(k_accum, ew_grid, ew_block, 0, st, np, c.spp, w.scol.p, (float*)c.out, pix0, c.W, c.nsub, t, make_fastdiv(c.W));
        break;
    case Samp::PASS:
        hipLaunchKernelGGL(k_accum_samples, ew_grid, ew_block, 0, st, np, c.spp, c.sample0, w.scol.p, (float*)c.accum, (float*)c.out,
                           pix0, c.W, c.nsub, t, make_fastdiv(c.W));
        break;
    case Samp::LIST:
        hipLaunchKernelGGL(k_accum_list, ew_grid, ew_block, 0, st, np, c.spp, c.sample0, w.scol.p, (float*)c.accum, (float*)c.lp->sumsq,
                           c.lp->counts, (float*)c.out, list, pix0);
        break;
    case Samp::RAYS:  // never a tile's mode: explicit rays have their own driver (render_rays)
        break;
    }
    HIPCHK(hipEventRecord(w.ev[1], st));
    HIPCHK(hipGetLastError());
    return RTMI_OK;
}

// Collects batch p0 of sub-tile t once its stream has finished it: the work counters, and the closest-hit launch of every
// pass (k_path_primary for pass 0 of the path kernels) with its time
static int collect_batch(rtmi_scene* s, const TileCall& c, uint32_t t, uint64_t p0, TileSums& sum) {
    Work& w = s->w[t];
    DCtrl h;
    HIPCHK(hipMemcpyAsync(&h, w.ctrl.p, sizeof(DCtrl), hipMemcpyDeviceToHost, s->istream[t]));
    HIPCHK(hipStreamSynchronize(s->istream[t]));
    add_counters(sum.counters, ctrl_counters(h));
    for (uint32_t pass = 0; pass < c.maxdepth; pass++) {
        float pm = 0.f;
        HIPCHK(hipEventElapsedTime(&pm, w.pass_ev[2 * pass], w.pass_ev[2 * pass + 1]));
        sum.launches++;
        sum.trace_ms += pm;
        if (c.path_kernels) { if (pass == 0) sum.primary_ms += pm; else sum.bounce_ms += pm; }
        if (c.ao || c.li || c.pv || c.sh) sum.primary_ms += pm;
        if (s->verbose) fprintf(stderr, "[rtmi] stream %u batch@%llu pass %u: %u rays, trace %.3f ms, %.1f Mrays/s\n", t, (unsigned long long)p0, pass, h.count[pass], pm, h.count[pass] / (pm * 1e3));
    }
    if (c.ao) {  // the AO rays' walk: queue 1
        float pm = 0.f;
        HIPCHK(hipEventElapsedTime(&pm, w.pass_ev[2], w.pass_ev[3]));
        sum.launches++;
        sum.trace_ms += pm;
        sum.bounce_ms += pm;
        sum.ao_hits += h.count[RTMI_AO_HITS];
        if (s->verbose) fprintf(stderr, "[rtmi] stream %u batch@%llu AO: %u rays, walk %.3f ms, %.1f Mrays/s\n", t, (unsigned long long)p0, h.count[1], pm, h.count[1] / (pm * 1e3));
    }
    if (c.li) {  // the shadow rays' walk: queue 1
        float pm = 0.f;
        HIPCHK(hipEventElapsedTime(&pm, w.pass_ev[2], w.pass_ev[3]));
        sum.launches++;
        sum.trace_ms += pm;
        sum.bounce_ms += pm;
        if (s->verbose) fprintf(stderr, "[rtmi] stream %u batch@%llu light: %u live rays, walk %.3f ms\n", t, (unsigned long long)p0, h.count[1], pm);
    }
    if (c.sh) {  // the shadow rays' walks, one per pass: their control block's rays and work counters, their times
        Work& sw = s->shadow[t].walk;
        DCtrl hs;
        HIPCHK(hipMemcpyAsync(&hs, sw.ctrl.p, sizeof(DCtrl), hipMemcpyDeviceToHost, s->istream[t]));
        HIPCHK(hipStreamSynchronize(s->istream[t]));
        add_counters(sum.counters, ctrl_counters(hs));
        for (uint32_t pass = 0; pass < c.maxdepth; pass++) {
            float pm = 0.f;
            HIPCHK(hipEventElapsedTime(&pm, sw.pass_ev[2 * pass], sw.pass_ev[2 * pass + 1]));
            sum.launches++;
            sum.trace_ms += pm;
            sum.bounce_ms += pm;
            if (s->verbose) fprintf(stderr, "[rtmi] stream %u batch@%llu pass %u shadow: %u live rays, walk %.3f ms\n", t, (unsigned long long)p0, pass, hs.count[pass + 1], pm);
        }
    }
    if (c.pv && c.pv->per_path) {  // the one walk of the AO rays and every light's live rays: queue 1
        float pm = 0.f;
        HIPCHK(hipEventElapsedTime(&pm, w.pass_ev[2], w.pass_ev[3]));
        sum.launches++;
        sum.trace_ms += pm;
        sum.bounce_ms += pm;
        if (s->verbose) fprintf(stderr, "[rtmi] stream %u batch@%llu preview: %u secondary rays, walk %.3f ms\n", t, (unsigned long long)p0, h.count[1], pm);
    }
    return RTMI_OK;
}

// Samples [sample0, sample0 + nsamples) of every pixel of the tile.  accum == nullptr: the whole frame (0, S) into out_device
// (Samp::FRAME, rtmi_render_tile_device).  Otherwise a progressive pass (Samp::PASS, rtmi_render_samples_device): the running
// per-pixel sums continue in accum, out_device (optional) receives the preview.  Batches and automatic streams are sized
// from the paths of THIS call, npix * nsamples.
// lp != nullptr (with accum): an adaptive pass over the pixels of lp->list (Samp::LIST), dealt out to the streams in
// contiguous chunks of the list.  Batches and automatic streams are then sized from lp->n * nsamples.
// fo != nullptr (no accum, no out_device; the caller passes maxdepth = 1): a features call (rtmi_render_features_device).  Its
// batches run k_gen_samples, the scene's closest-hit launch and k_features, which writes fo's buffers.
// ao != nullptr (no accum, no out_device; maxdepth = 1 likewise): an ambient-occlusion call (rtmi_render_ao_device).  Its
// batches run a features call's primary pass, k_ao_rays, the scene's any-hit walk of the compacted AO rays and k_ao_resolve,
// which writes ao->out.  A batch is sized so that its AO rays (paths * K at most) stay within batch_paths.
// li != nullptr (no accum, no out_device; maxdepth = 1 likewise): a direct-light call (rtmi_render_light_device).  Its batches
// run a features call's primary pass, k_light_rays, the scene's any-hit walk of the compacted live shadow rays and
// k_light_resolve, which writes li's planes.  A batch is sized like an AO call's, in candidates.
// pv != nullptr (no accum, no out_device; maxdepth = 1 likewise): a preview call (rtmi_render_preview_device).  Its batches run
// a features call's primary pass once (with k_features when pv->fo asks), k_preview_rays, ONE any-hit walk of the AO rays and
// all lights' live rays and k_preview_resolve, which writes pv's colour and planes.  A batch is sized in queue entries.
// sh != nullptr (with accum): a shadowed path-trace (rtmi_render_shadowed_device).  A progressive pass in every respect, always
// on the per-pass pipeline, whose batches run k_shadow_rays, the scene's any-hit walk of the pass's live shadow rays and
// k_shade_shadowed (for k_shade_samples) in every bounce pass.
// cam != nullptr (with accum, or with fo): a camera call (rtmi_render_camera_device).  A progressive pass (or a features call)
// in every respect, always on the per-pass pipeline, whose batches run k_gen_camera for k_gen_samples and, with accum,
// k_features on pass 0's hit records when cam->fo asks.
// views > 0 (no accum): a batch of views (Samp::VIEWS, rtmi_render_views_device); vp is the stacked image (height = views *
// the views' height) and s->hvcams holds the view table, uploaded here on hip_stream before the internal streams fork.
static int render_tile(rtmi_scene_t* s, const rtmi_viewport_t* vp, uint64_t seed, const rtmi_tile_t* tile, uint32_t sample0,
                       uint32_t nsamples, float4* accum, void* out_device, void* hip_stream, rtmi_stats_t* stats,
                       const ListPass* lp = nullptr, uint32_t views = 0, const FeatOut* fo = nullptr, const AoCall* ao = nullptr,
                       const LightCall* li = nullptr, const PreviewCall* pv = nullptr, const ShadowCall* sh = nullptr,
                       const CameraCall* cam = nullptr) {
    if (stats) memset(stats, 0, sizeof(*stats));
    if (tile->nrows == 0) return RTMI_OK;
    RTMI_GUARD_BEGIN
    // leftovers of the caller's own HIP calls on this thread (or of failures this library tolerated, e.g. an occupancy
    // query) must not make a launch below look refused: hipGetLastError() reports the last error of ANY runtime call
    (void)hipGetLastError();
    if (!out_device && !accum && !fo && !ao && !li && !pv) return fail(RTMI_ERR_INVALID, "NULL argument");
    int rc = check_view(vp, tile);
    if (rc != RTMI_OK) return rc;
    HIPCHK(hipSetDevice(s->device));
    hipStream_t ust = (hipStream_t)hip_stream;
    float4* out = (float4*)out_device;
    if (vp->maxdepth == 0) {  // project_ray returns black immediately (raytrace.rs:1261-1263); acc*(1/spp) of zeros
        const uint64_t npix = (uint64_t)tile->nrows * vp->width;
        if (accum) HIPCHK(hipMemsetAsync(accum, 0, npix * sizeof(float4), ust));
        if (out) HIPCHK(hipMemsetAsync(out, 0, npix * sizeof(float4), ust));
        HIPCHK(hipStreamSynchronize(ust));
        return RTMI_OK;
    }
    TileCall c;
    c.seed = seed; c.sample0 = sample0; c.spp = nsamples; c.maxdepth = vp->maxdepth; c.W = vp->width;
    c.accum = accum; c.out = out; c.lp = lp; c.fo = fo; c.ao = ao; c.li = li; c.pv = pv; c.sh = sh; c.cam = cam; c.vt = ViewTab{nullptr, FastDiv{}};
    c.mode = lp ? Samp::LIST : (accum || fo || ao || li || pv) ? Samp::PASS : views ? Samp::VIEWS : Samp::FRAME;
    c.counting = (s->options & RTMI_OPT_COUNTERS) != 0;
    rc = plan_tile(s, vp, tile, c);
    if (rc != RTMI_OK) return rc;
    if (views) {  // the views share one height: pixel_ray's vv_delta and pixel_key's row split use it, not the stack's
        const uint32_t h = vp->height / views;
        for (uint32_t t = 0; t < c.nsub; t++) c.sub[t].dv.height = h;
        HIPCHK(s->vcams.ensure(views));
        HIPCHK(hipMemcpyAsync(s->vcams.p, s->hvcams.data(), views * sizeof(VCam), hipMemcpyHostToDevice, ust));
        if (!s->vcams_ev) HIPCHK(hipEventCreateWithFlags(&s->vcams_ev, hipEventDisableTiming));
        HIPCHK(hipEventRecord(s->vcams_ev, ust));  // set_views of the next call waits for it
        c.vt = ViewTab{s->vcams.p, make_fastdiv(h)};
    }

    // internal streams start after whatever the caller queued on its stream
    HIPCHK(hipEventRecord(s->fork_ev, ust));
    for (uint32_t t = 0; t < c.nsub; t++) HIPCHK(hipStreamWaitEvent(s->istream[t], s->fork_ev, 0));
    TileSums sum;
    for (uint64_t p0 = 0; p0 < c.max_npix; p0 += c.pix_per_batch) {
        for (uint32_t t = 0; t < c.nsub && rc == RTMI_OK; t++)
            if (p0 < c.sub[t].npix) rc = enqueue_batch(s, c, t, p0);
        for (uint32_t t = 0; t < c.nsub && rc == RTMI_OK; t++)
            if (p0 < c.sub[t].npix) rc = collect_batch(s, c, t, p0, sum);
        if (rc != RTMI_OK) return rc;
    }
    // the caller's stream continues after both internal streams
    for (uint32_t t = 0; t < c.nsub; t++) {
        HIPCHK(hipEventRecord(s->join_ev[t], s->istream[t]));
        HIPCHK(hipStreamWaitEvent(ust, s->join_ev[t], 0));
    }
    HIPCHK(hipEventRecord(s->end_ev, ust));
    HIPCHK(hipEventSynchronize(s->end_ev));
    float kernel_ms = 0.f;
    HIPCHK(hipEventElapsedTime(&kernel_ms, s->fork_ev, s->end_ev));
    if (stats) {
        add_counters(*stats, sum.counters);
        stats->kernel_ms = kernel_ms; stats->trace_ms = sum.trace_ms; stats->trace_launches = sum.launches; stats->streams = c.nsub;
        stats->primary_ms = sum.primary_ms; stats->bounce_ms = sum.bounce_ms; stats->pipeline = c.path_kernels ? 3u : 1u;
    }
    if (s->verbose && ao) fprintf(stderr, "[rtmi] AO: %llu of %llu samples hit\n", (unsigned long long)sum.ao_hits, (unsigned long long)tile->nrows * c.W * nsamples);
    return RTMI_OK;
    RTMI_GUARD_END
}

int rtmi_render_tile_device(rtmi_scene_t* s, const rtmi_viewport_t* vp, uint64_t seed, const rtmi_tile_t* tile,
                            void* out_device, void* hip_stream, rtmi_stats_t* stats) {
    if (!s || !vp || !tile) return fail(RTMI_ERR_INVALID, "NULL argument");
    return render_tile(s, vp, seed, tile, 0u, vp->samples_per_pixel, nullptr, out_device, hip_stream, stats);
}

// Checks of the progressive entry points that come before any HIP call (a CPU-only caller reaches them).
static int check_samples(rtmi_scene_t* s, const rtmi_viewport_t* vp, uint32_t sample0, uint32_t nsamples, const void* accum,
                         const void* out) {
    if (!s || !vp) return fail(RTMI_ERR_INVALID, "NULL argument (scene or viewport)");
    if (!accum) return fail(RTMI_ERR_INVALID, "NULL accumulator");
    if (accum == out) return fail(RTMI_ERR_INVALID, "accumulator and output must be different buffers");
    if (vp->samples_per_pixel == 0) return fail(RTMI_ERR_INVALID, "samples_per_pixel must be >= 1");
    if (nsamples == 0) return fail(RTMI_ERR_INVALID, "nsamples must be >= 1");
    if ((uint64_t)sample0 + nsamples > vp->samples_per_pixel)
        return fail(RTMI_ERR_INVALID, "samples [sample0, sample0 + nsamples) outside the frame's samples_per_pixel");
    if (sample0 & RTMI_KEY_JITTER) return fail(RTMI_ERR_UNSUPPORTED, "sample0 above 2^31");  // DView::sample_key
    return RTMI_OK;
}

int rtmi_render_samples_device(rtmi_scene_t* s, const rtmi_viewport_t* vp, uint64_t seed, const rtmi_tile_t* tile,
                               uint32_t sample0, uint32_t nsamples, void* accum_device, void* out_device, void* hip_stream,
                               rtmi_stats_t* stats) {
    if (stats) memset(stats, 0, sizeof(*stats));
    const int rc = check_samples(s, vp, sample0, nsamples, accum_device, out_device);
    if (rc != RTMI_OK) return rc;
    if (!tile) return fail(RTMI_ERR_INVALID, "NULL argument (tile)");
    return render_tile(s, vp, seed, tile, sample0, nsamples, (float4*)accum_device, out_device, hip_stream, stats);
}

// Host variant: accum is copied in (only when sample0 > 0) and out again, 2 x 16 B per pixel over the host link per pass.
int rtmi_render_samples(rtmi_scene_t* s, const rtmi_viewport_t* vp, uint64_t seed, uint32_t row0, uint32_t nrows,
                        uint32_t sample0, uint32_t nsamples, float* accum_host, float* out_host, rtmi_stats_t* stats) {
    if (stats) memset(stats, 0, sizeof(*stats));
    const int rc0 = check_samples(s, vp, sample0, nsamples, accum_host, out_host);
    if (rc0 != RTMI_OK) return rc0;
    const uint64_t npix = (uint64_t)nrows * vp->width;
    if (npix == 0) return RTMI_OK;
    if ((uint64_t)row0 + nrows > vp->height) return fail(RTMI_ERR_INVALID, "row range outside the viewport");
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(s->acc.ensure(npix));
    if (out_host) HIPCHK(s->tile.ensure(npix));
    if (sample0 > 0) HIPCHK(hipMemcpy(s->acc.p, accum_host, npix * sizeof(float4), hipMemcpyHostToDevice));
    const rtmi_tile_t tile{row0, nrows, nrows, 0u};
    int rc = render_tile(s, vp, seed, &tile, sample0, nsamples, s->acc.p, out_host ? (void*)s->tile.p : nullptr, nullptr, stats);
    if (rc != RTMI_OK) return rc;
    HIPCHK(hipMemcpy(accum_host, s->acc.p, npix * sizeof(float4), hipMemcpyDeviceToHost));
    if (out_host) HIPCHK(hipMemcpy(out_host, s->tile.p, npix * sizeof(float4), hipMemcpyDeviceToHost));
    return RTMI_OK;
}

// ---------------------------------------------------------------- first-hit feature buffers
// Checks of the features entry points that come before any HIP call and before the scene is used (a CPU-only caller reaches
// them).  RTMI_OK with *empty set: the tile has no rows, nothing to do.  v1 receives the viewport with maxdepth = 1: the
// caller's maxdepth is not consulted, only the primary ray is traced.
static int check_features(rtmi_scene_t* s, const rtmi_viewport_t* vp, const rtmi_tile_t* tile, uint32_t sample0, uint32_t nsamples,
                          const void* albedo, const void* normal, const void* ids, rtmi_viewport_t& v1, bool* empty) {
    *empty = false;
    if (!s || !vp) return fail(RTMI_ERR_INVALID, "NULL argument (scene or viewport)");
    if (!tile) return fail(RTMI_ERR_INVALID, "NULL argument (tile)");
    if (!albedo && !normal && !ids) return fail(RTMI_ERR_INVALID, "NULL outputs: at least one of albedo, normal and ids is required");
    if ((albedo && (albedo == normal || albedo == ids)) || (normal && normal == ids))
        return fail(RTMI_ERR_INVALID, "outputs must not alias (albedo, normal, ids)");
    if (vp->samples_per_pixel == 0) return fail(RTMI_ERR_INVALID, "samples_per_pixel must be >= 1");
    if (nsamples == 0) return fail(RTMI_ERR_INVALID, "nsamples must be >= 1");
    if ((uint64_t)sample0 + nsamples > vp->samples_per_pixel)
        return fail(RTMI_ERR_INVALID, "samples [sample0, sample0 + nsamples) outside the frame's samples_per_pixel");
    if (sample0 & RTMI_KEY_JITTER) return fail(RTMI_ERR_UNSUPPORTED, "sample0 above 2^31");  // DView::sample_key
    if (tile->nrows == 0) { *empty = true; return RTMI_OK; }
    v1 = *vp;
    v1.maxdepth = 1;
    return check_view(&v1, tile);
}

int rtmi_render_features_device(rtmi_scene_t* s, const rtmi_viewport_t* vp, uint64_t seed, const rtmi_tile_t* tile,
                                uint32_t sample0, uint32_t nsamples, void* albedo_device, void* normal_device, void* ids_device,
                                void* hip_stream, rtmi_stats_t* stats) {
    if (stats) memset(stats, 0, sizeof(*stats));
    rtmi_viewport_t v1;
    bool empty;
    const int rc = check_features(s, vp, tile, sample0, nsamples, albedo_device, normal_device, ids_device, v1, &empty);
    if (rc != RTMI_OK || empty) return rc;
    if (s->d.nspheres)
        return fail(RTMI_ERR_UNSUPPORTED, "features: the scene has analytic spheres (a build-defined primitive whose normal needs the hit point)");
    const FeatOut fo{(float4*)albedo_device, (float4*)normal_device, (uint32_t*)ids_device};
    return render_tile(s, &v1, seed, tile, sample0, nsamples, nullptr, nullptr, hip_stream, stats, nullptr, 0, &fo);
}

// Host variant: the requested buffers are rendered into the handle's own device buffers and copied out once.
int rtmi_render_features(rtmi_scene_t* s, const rtmi_viewport_t* vp, uint64_t seed, uint32_t row0, uint32_t nrows,
                         uint32_t sample0, uint32_t nsamples, float* albedo_host, float* normal_host, uint32_t* ids_host,
                         rtmi_stats_t* stats) {
    if (stats) memset(stats, 0, sizeof(*stats));
    const rtmi_tile_t tile{row0, nrows, nrows ? nrows : 1u, 0u};
    rtmi_viewport_t v1;
    bool empty;
    const int rc0 = check_features(s, vp, &tile, sample0, nsamples, albedo_host, normal_host, ids_host, v1, &empty);
    if (rc0 != RTMI_OK || empty) return rc0;
    if (s->d.nspheres)
        return fail(RTMI_ERR_UNSUPPORTED, "features: the scene has analytic spheres (a build-defined primitive whose normal needs the hit point)");
    const uint64_t npix = (uint64_t)nrows * vp->width;
    HIPCHK(hipSetDevice(s->device));
    if (albedo_host) HIPCHK(s->tile.ensure(npix));
    if (normal_host) HIPCHK(s->acc.ensure(npix));
    if (ids_host) HIPCHK(s->acnt.ensure(npix));
    const FeatOut fo{albedo_host ? s->tile.p : nullptr, normal_host ? s->acc.p : nullptr, ids_host ? s->acnt.p : nullptr};
    const int rc = render_tile(s, &v1, seed, &tile, sample0, nsamples, nullptr, nullptr, nullptr, stats, nullptr, 0, &fo);
    if (rc != RTMI_OK) return rc;
    if (albedo_host) HIPCHK(hipMemcpy(albedo_host, fo.albedo, npix * sizeof(float4), hipMemcpyDeviceToHost));
    if (normal_host) HIPCHK(hipMemcpy(normal_host, fo.normal, npix * sizeof(float4), hipMemcpyDeviceToHost));
    if (ids_host) HIPCHK(hipMemcpy(ids_host, fo.ids, npix * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return RTMI_OK;
}

// ---------------------------------------------------------------- built-in camera models (rtmi_render_camera*)
void rtmi_camera_defaults(rtmi_camera_t* c) {
    if (!c) return;
    c->model = RTMI_CAMERA_PINHOLE; c->flags = 0; c->lens_radius = 0.f; c->focus = 1.f;
}

// Checks of the camera entry points that come before any HIP call and before the scene is used (a CPU-only caller reaches
// them): rtmi_render_samples_device's, then the camera's and the guides'.  RTMI_OK with *empty set: the tile has no rows.
static int check_camera(rtmi_scene_t* s, const rtmi_viewport_t* vp, const rtmi_tile_t* tile, const rtmi_camera_t* cam, uint32_t sample0,
                        uint32_t nsamples, const void* accum, const void* out, const rtmi_camera_out_t* g, bool* empty) {
    *empty = false;
    const int rc = check_samples(s, vp, sample0, nsamples, accum, out);
    if (rc != RTMI_OK) return rc;
    if (!tile) return fail(RTMI_ERR_INVALID, "NULL argument (tile)");
    if (!cam) return fail(RTMI_ERR_INVALID, "camera: NULL argument (rtmi_camera_t)");
    if (cam->model > RTMI_CAMERA_ORTHO) return fail(RTMI_ERR_INVALID, "camera: unknown model");
    if (cam->flags != 0) return fail(RTMI_ERR_INVALID, "camera: flags must be 0");
    if (cam->model == RTMI_CAMERA_THIN_LENS) {
        if (!(cam->lens_radius >= 0.f) || !std::isfinite(cam->lens_radius))
            return fail(RTMI_ERR_INVALID, "camera: lens_radius must be finite and >= 0");
        if (!(cam->focus > 0.f) || !std::isfinite(cam->focus)) return fail(RTMI_ERR_INVALID, "camera: focus must be finite and > 0");
    }
    if (g) {
        const void* b[5] = {accum, out, g->albedo, g->normal, g->ids};
        for (int i = 2; i < 5; i++)
            for (int j = 0; j < i; j++)
                if (b[i] && b[i] == b[j]) return fail(RTMI_ERR_INVALID, "camera: a guide buffer aliases another buffer (accum, out, albedo, normal, ids)");
    }
    if (tile->nrows == 0) { *empty = true; return RTMI_OK; }
    return check_view(vp, tile);
}

// Both variants, on device buffers, after check_camera.  maxdepth == 0: render_tile writes the zeros; the guides do not depend
// on the depth and come from a features call with the camera's generator.
static int render_camera(rtmi_scene_t* s, const rtmi_viewport_t* vp, uint64_t seed, const rtmi_tile_t* tile, const rtmi_camera_t* cam,
                         uint32_t sample0, uint32_t nsamples, float4* accum, void* out, const FeatOut& fo, void* hip_stream,
                         rtmi_stats_t* stats) {
    const bool guides = fo.albedo || fo.normal || fo.ids;
    if (guides && s->d.nspheres)
        return fail(RTMI_ERR_UNSUPPORTED, "camera: no guide buffers (albedo, normal, ids) for scenes with analytic spheres");
    const CameraCall cc{DCam{cam->model, cam->lens_radius, cam->focus}, fo};
    const int rc = render_tile(s, vp, seed, tile, sample0, nsamples, accum, out, hip_stream, stats, nullptr, 0, nullptr, nullptr, nullptr,
                               nullptr, nullptr, &cc);
    if (rc != RTMI_OK || vp->maxdepth != 0 || !guides) return rc;
    rtmi_viewport_t v1 = *vp;
    v1.maxdepth = 1;
    return render_tile(s, &v1, seed, tile, sample0, nsamples, nullptr, nullptr, hip_stream, stats, nullptr, 0, &cc.fo, nullptr, nullptr,
                       nullptr, nullptr, &cc);
}

int rtmi_render_camera_device(rtmi_scene_t* s, const rtmi_viewport_t* vp, uint64_t seed, const rtmi_tile_t* tile,
                              const rtmi_camera_t* camera, uint32_t sample0, uint32_t nsamples, void* accum_device, void* out_device,
                              const rtmi_camera_out_t* guides, void* hip_stream, rtmi_stats_t* stats) {
    if (stats) memset(stats, 0, sizeof(*stats));
    bool empty;
    const int rc = check_camera(s, vp, tile, camera, sample0, nsamples, accum_device, out_device, guides, &empty);
    if (rc != RTMI_OK || empty) return rc;
    const FeatOut fo = guides ? FeatOut{(float4*)guides->albedo, (float4*)guides->normal, (uint32_t*)guides->ids} : FeatOut{nullptr, nullptr, nullptr};
    return render_camera(s, vp, seed, tile, camera, sample0, nsamples, (float4*)accum_device, out_device, fo, hip_stream, stats);
}

// Host variant: accum is copied in (only when sample0 > 0) and out again like rtmi_render_samples; the guides are rendered
// into the host variants' per-pixel buffers of the handle (asq: albedo, then normal; acnt: ids) and copied out once.
int rtmi_render_camera(rtmi_scene_t* s, const rtmi_viewport_t* vp, uint64_t seed, uint32_t row0, uint32_t nrows,
                       const rtmi_camera_t* camera, uint32_t sample0, uint32_t nsamples, float* accum_host, float* out_host,
                       const rtmi_camera_out_t* guides_host, rtmi_stats_t* stats) {
    if (stats) memset(stats, 0, sizeof(*stats));
    const rtmi_tile_t tile{row0, nrows, nrows ? nrows : 1u, 0u};
    bool empty;
    const int rc0 = check_camera(s, vp, &tile, camera, sample0, nsamples, accum_host, out_host, guides_host, &empty);
    if (rc0 != RTMI_OK || empty) return rc0;
    const rtmi_camera_out_t g = guides_host ? *guides_host : rtmi_camera_out_t{nullptr, nullptr, nullptr};
    if ((g.albedo || g.normal || g.ids) && s->d.nspheres)
        return fail(RTMI_ERR_UNSUPPORTED, "camera: no guide buffers (albedo, normal, ids) for scenes with analytic spheres");
    const uint64_t npix = (uint64_t)nrows * vp->width;
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(s->acc.ensure(npix));
    if (out_host) HIPCHK(s->tile.ensure(npix));
    if (g.albedo || g.normal) HIPCHK(s->asq.ensure(2 * npix));
    if (g.ids) HIPCHK(s->acnt.ensure(npix));
    if (sample0 > 0) HIPCHK(hipMemcpy(s->acc.p, accum_host, npix * sizeof(float4), hipMemcpyHostToDevice));
    const FeatOut fo{g.albedo ? s->asq.p : nullptr, g.normal ? s->asq.p + npix : nullptr, g.ids ? s->acnt.p : nullptr};
    const int rc = render_camera(s, vp, seed, &tile, camera, sample0, nsamples, s->acc.p, out_host ? (void*)s->tile.p : nullptr, fo, nullptr, stats);
    if (rc != RTMI_OK) return rc;
    HIPCHK(hipMemcpy(accum_host, s->acc.p, npix * sizeof(float4), hipMemcpyDeviceToHost));
    if (out_host) HIPCHK(hipMemcpy(out_host, s->tile.p, npix * sizeof(float4), hipMemcpyDeviceToHost));
    if (g.albedo) HIPCHK(hipMemcpy(g.albedo, fo.albedo, npix * sizeof(float4), hipMemcpyDeviceToHost));
    if (g.normal) HIPCHK(hipMemcpy(g.normal, fo.normal, npix * sizeof(float4), hipMemcpyDeviceToHost));
    if (g.ids) HIPCHK(hipMemcpy(g.ids, fo.ids, npix * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return RTMI_OK;
}

// ---------------------------------------------------------------- ambient occlusion (rtmi_render_ao*)
void rtmi_ao_defaults(rtmi_ao_t* p) {
    if (!p) return;
    p->rays = 4; p->flags = 0; p->radius = INFINITY;
    p->bias = 0.001f;  // the reference's bounce offset (raytrace.rs:284-296)
}

// Checks of the AO entry points that come before any HIP call and before the scene is used (a CPU-only caller reaches them).
// RTMI_OK with *empty set: the tile has no rows, nothing to do.  v1 receives the viewport with maxdepth = 1, as for features.
static int check_ao(rtmi_scene_t* s, const rtmi_viewport_t* vp, const rtmi_tile_t* tile, uint32_t sample0, uint32_t nsamples,
                    const rtmi_ao_t* ao, const void* out, rtmi_viewport_t& v1, bool* empty) {
    *empty = false;
    if (!s || !vp) return fail(RTMI_ERR_INVALID, "ao: NULL argument (scene or viewport)");
    if (!tile) return fail(RTMI_ERR_INVALID, "ao: NULL argument (tile)");
    if (!ao) return fail(RTMI_ERR_INVALID, "ao: NULL argument (rtmi_ao_t)");
    if (!out) return fail(RTMI_ERR_INVALID, "ao: NULL argument (output)");
    if (ao->rays == 0 || ao->rays > 256) return fail(RTMI_ERR_INVALID, "ao: rays must be in [1, 256]");
    if (ao->flags != 0) return fail(RTMI_ERR_INVALID, "ao: flags must be 0");
    if (!(ao->radius >= 0.f)) return fail(RTMI_ERR_INVALID, "ao: radius must be >= 0 (+inf: unlimited) and not NaN");
    if (!std::isfinite(ao->bias)) return fail(RTMI_ERR_INVALID, "ao: bias must be finite");
    if (vp->samples_per_pixel == 0) return fail(RTMI_ERR_INVALID, "samples_per_pixel must be >= 1");
    if (nsamples == 0) return fail(RTMI_ERR_INVALID, "nsamples must be >= 1");
    if ((uint64_t)sample0 + nsamples > vp->samples_per_pixel)
        return fail(RTMI_ERR_INVALID, "samples [sample0, sample0 + nsamples) outside the frame's samples_per_pixel");
    if (sample0 & RTMI_KEY_JITTER) return fail(RTMI_ERR_UNSUPPORTED, "sample0 above 2^31");  // DView::sample_key
    if ((uint64_t)nsamples * ao->rays >= (1ull << 24))
        return fail(RTMI_ERR_UNSUPPORTED, "ao: nsamples * rays must stay below 2^24 (the per-pixel count is exact in f32)");
    if (tile->nrows == 0) { *empty = true; return RTMI_OK; }
    v1 = *vp;
    v1.maxdepth = 1;
    return check_view(&v1, tile);
}

int rtmi_render_ao_device(rtmi_scene_t* s, const rtmi_viewport_t* vp, uint64_t seed, const rtmi_tile_t* tile, uint32_t sample0,
                          uint32_t nsamples, const rtmi_ao_t* ao, void* ao_device, void* hip_stream, rtmi_stats_t* stats) {
    if (stats) memset(stats, 0, sizeof(*stats));
    rtmi_viewport_t v1;
    bool empty;
    const int rc = check_ao(s, vp, tile, sample0, nsamples, ao, ao_device, v1, &empty);
    if (rc != RTMI_OK || empty) return rc;
    if (s->d.nspheres)
        return fail(RTMI_ERR_UNSUPPORTED, "ao: the scene has analytic spheres (a build-defined primitive whose normal needs the hit point)");
    const AoCall call{*ao, (float*)ao_device};
    return render_tile(s, &v1, seed, tile, sample0, nsamples, nullptr, nullptr, hip_stream, stats, nullptr, 0, nullptr, &call);
}

// Host variant: the image is rendered into the handle's own device buffer and copied out once (4 B per pixel).
int rtmi_render_ao(rtmi_scene_t* s, const rtmi_viewport_t* vp, uint64_t seed, uint32_t row0, uint32_t nrows, uint32_t sample0,
                   uint32_t nsamples, const rtmi_ao_t* ao, float* ao_host, rtmi_stats_t* stats) {
    if (stats) memset(stats, 0, sizeof(*stats));
    const rtmi_tile_t tile{row0, nrows, nrows ? nrows : 1u, 0u};
    rtmi_viewport_t v1;
    bool empty;
    const int rc0 = check_ao(s, vp, &tile, sample0, nsamples, ao, ao_host, v1, &empty);
    if (rc0 != RTMI_OK || empty) return rc0;
    if (s->d.nspheres)
        return fail(RTMI_ERR_UNSUPPORTED, "ao: the scene has analytic spheres (a build-defined primitive whose normal needs the hit point)");
    const uint64_t npix = (uint64_t)nrows * vp->width;
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(s->ao_out.ensure(npix));
    const AoCall call{*ao, s->ao_out.p};
    const int rc = render_tile(s, &v1, seed, &tile, sample0, nsamples, nullptr, nullptr, nullptr, stats, nullptr, 0, nullptr, &call);
    if (rc != RTMI_OK) return rc;
    HIPCHK(hipMemcpy(ao_host, s->ao_out.p, npix * sizeof(float), hipMemcpyDeviceToHost));
    return RTMI_OK;
}

// ---------------------------------------------------------------- direct light (rtmi_render_light*)
void rtmi_light_defaults(rtmi_light_t* p) {
    if (!p) return;
    p->orig[0] = p->orig[1] = p->orig[2] = 0.f;
    p->len2 = 0.f; p->rays = 4; p->flags = 0;
    p->bias = 0.005f;  // the reference's smudge factor (raytrace.rs:607)
}

// Checks of the direct-light entry points that come before any HIP call and before the scene is used (a CPU-only caller
// reaches them).  RTMI_OK with *empty set: the tile has no rows, nothing to do.  v1 receives the viewport with maxdepth = 1,
// as for features.
static int check_light(rtmi_scene_t* s, const rtmi_viewport_t* vp, const rtmi_tile_t* tile, uint32_t sample0, uint32_t nsamples,
                       const rtmi_light_t* li, const void* shadow, const void* irradiance, rtmi_viewport_t& v1, bool* empty) {
    *empty = false;
    if (!s || !vp) return fail(RTMI_ERR_INVALID, "light: NULL argument (scene or viewport)");
    if (!tile) return fail(RTMI_ERR_INVALID, "light: NULL argument (tile)");
    if (!li) return fail(RTMI_ERR_INVALID, "light: NULL argument (rtmi_light_t)");
    if (!shadow && !irradiance) return fail(RTMI_ERR_INVALID, "light: NULL argument (both outputs)");
    if (shadow == irradiance) return fail(RTMI_ERR_INVALID, "light: the two outputs must not alias");
    if (li->rays == 0 || li->rays > 256) return fail(RTMI_ERR_INVALID, "light: rays must be in [1, 256]");
    if (li->flags & ~(uint32_t)RTMI_LIGHT_UNBOUNDED) return fail(RTMI_ERR_INVALID, "light: unknown flags");
    if (!(li->len2 >= 0.f) || std::isinf(li->len2)) return fail(RTMI_ERR_INVALID, "light: len2 must be >= 0, finite and not NaN");
    if (!std::isfinite(li->orig[0]) || !std::isfinite(li->orig[1]) || !std::isfinite(li->orig[2]))
        return fail(RTMI_ERR_INVALID, "light: orig must be finite");
    if (!std::isfinite(li->bias)) return fail(RTMI_ERR_INVALID, "light: bias must be finite");
    if (vp->samples_per_pixel == 0) return fail(RTMI_ERR_INVALID, "samples_per_pixel must be >= 1");
    if (nsamples == 0) return fail(RTMI_ERR_INVALID, "nsamples must be >= 1");
    if ((uint64_t)sample0 + nsamples > vp->samples_per_pixel)
        return fail(RTMI_ERR_INVALID, "samples [sample0, sample0 + nsamples) outside the frame's samples_per_pixel");
    if (sample0 & RTMI_KEY_JITTER) return fail(RTMI_ERR_UNSUPPORTED, "sample0 above 2^31");  // DView::sample_key
    if ((uint64_t)nsamples * li->rays >= (1ull << 24))
        return fail(RTMI_ERR_UNSUPPORTED, "light: nsamples * rays must stay below 2^24 (the per-pixel count is exact in f32)");
    if (tile->nrows == 0) { *empty = true; return RTMI_OK; }
    v1 = *vp;
    v1.maxdepth = 1;
    return check_view(&v1, tile);
}

int rtmi_render_light_device(rtmi_scene_t* s, const rtmi_viewport_t* vp, uint64_t seed, const rtmi_tile_t* tile, uint32_t sample0,
                             uint32_t nsamples, const rtmi_light_t* li, void* shadow_device, void* irradiance_device, void* hip_stream,
                             rtmi_stats_t* stats) {
    if (stats) memset(stats, 0, sizeof(*stats));
    rtmi_viewport_t v1;
    bool empty;
    const int rc = check_light(s, vp, tile, sample0, nsamples, li, shadow_device, irradiance_device, v1, &empty);
    if (rc != RTMI_OK || empty) return rc;
    if (s->d.nspheres)
        return fail(RTMI_ERR_UNSUPPORTED, "light: the scene has analytic spheres (a build-defined primitive whose normal needs the hit point)");
    const LightCall call{*li, (float*)shadow_device, (float*)irradiance_device};
    return render_tile(s, &v1, seed, tile, sample0, nsamples, nullptr, nullptr, hip_stream, stats, nullptr, 0, nullptr, nullptr, &call);
}

// Host variant: the planes are rendered into the handle's own device buffer and copied out once (4 B per pixel and plane).
int rtmi_render_light(rtmi_scene_t* s, const rtmi_viewport_t* vp, uint64_t seed, uint32_t row0, uint32_t nrows, uint32_t sample0,
                      uint32_t nsamples, const rtmi_light_t* li, float* shadow_host, float* irradiance_host, rtmi_stats_t* stats) {
    if (stats) memset(stats, 0, sizeof(*stats));
    const rtmi_tile_t tile{row0, nrows, nrows ? nrows : 1u, 0u};
    rtmi_viewport_t v1;
    bool empty;
    const int rc0 = check_light(s, vp, &tile, sample0, nsamples, li, shadow_host, irradiance_host, v1, &empty);
    if (rc0 != RTMI_OK || empty) return rc0;
    if (s->d.nspheres)
        return fail(RTMI_ERR_UNSUPPORTED, "light: the scene has analytic spheres (a build-defined primitive whose normal needs the hit point)");
    const uint64_t npix = (uint64_t)nrows * vp->width;
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(s->light_out.ensure(2 * npix));
    float* const d_sh = shadow_host ? s->light_out.p : nullptr;
    float* const d_ir = irradiance_host ? s->light_out.p + npix : nullptr;
    const LightCall call{*li, d_sh, d_ir};
    const int rc = render_tile(s, &v1, seed, &tile, sample0, nsamples, nullptr, nullptr, nullptr, stats, nullptr, 0, nullptr, nullptr, &call);
    if (rc != RTMI_OK) return rc;
    if (d_sh) HIPCHK(hipMemcpy(shadow_host, d_sh, npix * sizeof(float), hipMemcpyDeviceToHost));
    if (d_ir) HIPCHK(hipMemcpy(irradiance_host, d_ir, npix * sizeof(float), hipMemcpyDeviceToHost));
    return RTMI_OK;
}

// ---------------------------------------------------------------- shadowed path-trace (rtmi_render_shadowed*)
// Checks of the shadowed entry points that come before any HIP call and before the scene is used (a CPU-only caller reaches
// them): rtmi_render_samples_device's, then rtmi_render_light*'s on the light, then rays == 1.
static int check_shadowed(rtmi_scene_t* s, const rtmi_viewport_t* vp, uint32_t sample0, uint32_t nsamples, const rtmi_light_t* li,
                          const void* accum, const void* out) {
    const int rc = check_samples(s, vp, sample0, nsamples, accum, out);
    if (rc != RTMI_OK) return rc;
    if (!li) return fail(RTMI_ERR_INVALID, "shadowed: NULL argument (rtmi_light_t)");
    if (li->rays == 0 || li->rays > 256) return fail(RTMI_ERR_INVALID, "shadowed: rays must be in [1, 256]");
    if (li->flags & ~(uint32_t)RTMI_LIGHT_UNBOUNDED) return fail(RTMI_ERR_INVALID, "shadowed: unknown flags");
    if (!(li->len2 >= 0.f) || std::isinf(li->len2)) return fail(RTMI_ERR_INVALID, "shadowed: len2 must be >= 0, finite and not NaN");
    if (!std::isfinite(li->orig[0]) || !std::isfinite(li->orig[1]) || !std::isfinite(li->orig[2]))
        return fail(RTMI_ERR_INVALID, "shadowed: orig must be finite");
    if (!std::isfinite(li->bias)) return fail(RTMI_ERR_INVALID, "shadowed: bias must be finite");
    if (li->rays != 1) return fail(RTMI_ERR_INVALID, "shadowed: rays must be 1 (the reference draws one shadow ray per hit)");
    return RTMI_OK;
}
// scenes the shadowed shading (shadowed.hpp has its own shade_hit) does not take; before any HIP call
static int refuse_scene_shadowed(const rtmi_scene_t* s) {
    if (s->d.nspheres)
        return fail(RTMI_ERR_UNSUPPORTED, "shadowed: the scene has analytic spheres (a build-defined primitive whose normal needs the hit point)");
    if (s->has_dielectric)
        return fail(RTMI_ERR_UNSUPPORTED, "shadowed: the scene has a dielectric surface (the shadowed shading has no glass arm)");
    if (s->has_env)
        return fail(RTMI_ERR_UNSUPPORTED, "shadowed: the scene has an environment (the shadowed shading has no environment arm)");
    if (s->has_normals)
        return fail(RTMI_ERR_UNSUPPORTED, "shadowed: the scene has vertex normals (the shadowed shading has no smooth arm)");
    if (s->has_tex)
        return fail(RTMI_ERR_UNSUPPORTED, "shadowed: the scene has textures (the shadowed shading has no texture arm)");
    return RTMI_OK;
}

int rtmi_render_shadowed_device(rtmi_scene_t* s, const rtmi_viewport_t* vp, uint64_t seed, const rtmi_tile_t* tile, uint32_t sample0,
                                uint32_t nsamples, const rtmi_light_t* li, void* accum_device, void* out_device, void* hip_stream,
                                rtmi_stats_t* stats) {
    if (stats) memset(stats, 0, sizeof(*stats));
    int rc = check_shadowed(s, vp, sample0, nsamples, li, accum_device, out_device);
    if (rc != RTMI_OK) return rc;
    if (!tile) return fail(RTMI_ERR_INVALID, "NULL argument (tile)");
    if (tile->nrows == 0) return RTMI_OK;
    rc = check_view(vp, tile);
    if (rc != RTMI_OK) return rc;
    rc = refuse_scene_shadowed(s);
    if (rc != RTMI_OK) return rc;
    const ShadowCall call{*li};
    return render_tile(s, vp, seed, tile, sample0, nsamples, (float4*)accum_device, out_device, hip_stream, stats, nullptr, 0, nullptr,
                       nullptr, nullptr, nullptr, &call);
}

// Host variant: rtmi_render_samples' copies (accum in only when sample0 > 0, accum and out back).
int rtmi_render_shadowed(rtmi_scene_t* s, const rtmi_viewport_t* vp, uint64_t seed, uint32_t row0, uint32_t nrows, uint32_t sample0,
                         uint32_t nsamples, const rtmi_light_t* li, float* accum_host, float* out_host, rtmi_stats_t* stats) {
    if (stats) memset(stats, 0, sizeof(*stats));
    int rc = check_shadowed(s, vp, sample0, nsamples, li, accum_host, out_host);
    if (rc != RTMI_OK) return rc;
    const uint64_t npix = (uint64_t)nrows * vp->width;
    if (npix == 0) return RTMI_OK;
    if ((uint64_t)row0 + nrows > vp->height) return fail(RTMI_ERR_INVALID, "row range outside the viewport");
    const rtmi_tile_t tile{row0, nrows, nrows, 0u};
    rc = check_view(vp, &tile);
    if (rc != RTMI_OK) return rc;
    rc = refuse_scene_shadowed(s);
    if (rc != RTMI_OK) return rc;
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(s->acc.ensure(npix));
    if (out_host) HIPCHK(s->tile.ensure(npix));
    if (sample0 > 0) HIPCHK(hipMemcpy(s->acc.p, accum_host, npix * sizeof(float4), hipMemcpyHostToDevice));
    const ShadowCall call{*li};
    rc = render_tile(s, vp, seed, &tile, sample0, nsamples, s->acc.p, out_host ? (void*)s->tile.p : nullptr, nullptr, stats, nullptr, 0,
                     nullptr, nullptr, nullptr, nullptr, &call);
    if (rc != RTMI_OK) return rc;
    HIPCHK(hipMemcpy(accum_host, s->acc.p, npix * sizeof(float4), hipMemcpyDeviceToHost));
    if (out_host) HIPCHK(hipMemcpy(out_host, s->tile.p, npix * sizeof(float4), hipMemcpyDeviceToHost));
    return RTMI_OK;
}

// ---------------------------------------------------------------- environment sampling at matte hits (rtmi_render_envlight*)
void rtmi_envlight_defaults(rtmi_envlight_t* e) {
    if (!e) return;
    e->bias = 0.001f;
    e->flags = 0u;
}

// The sampler table of the scene's environment (envlight.hpp), built once per table: wmax, then q and the in-row prefix sums
// (a wave per row), then the scan of the row totals.  The launches are sized by n.
static int ensure_env_sampler(rtmi_scene_t* s) {
    if (s->envsamp_ok) return RTMI_OK;
    const uint32_t n = s->envtab.n;
    const size_t nt = (size_t)n * n;
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(s->envq.ensure(nt)); HIPCHK(s->envex.ensure(nt)); HIPCHK(s->envq_max.ensure(1));
    HIPCHK(s->envrows.ensure((size_t)n + 1)); HIPCHK(s->envrowsum.ensure(n));
    HIPCHK(hipMemsetAsync(s->envq_max.p, 0, sizeof(uint32_t), 0));
    hipLaunchKernelGGL(k_envq_max, dim3((unsigned)((nt + 255u) / 256u)), dim3(256), 0, 0, s->env.p, n, s->envtab.fn, s->envq_max.p);
    hipLaunchKernelGGL(k_envq_rows, dim3((n + 3u) / 4u), dim3(256), 0, 0, s->env.p, n, s->envtab.fn, s->envq_max.p, s->envq.p, s->envex.p,
                       s->envrowsum.p);
    hipLaunchKernelGGL(k_envq_scan, dim3(1), dim3(256), 0, 0, s->envrowsum.p, n, s->envrows.p);
    HIPCHK(hipGetLastError());
    unsigned long long total = 0ull;
    HIPCHK(hipMemcpy(&total, s->envrows.p + n, sizeof total, hipMemcpyDeviceToHost));  // (synchronises with the three kernels)
    s->envsamp = EnvSampler{s->envq.p, s->envex.p, s->envrows.p, total};
    s->envsamp_ok = true;
    return RTMI_OK;
}

int rtmi_scene_get_env_sampler(rtmi_scene_t* s, uint32_t* q_out, uint64_t* total_out, uint32_t* n_out) {
    if (!s || !n_out) return fail(RTMI_ERR_INVALID, "NULL argument");
    *n_out = s->has_env ? s->envtab.n : 0u;
    if (total_out) *total_out = 0u;
    if (!s->has_env) return RTMI_OK;
    RTMI_GUARD_BEGIN
    const int rc = ensure_env_sampler(s);
    if (rc != RTMI_OK) return rc;
    if (total_out) *total_out = s->envsamp.total;
    if (q_out) HIPCHK(hipMemcpy(q_out, s->envq.p, (size_t)s->envtab.n * s->envtab.n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return RTMI_OK;
    RTMI_GUARD_END
}

// Checks of the envlight entry points that come before any HIP call: rtmi_render_samples_device's on the arguments, then the
// parameters, then the scenes the call does not take
static int check_envlight(rtmi_scene_t* s, const rtmi_viewport_t* vp, uint32_t sample0, uint32_t nsamples, const rtmi_envlight_t* el,
                          const void* accum, const void* out) {
    const int rc = check_samples(s, vp, sample0, nsamples, accum, out);
    if (rc != RTMI_OK) return rc;
    if (el) {
        if (!std::isfinite(el->bias)) return fail(RTMI_ERR_INVALID, "envlight: bias must be finite");
        if (el->flags != 0u) return fail(RTMI_ERR_INVALID, "envlight: unknown flags");
    }
    return RTMI_OK;
}
static int refuse_scene_envlight(const rtmi_scene_t* s) {
    if (!s->has_env) return fail(RTMI_ERR_UNSUPPORTED, "envlight: the scene has no environment (rtmi_scene_set_environment / rtmi_scene_set_sky)");
    if (s->d.nspheres)
        return fail(RTMI_ERR_UNSUPPORTED, "envlight: the scene has analytic spheres (a build-defined primitive whose normal needs the hit point)");
    if (s->has_dielectric) return fail(RTMI_ERR_UNSUPPORTED, "envlight: the scene has a dielectric surface (the envlight shading has no glass arm)");
    if (s->has_normals) return fail(RTMI_ERR_UNSUPPORTED, "envlight: the scene has vertex normals (the envlight shading has no smooth arm)");
    if (s->has_nmap) return fail(RTMI_ERR_UNSUPPORTED, "envlight: the scene has normal maps (the envlight shading has no normal-map arm)");
    if (s->has_tex) return fail(RTMI_ERR_UNSUPPORTED, "envlight: the scene has textures (the envlight shading has no texture arm)");
    // pe divides the map's density by a^3, which is the solid angle's measure only when the frame is a rotation
    const float4 r[3] = {s->envtab.r0, s->envtab.r1, s->envtab.r2};
    for (int a = 0; a < 3; a++)
        for (int b = 0; b < 3; b++) {
            const float d = vdot(V4{r[a].x, r[a].y, r[a].z, r[a].w}, V4{r[b].x, r[b].y, r[b].z, r[b].w}) - (a == b ? 1.f : 0.f);
            if (!(fabsf(d) <= 1e-4f)) return fail(RTMI_ERR_UNSUPPORTED, "envlight: the environment's frame is not a rotation (|r_i . r_j - delta_ij| > 1e-4)");
        }
    return RTMI_OK;
}

int rtmi_render_envlight_device(rtmi_scene_t* s, const rtmi_viewport_t* vp, uint64_t seed, const rtmi_tile_t* tile, uint32_t sample0,
                                uint32_t nsamples, const rtmi_envlight_t* el, void* accum_device, void* out_device, void* hip_stream,
                                rtmi_stats_t* stats) {
    if (stats) memset(stats, 0, sizeof(*stats));
    int rc = check_envlight(s, vp, sample0, nsamples, el, accum_device, out_device);
    if (rc != RTMI_OK) return rc;
    if (!tile) return fail(RTMI_ERR_INVALID, "NULL argument (tile)");
    if (tile->nrows == 0) return RTMI_OK;
    rc = check_view(vp, tile);
    if (rc != RTMI_OK) return rc;
    rc = refuse_scene_envlight(s);
    if (rc != RTMI_OK) return rc;
    rtmi_envlight_t e;
    rtmi_envlight_defaults(&e);
    if (el) e = *el;
    if (vp->maxdepth != 0) {  // (depth 0 writes zeros and needs no table)
        rc = ensure_env_sampler(s);
        if (rc != RTMI_OK) return rc;
    }
    rtmi_light_t unb{};
    unb.rays = 1; unb.flags = RTMI_LIGHT_UNBOUNDED;
    const ShadowCall call{unb, &e};
    return render_tile(s, vp, seed, tile, sample0, nsamples, (float4*)accum_device, out_device, hip_stream, stats, nullptr, 0, nullptr,
                       nullptr, nullptr, nullptr, &call);
}

// Host variant: rtmi_render_samples' copies (accum in only when sample0 > 0, accum and out back).
int rtmi_render_envlight(rtmi_scene_t* s, const rtmi_viewport_t* vp, uint64_t seed, uint32_t row0, uint32_t nrows, uint32_t sample0,
                         uint32_t nsamples, const rtmi_envlight_t* el, float* accum_host, float* out_host, rtmi_stats_t* stats) {
    if (stats) memset(stats, 0, sizeof(*stats));
    int rc = check_envlight(s, vp, sample0, nsamples, el, accum_host, out_host);
    if (rc != RTMI_OK) return rc;
    const uint64_t npix = (uint64_t)nrows * vp->width;
    if (npix == 0) return RTMI_OK;
    if ((uint64_t)row0 + nrows > vp->height) return fail(RTMI_ERR_INVALID, "row range outside the viewport");
    const rtmi_tile_t tile{row0, nrows, nrows, 0u};
    rc = check_view(vp, &tile);
    if (rc != RTMI_OK) return rc;
    rc = refuse_scene_envlight(s);
    if (rc != RTMI_OK) return rc;
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(s->acc.ensure(npix));
    if (out_host) HIPCHK(s->tile.ensure(npix));
    if (sample0 > 0) HIPCHK(hipMemcpy(s->acc.p, accum_host, npix * sizeof(float4), hipMemcpyHostToDevice));
    rc = rtmi_render_envlight_device(s, vp, seed, &tile, sample0, nsamples, el, s->acc.p, out_host ? (void*)s->tile.p : nullptr, nullptr, stats);
    if (rc != RTMI_OK) return rc;
    HIPCHK(hipMemcpy(accum_host, s->acc.p, npix * sizeof(float4), hipMemcpyDeviceToHost));
    if (out_host) HIPCHK(hipMemcpy(out_host, s->tile.p, npix * sizeof(float4), hipMemcpyDeviceToHost));
    return RTMI_OK;
}

// ---------------------------------------------------------------- emissive triangles sampled at matte hits (rtmi_render_emissive*)
int rtmi_scene_set_emitters(rtmi_scene_t* s, const float* corners9, const uint8_t* emit_of_tri, uint64_t n) {
    if (!s) return fail(RTMI_ERR_INVALID, "scene is NULL");
    const bool set = emit_of_tri && n;
    if (set) {
        if (!corners9) return fail(RTMI_ERR_INVALID, "emitters: corners is NULL");
        if (n != s->d.ntris) return fail(RTMI_ERR_INVALID, "emitters: n must equal ntris");
        for (uint64_t g = 1; g < n; g++) {  // (entry 0 is the sentinel's and is ignored)
            if (!emit_of_tri[g]) continue;
            for (int k = 0; k < 9; k++)
                if (!std::isfinite(corners9[9 * g + k])) return fail(RTMI_ERR_INVALID, "emitters: a corner of triangle " + std::to_string(g) + " is not finite");
            if (s->htris[g].surface_kind != RTMI_SOLID)
                return fail(RTMI_ERR_INVALID, "emitters: triangle " + std::to_string(g) + " is marked and its surface is not Solid");
        }
    }
    RTMI_GUARD_BEGIN
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(hipDeviceSynchronize());  // no render of this scene is in flight: its streams are done with the old tables
    s->emtab_ok = false;
    s->emtab = EmTab{};
    s->em_tris.clear();
    s->em_corners.clear();
    if (!set) return RTMI_OK;
    for (uint64_t g = 1; g < n; g++)
        if (emit_of_tri[g]) {
            s->em_tris.push_back((uint32_t)g);
            s->em_corners.insert(s->em_corners.end(), corners9 + 9 * g, corners9 + 9 * g + 9);
        }
    return RTMI_OK;
    RTMI_GUARD_END
}

// The lamps' tables (emissive.hpp), built once per set of marks: the records and wmax (a thread per lamp), then q and the prefix
// sums (one block).  The triangle -> lamp index is integers only and comes from the host's list.
static int ensure_emitters(rtmi_scene_t* s) {
    if (s->emtab_ok) return RTMI_OK;
    RTMI_GUARD_BEGIN
    const uint32_t n = (uint32_t)s->em_tris.size(), ntris = s->d.ntris;
    std::vector<uint32_t> idx(ntris, 0u);
    std::vector<float4> cs((size_t)n * 3);
    for (uint32_t k = 0; k < n; k++) {
        idx[s->em_tris[k]] = k + 1u;
        const float* c = &s->em_corners[(size_t)9 * k];
        for (int j = 0; j < 3; j++) cs[(size_t)3 * k + j] = make_float4(c[3 * j], c[3 * j + 1], c[3 * j + 2], 0.f);
    }
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(s->em_idx.ensure(ntris)); HIPCHK(s->em_list.ensure(n)); HIPCHK(s->em_c.ensure((size_t)n * 3));
    HIPCHK(s->em_lamp.ensure((size_t)n * RTMI_EMISSIVE_REC)); HIPCHK(s->em_q.ensure(n)); HIPCHK(s->em_cum.ensure((size_t)n + 1));
    HIPCHK(s->em_max.ensure(1));
    HIPCHK(hipMemcpy(s->em_idx.p, idx.data(), (size_t)ntris * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(s->em_list.p, s->em_tris.data(), (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(s->em_c.p, cs.data(), cs.size() * sizeof(float4), hipMemcpyHostToDevice));
    HIPCHK(hipMemsetAsync(s->em_max.p, 0, sizeof(uint32_t), 0));
    hipLaunchKernelGGL(k_emq_lamps, dim3((n + 255u) / 256u), dim3(256), 0, 0, s->d, s->em_list.p, s->em_c.p, n, s->em_lamp.p, s->em_max.p);
    hipLaunchKernelGGL(k_emq_scan, dim3(1), dim3(256), 0, 0, s->em_lamp.p, n, s->em_max.p, s->em_q.p, s->em_cum.p, s->em_cum.p + n);
    HIPCHK(hipGetLastError());
    unsigned long long total = 0ull;
    HIPCHK(hipMemcpy(&total, s->em_cum.p + n, sizeof total, hipMemcpyDeviceToHost));  // (synchronises with the two kernels)
    s->emtab = EmTab{s->em_idx.p, s->em_lamp.p, s->em_q.p, s->em_cum.p, total, n};
    s->emtab_ok = true;
    return RTMI_OK;
    RTMI_GUARD_END
}

int rtmi_scene_get_emitter_sampler(rtmi_scene_t* s, uint32_t* q_out, uint64_t* cum_out, uint32_t* lamp_of_tri_out, float* lamps_out,
                                   uint64_t* total_out, uint32_t* n_out) {
    if (!s || !n_out) return fail(RTMI_ERR_INVALID, "NULL argument");
    const uint32_t n = (uint32_t)s->em_tris.size();
    *n_out = n;
    if (total_out) *total_out = 0u;
    if (n == 0u) return RTMI_OK;
    const int rc = ensure_emitters(s);
    if (rc != RTMI_OK) return rc;
    if (total_out) *total_out = s->emtab.total;
    if (q_out) HIPCHK(hipMemcpy(q_out, s->em_q.p, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (cum_out) HIPCHK(hipMemcpy(cum_out, s->em_cum.p, (size_t)n * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (lamp_of_tri_out) HIPCHK(hipMemcpy(lamp_of_tri_out, s->em_idx.p, (size_t)s->d.ntris * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (lamps_out) HIPCHK(hipMemcpy(lamps_out, s->em_lamp.p, (size_t)n * RTMI_EMISSIVE_REC * sizeof(float4), hipMemcpyDeviceToHost));
    return RTMI_OK;
}

// scenes the call does not take; before any HIP call
static int refuse_scene_emissive(const rtmi_scene_t* s) {
    if (s->em_tris.empty()) return fail(RTMI_ERR_UNSUPPORTED, "emissive: the scene has no emitters (rtmi_scene_set_emitters)");
    if (s->d.nspheres)
        return fail(RTMI_ERR_UNSUPPORTED, "emissive: the scene has analytic spheres (a build-defined primitive whose normal needs the hit point)");
    if (s->has_dielectric) return fail(RTMI_ERR_UNSUPPORTED, "emissive: the scene has a dielectric surface (the emissive shading has no glass arm)");
    if (s->has_normals) return fail(RTMI_ERR_UNSUPPORTED, "emissive: the scene has vertex normals (the emissive shading has no smooth arm)");
    if (s->has_nmap) return fail(RTMI_ERR_UNSUPPORTED, "emissive: the scene has normal maps (the emissive shading has no normal-map arm)");
    if (s->has_tex) return fail(RTMI_ERR_UNSUPPORTED, "emissive: the scene has textures (the emissive shading has no texture arm)");
    if (s->options & RTMI_OPT_BVH)
        return fail(RTMI_ERR_UNSUPPORTED, "emissive: RTMI_OPT_BVH (a non-exact first hit would break the test that a shadow ray's first hit is its lamp)");
    return RTMI_OK;
}

int rtmi_render_emissive_device(rtmi_scene_t* s, const rtmi_viewport_t* vp, uint64_t seed, const rtmi_tile_t* tile, uint32_t sample0,
                                uint32_t nsamples, void* accum_device, void* out_device, void* hip_stream, rtmi_stats_t* stats) {
    if (stats) memset(stats, 0, sizeof(*stats));
    int rc = check_samples(s, vp, sample0, nsamples, accum_device, out_device);
    if (rc != RTMI_OK) return rc;
    if (!tile) return fail(RTMI_ERR_INVALID, "NULL argument (tile)");
    if (tile->nrows == 0) return RTMI_OK;
    rc = check_view(vp, tile);
    if (rc != RTMI_OK) return rc;
    rc = refuse_scene_emissive(s);
    if (rc != RTMI_OK) return rc;
    if (vp->maxdepth != 0) {  // (depth 0 writes zeros and needs no table)
        rc = ensure_emitters(s);
        if (rc != RTMI_OK) return rc;
    }
    ShadowCall call{};
    call.em = &s->emtab;
    return render_tile(s, vp, seed, tile, sample0, nsamples, (float4*)accum_device, out_device, hip_stream, stats, nullptr, 0, nullptr,
                       nullptr, nullptr, nullptr, &call);
}

// Host variant: rtmi_render_samples' copies (accum in only when sample0 > 0, accum and out back).
int rtmi_render_emissive(rtmi_scene_t* s, const rtmi_viewport_t* vp, uint64_t seed, uint32_t row0, uint32_t nrows, uint32_t sample0,
                         uint32_t nsamples, float* accum_host, float* out_host, rtmi_stats_t* stats) {
    if (stats) memset(stats, 0, sizeof(*stats));
    int rc = check_samples(s, vp, sample0, nsamples, accum_host, out_host);
    if (rc != RTMI_OK) return rc;
    const uint64_t npix = (uint64_t)nrows * vp->width;
    if (npix == 0) return RTMI_OK;
    if ((uint64_t)row0 + nrows > vp->height) return fail(RTMI_ERR_INVALID, "row range outside the viewport");
    const rtmi_tile_t tile{row0, nrows, nrows, 0u};
    rc = check_view(vp, &tile);
    if (rc != RTMI_OK) return rc;
    rc = refuse_scene_emissive(s);
    if (rc != RTMI_OK) return rc;
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(s->acc.ensure(npix));
    if (out_host) HIPCHK(s->tile.ensure(npix));
    if (sample0 > 0) HIPCHK(hipMemcpy(s->acc.p, accum_host, npix * sizeof(float4), hipMemcpyHostToDevice));
    rc = rtmi_render_emissive_device(s, vp, seed, &tile, sample0, nsamples, s->acc.p, out_host ? (void*)s->tile.p : nullptr, nullptr, stats);
    if (rc != RTMI_OK) return rc;
    HIPCHK(hipMemcpy(accum_host, s->acc.p, npix * sizeof(float4), hipMemcpyDeviceToHost));
    if (out_host) HIPCHK(hipMemcpy(out_host, s->tile.p, npix * sizeof(float4), hipMemcpyDeviceToHost));
    return RTMI_OK;
}

// ---------------------------------------------------------------- box lights in the path (rtmi_render_lit*)
void rtmi_lit_defaults(rtmi_lit_t* p) {
    if (!p) return;
    p->nlights = 0; p->flags = 0;
    for (int l = 0; l < RTMI_LIT_MAX_LIGHTS; l++) {
        rtmi_light_defaults(&p->lights[l]);
        p->lights[l].rays = 1;
        p->light_color[l][0] = p->light_color[l][1] = p->light_color[l][2] = 1.f;
    }
}

// Checks of the lit entry points that come before any HIP call and before the scene is used: rtmi_render_samples_device's, then
// the parameters, each used light as rtmi_render_shadowed* checks its one
static int check_lit_params(const rtmi_lit_t* p);
static int check_lit(rtmi_scene_t* s, const rtmi_viewport_t* vp, uint32_t sample0, uint32_t nsamples, const rtmi_lit_t* p, const void* accum,
                     const void* out) {
    const int rc = check_samples(s, vp, sample0, nsamples, accum, out);
    if (rc != RTMI_OK) return rc;
    return check_lit_params(p);
}
// the parameters alone: rtmi_render_rays_lit* and rtmi_bake_lit* make these checks after their own
static int check_lit_params(const rtmi_lit_t* p) {
    if (!p) return fail(RTMI_ERR_INVALID, "lit: NULL argument (rtmi_lit_t)");
    if (p->nlights > (uint32_t)RTMI_LIT_MAX_LIGHTS) return fail(RTMI_ERR_INVALID, "lit: nlights above RTMI_LIT_MAX_LIGHTS");
    if (p->flags & ~(uint32_t)(RTMI_LIT_INVERSE_SQUARE | RTMI_LIT_SURFACES)) return fail(RTMI_ERR_INVALID, "lit: unknown flags");
    for (uint32_t l = 0; l < p->nlights; l++) {
        const rtmi_light_t& li = p->lights[l];
        char msg[160];
        const char* bad = nullptr;
        if (li.rays == 0 || li.rays > 256) bad = "rays must be in [1, 256]";
        else if (li.flags & ~(uint32_t)RTMI_LIGHT_UNBOUNDED) bad = "unknown flags";
        else if (!(li.len2 >= 0.f) || std::isinf(li.len2)) bad = "len2 must be >= 0, finite and not NaN";
        else if (!std::isfinite(li.orig[0]) || !std::isfinite(li.orig[1]) || !std::isfinite(li.orig[2])) bad = "orig must be finite";
        else if (!std::isfinite(li.bias)) bad = "bias must be finite";
        else if (li.rays != 1) bad = "rays must be 1 (one shadow ray per light and hit)";
        else if (!std::isfinite(p->light_color[l][0]) || !std::isfinite(p->light_color[l][1]) || !std::isfinite(p->light_color[l][2]))
            bad = "light_color must be finite";
        if (bad) {
            snprintf(msg, sizeof msg, "lit: light %u: %s", l, bad);
            return fail(RTMI_ERR_INVALID, msg);
        }
    }
    return RTMI_OK;
}
// scenes the lit shading (lit.hpp has its own shade_hit) does not take; before any HIP call.  An environment is fine.  With
// RTMI_LIT_SURFACES in the call's flags only analytic spheres are refused: the surface features run through the *_surf kernels.
static int refuse_scene_lit(const rtmi_scene_t* s, uint32_t flags) {
    if (s->d.nspheres)
        return fail(RTMI_ERR_UNSUPPORTED, "lit: the scene has analytic spheres (a build-defined primitive whose normal needs the hit point)");
    if (flags & RTMI_LIT_SURFACES) return RTMI_OK;
    if (s->has_dielectric) return fail(RTMI_ERR_UNSUPPORTED, "lit: the scene has a dielectric surface (the lit shading has no glass arm)");
    if (s->has_normals) return fail(RTMI_ERR_UNSUPPORTED, "lit: the scene has vertex normals (the lit shading has no smooth arm)");
    if (s->has_nmap) return fail(RTMI_ERR_UNSUPPORTED, "lit: the scene has normal maps (the lit shading has no normal-map arm)");
    if (s->has_tex) return fail(RTMI_ERR_UNSUPPORTED, "lit: the scene has textures (the lit shading has no texture arm)");
    return RTMI_OK;
}
static LitArgs lit_args(const rtmi_lit_t& p) {
    LitArgs a{};
    a.nlights = p.nlights;
    a.inverse_square = (p.flags & RTMI_LIT_INVERSE_SQUARE) ? 1u : 0u;
    for (uint32_t l = 0; l < p.nlights; l++) {
        const rtmi_light_t& li = p.lights[l];
        LitLight& d = a.li[l];
        d.orig = mk(li.orig[0], li.orig[1], li.orig[2]);
        d.len2 = li.len2; d.bias = li.bias;
        d.unbounded = (li.flags & RTMI_LIGHT_UNBOUNDED) ? 1u : 0u;
        for (int c = 0; c < 3; c++) d.col[c] = p.light_color[l][c];
    }
    return a;
}

int rtmi_render_lit_device(rtmi_scene_t* s, const rtmi_viewport_t* vp, uint64_t seed, const rtmi_tile_t* tile, uint32_t sample0,
                           uint32_t nsamples, const rtmi_lit_t* lit, void* accum_device, void* out_device, void* hip_stream,
                           rtmi_stats_t* stats) {
    if (stats) memset(stats, 0, sizeof(*stats));
    int rc = check_lit(s, vp, sample0, nsamples, lit, accum_device, out_device);
    if (rc != RTMI_OK) return rc;
    if (!tile) return fail(RTMI_ERR_INVALID, "NULL argument (tile)");
    if (tile->nrows == 0) return RTMI_OK;
    rc = check_view(vp, tile);
    if (rc != RTMI_OK) return rc;
    rc = refuse_scene_lit(s, lit->flags);
    if (rc != RTMI_OK) return rc;
    const LitArgs la = lit_args(*lit);
    ShadowCall call{};
    call.lit = &la;
    return render_tile(s, vp, seed, tile, sample0, nsamples, (float4*)accum_device, out_device, hip_stream, stats, nullptr, 0, nullptr,
                       nullptr, nullptr, nullptr, &call);
}

// Host variant: rtmi_render_samples' copies (accum in only when sample0 > 0, accum and out back).
int rtmi_render_lit(rtmi_scene_t* s, const rtmi_viewport_t* vp, uint64_t seed, uint32_t row0, uint32_t nrows, uint32_t sample0,
                    uint32_t nsamples, const rtmi_lit_t* lit, float* accum_host, float* out_host, rtmi_stats_t* stats) {
    if (stats) memset(stats, 0, sizeof(*stats));
    int rc = check_lit(s, vp, sample0, nsamples, lit, accum_host, out_host);
    if (rc != RTMI_OK) return rc;
    const uint64_t npix = (uint64_t)nrows * vp->width;
    if (npix == 0) return RTMI_OK;
    if ((uint64_t)row0 + nrows > vp->height) return fail(RTMI_ERR_INVALID, "row range outside the viewport");
    const rtmi_tile_t tile{row0, nrows, nrows, 0u};
    rc = check_view(vp, &tile);
    if (rc != RTMI_OK) return rc;
    rc = refuse_scene_lit(s, lit->flags);
    if (rc != RTMI_OK) return rc;
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(s->acc.ensure(npix));
    if (out_host) HIPCHK(s->tile.ensure(npix));
    if (sample0 > 0) HIPCHK(hipMemcpy(s->acc.p, accum_host, npix * sizeof(float4), hipMemcpyHostToDevice));
    rc = rtmi_render_lit_device(s, vp, seed, &tile, sample0, nsamples, lit, s->acc.p, out_host ? (void*)s->tile.p : nullptr, nullptr, stats);
    if (rc != RTMI_OK) return rc;
    HIPCHK(hipMemcpy(accum_host, s->acc.p, npix * sizeof(float4), hipMemcpyDeviceToHost));
    if (out_host) HIPCHK(hipMemcpy(out_host, s->tile.p, npix * sizeof(float4), hipMemcpyDeviceToHost));
    return RTMI_OK;
}

// ---------------------------------------------------------------- shaded preview (rtmi_render_preview*)
void rtmi_preview_defaults(rtmi_preview_t* p) {
    if (!p) return;
    p->ambient[0] = p->ambient[1] = p->ambient[2] = 0.3f;
    p->nlights = 0; p->flags = 0;
    rtmi_ao_defaults(&p->ao);
    for (int l = 0; l < RTMI_PREVIEW_MAX_LIGHTS; l++) {
        rtmi_light_defaults(&p->lights[l]);
        p->light_color[l][0] = p->light_color[l][1] = p->light_color[l][2] = 1.f;
    }
}

// Checks of the preview entry points that come before any HIP call and before the scene is used (a CPU-only caller reaches
// them).  RTMI_OK with *empty set: the tile has no rows, nothing to do.  v1 receives the viewport with maxdepth = 1, as for
// features.  The outputs' byte ranges are those of a tile of tile->nrows rows.
static int check_preview(rtmi_scene_t* s, const rtmi_viewport_t* vp, const rtmi_tile_t* tile, uint32_t sample0, uint32_t nsamples,
                         const rtmi_preview_t* pv, const rtmi_preview_out_t* out, rtmi_viewport_t& v1, bool* empty) {
    *empty = false;
    if (!s || !vp) return fail(RTMI_ERR_INVALID, "preview: NULL argument (scene or viewport)");
    if (!tile) return fail(RTMI_ERR_INVALID, "preview: NULL argument (tile)");
    if (!pv) return fail(RTMI_ERR_INVALID, "preview: NULL argument (rtmi_preview_t)");
    if (!out) return fail(RTMI_ERR_INVALID, "preview: NULL argument (rtmi_preview_out_t)");
    if (!out->color && !out->albedo && !out->normal && !out->ids && !out->ao && !out->shadow && !out->irradiance)
        return fail(RTMI_ERR_INVALID, "preview: NULL outputs: at least one is required");
    if (pv->nlights > RTMI_PREVIEW_MAX_LIGHTS) return fail(RTMI_ERR_INVALID, "preview: nlights must be in [0, 4]");
    if (pv->flags != 0) return fail(RTMI_ERR_INVALID, "preview: flags must be 0");
    for (int c = 0; c < 3; c++)
        if (!std::isfinite(pv->ambient[c])) return fail(RTMI_ERR_INVALID, "preview: ambient must be finite");
    const rtmi_ao_t& ao = pv->ao;
    if (ao.rays > 256) return fail(RTMI_ERR_INVALID, "preview: ao.rays must be in [0, 256]");
    if (ao.flags != 0) return fail(RTMI_ERR_INVALID, "preview: ao.flags must be 0");
    if (!(ao.radius >= 0.f)) return fail(RTMI_ERR_INVALID, "preview: ao.radius must be >= 0 (+inf: unlimited) and not NaN");
    if (!std::isfinite(ao.bias)) return fail(RTMI_ERR_INVALID, "preview: ao.bias must be finite");
    for (uint32_t l = 0; l < pv->nlights; l++) {
        const rtmi_light_t& li = pv->lights[l];
        const std::string who = "preview: light " + std::to_string(l) + ": ";
        if (li.rays == 0 || li.rays > 256) return fail(RTMI_ERR_INVALID, who + "rays must be in [1, 256]");
        if (li.flags & ~(uint32_t)RTMI_LIGHT_UNBOUNDED) return fail(RTMI_ERR_INVALID, who + "unknown flags");
        if (!(li.len2 >= 0.f) || std::isinf(li.len2)) return fail(RTMI_ERR_INVALID, who + "len2 must be >= 0, finite and not NaN");
        if (!std::isfinite(li.orig[0]) || !std::isfinite(li.orig[1]) || !std::isfinite(li.orig[2]))
            return fail(RTMI_ERR_INVALID, who + "orig must be finite");
        if (!std::isfinite(li.bias)) return fail(RTMI_ERR_INVALID, who + "bias must be finite");
        for (int c = 0; c < 3; c++)
            if (!std::isfinite(pv->light_color[l][c])) return fail(RTMI_ERR_INVALID, who + "colour must be finite");
    }
    if (out->ao && ao.rays == 0) return fail(RTMI_ERR_INVALID, "preview: an ao output needs ao.rays >= 1");
    if ((out->shadow || out->irradiance) && pv->nlights == 0)
        return fail(RTMI_ERR_INVALID, "preview: shadow / irradiance outputs need nlights >= 1");
    if (vp->samples_per_pixel == 0) return fail(RTMI_ERR_INVALID, "samples_per_pixel must be >= 1");
    if (nsamples == 0) return fail(RTMI_ERR_INVALID, "nsamples must be >= 1");
    if ((uint64_t)sample0 + nsamples > vp->samples_per_pixel)
        return fail(RTMI_ERR_INVALID, "samples [sample0, sample0 + nsamples) outside the frame's samples_per_pixel");
    if (sample0 & RTMI_KEY_JITTER) return fail(RTMI_ERR_UNSUPPORTED, "sample0 above 2^31");  // DView::sample_key
    {   // no two outputs may overlap as byte ranges
        const uint64_t npix = (uint64_t)tile->nrows * vp->width;
        const void* ptr[7] = {out->color, out->albedo, out->normal, out->ids, out->ao, out->shadow, out->irradiance};
        const uint64_t len[7] = {16 * npix, 16 * npix, 16 * npix, 4 * npix, 4 * npix, 4 * npix * pv->nlights, 4 * npix * pv->nlights};
        for (int i = 0; i < 7; i++)
            for (int j = i + 1; j < 7; j++) {
                if (!ptr[i] || !ptr[j]) continue;
                const uintptr_t a = (uintptr_t)ptr[i], b = (uintptr_t)ptr[j];
                if (a == b || (a < b ? b - a < len[i] : a - b < len[j])) return fail(RTMI_ERR_INVALID, "preview: outputs must not overlap");
            }
    }
    if ((uint64_t)nsamples * ao.rays >= (1ull << 24))
        return fail(RTMI_ERR_UNSUPPORTED, "preview: nsamples * ao.rays must stay below 2^24 (the per-pixel count is exact in f32)");
    for (uint32_t l = 0; l < pv->nlights; l++)
        if ((uint64_t)nsamples * pv->lights[l].rays >= (1ull << 24))
            return fail(RTMI_ERR_UNSUPPORTED, "preview: light " + std::to_string(l) + ": nsamples * rays must stay below 2^24 (the per-pixel count is exact in f32)");
    if (tile->nrows == 0) { *empty = true; return RTMI_OK; }
    v1 = *vp;
    v1.maxdepth = 1;
    return check_view(&v1, tile);
}

// The call as the kernels take it; out's pointers are device memory
static PreviewCall preview_call(const rtmi_preview_t& pv, const rtmi_preview_out_t& out, uint64_t npix) {
    PreviewCall c{};
    for (int k = 0; k < 3; k++) c.a.amb[k] = pv.ambient[k];
    c.a.nlights = pv.nlights;
    c.a.Ka = pv.ao.rays; c.a.dKa = make_fastdiv(pv.ao.rays);
    c.a.radius = pv.ao.radius; c.a.abias = pv.ao.bias;
    uint32_t koff = 0;
    for (uint32_t l = 0; l < RTMI_PV_MAX_LIGHTS; l++) {
        PvLight& L = c.a.li[l];
        L = PvLight{};
        L.K = 1; L.dK = make_fastdiv(1);
        if (l >= pv.nlights) continue;
        const rtmi_light_t& li = pv.lights[l];
        L.orig = mk(li.orig[0], li.orig[1], li.orig[2]);
        L.len2 = li.len2; L.bias = li.bias;
        L.K = li.rays; L.koff = koff; L.dK = make_fastdiv(li.rays);
        L.unbounded = (li.flags & RTMI_LIGHT_UNBOUNDED) ? 1u : 0u;
        for (int k = 0; k < 3; k++) L.col[k] = pv.light_color[l][k];
        koff += li.rays;
    }
    c.per_path = pv.ao.rays + koff;
    c.color = (float4*)out.color;
    c.fo = FeatOut{(float4*)out.albedo, (float4*)out.normal, (uint32_t*)out.ids};
    c.ao = (float*)out.ao; c.shadow = (float*)out.shadow; c.irradiance = (float*)out.irradiance;
    c.plane = (size_t)npix;
    return c;
}

int rtmi_render_preview_device(rtmi_scene_t* s, const rtmi_viewport_t* vp, uint64_t seed, const rtmi_tile_t* tile, uint32_t sample0,
                               uint32_t nsamples, const rtmi_preview_t* preview, const rtmi_preview_out_t* out_device, void* hip_stream,
                               rtmi_stats_t* stats) {
    if (stats) memset(stats, 0, sizeof(*stats));
    rtmi_viewport_t v1;
    bool empty;
    const int rc = check_preview(s, vp, tile, sample0, nsamples, preview, out_device, v1, &empty);
    if (rc != RTMI_OK || empty) return rc;
    if (s->d.nspheres)
        return fail(RTMI_ERR_UNSUPPORTED, "preview: the scene has analytic spheres (a build-defined primitive whose normal needs the hit point)");
    if (s->has_tex)
        return fail(RTMI_ERR_UNSUPPORTED, "preview: the scene has textures (the preview's composition has no texture arm)");
    const PreviewCall call = preview_call(*preview, *out_device, (uint64_t)tile->nrows * vp->width);
    return render_tile(s, &v1, seed, tile, sample0, nsamples, nullptr, nullptr, hip_stream, stats, nullptr, 0, nullptr, nullptr, nullptr, &call);
}

// Host variant: the requested outputs are rendered into the handle's own device buffers and copied out once.
int rtmi_render_preview(rtmi_scene_t* s, const rtmi_viewport_t* vp, uint64_t seed, uint32_t row0, uint32_t nrows, uint32_t sample0,
                        uint32_t nsamples, const rtmi_preview_t* preview, const rtmi_preview_out_t* out_host, rtmi_stats_t* stats) {
    if (stats) memset(stats, 0, sizeof(*stats));
    const rtmi_tile_t tile{row0, nrows, nrows ? nrows : 1u, 0u};
    rtmi_viewport_t v1;
    bool empty;
    const int rc0 = check_preview(s, vp, &tile, sample0, nsamples, preview, out_host, v1, &empty);
    if (rc0 != RTMI_OK || empty) return rc0;
    if (s->d.nspheres)
        return fail(RTMI_ERR_UNSUPPORTED, "preview: the scene has analytic spheres (a build-defined primitive whose normal needs the hit point)");
    if (s->has_tex)
        return fail(RTMI_ERR_UNSUPPORTED, "preview: the scene has textures (the preview's composition has no texture arm)");
    const uint64_t npix = (uint64_t)nrows * vp->width;
    const uint32_t nl = preview->nlights;
    HIPCHK(hipSetDevice(s->device));
    // float4 images: colour, albedo, normal; f32 / u32 planes: ids, ao, nl shadow planes, nl irradiance planes
    HIPCHK(s->pv_out4.ensure(3 * npix));
    HIPCHK(s->pv_out1.ensure((2 + 2 * (uint64_t)nl) * npix));
    rtmi_preview_out_t d{};
    d.color = out_host->color ? s->pv_out4.p : nullptr;
    d.albedo = out_host->albedo ? s->pv_out4.p + npix : nullptr;
    d.normal = out_host->normal ? s->pv_out4.p + 2 * npix : nullptr;
    d.ids = out_host->ids ? s->pv_out1.p : nullptr;
    d.ao = out_host->ao ? s->pv_out1.p + npix : nullptr;
    d.shadow = out_host->shadow ? s->pv_out1.p + 2 * npix : nullptr;
    d.irradiance = out_host->irradiance ? s->pv_out1.p + (2 + (uint64_t)nl) * npix : nullptr;
    const PreviewCall call = preview_call(*preview, d, npix);
    const int rc = render_tile(s, &v1, seed, &tile, sample0, nsamples, nullptr, nullptr, nullptr, stats, nullptr, 0, nullptr, nullptr, nullptr, &call);
    if (rc != RTMI_OK) return rc;
    const void* src[7] = {d.color, d.albedo, d.normal, d.ids, d.ao, d.shadow, d.irradiance};
    void* dst[7] = {out_host->color, out_host->albedo, out_host->normal, out_host->ids, out_host->ao, out_host->shadow, out_host->irradiance};
    const uint64_t len[7] = {16 * npix, 16 * npix, 16 * npix, 4 * npix, 4 * npix, 4 * npix * nl, 4 * npix * nl};
    for (int k = 0; k < 7; k++)
        if (dst[k]) HIPCHK(hipMemcpy(dst[k], src[k], len[k], hipMemcpyDeviceToHost));
    return RTMI_OK;
}

// ---------------------------------------------------------------- adaptive sampling
// Checks of the adaptive entry points that come before any HIP call (a CPU-only caller reaches them).  bufs: the caller's
// buffers, nbufs of them, none NULL except an optional last one (out); no two may be the same.
static int check_adaptive(rtmi_scene_t* s, const rtmi_viewport_t* vp, const rtmi_adaptive_t* ad, const void* const* bufs,
                          int nbufs, bool last_optional) {
    if (!s || !vp) return fail(RTMI_ERR_INVALID, "NULL argument (scene or viewport)");
    if (!ad) return fail(RTMI_ERR_INVALID, "NULL argument (rtmi_adaptive_t)");
    const uint32_t S = vp->samples_per_pixel;
    if (S < 2) return fail(RTMI_ERR_INVALID, "adaptive sampling needs samples_per_pixel >= 2");
    if (ad->min_samples < 2 || ad->min_samples > S) return fail(RTMI_ERR_INVALID, "min_samples must be in [2, samples_per_pixel]");
    if (ad->pass_samples == 0) return fail(RTMI_ERR_INVALID, "pass_samples must be >= 1");
    if (S & RTMI_KEY_JITTER) return fail(RTMI_ERR_UNSUPPORTED, "samples_per_pixel above 2^31");  // DView::sample_key
    for (int i = 0; i < nbufs; i++) {
        if (!bufs[i] && !(last_optional && i == nbufs - 1)) return fail(RTMI_ERR_INVALID, "NULL buffer (accum, sumsq and counts are required)");
        for (int j = 0; j < i; j++)
            if (bufs[i] && bufs[i] == bufs[j]) return fail(RTMI_ERR_INVALID, "buffers must not alias (accum, sumsq, counts, out)");
    }
    return RTMI_OK;
}

// The passes of one adaptive call on device buffers (checked): pass 0 renders samples [0, m) of the whole tile; after each
// pass k_adapt_* apply the stop rule to the active pixels and compact the survivors into the next list, whose length
// (4 bytes) is read back to size the next pass.  Everything is enqueued on `ust`; every pass ends synchronised.
static int render_adaptive(rtmi_scene_t* s, const rtmi_viewport_t* vp, uint64_t seed, const rtmi_tile_t* tile,
                           rtmi_adaptive_t* ad, float4* accum, float4* sumsq, uint32_t* counts, float4* out, hipStream_t ust,
                           rtmi_stats_t* stats) {
    ad->passes = 0; ad->unconverged = 0; ad->samples = 0;
    if (tile->nrows == 0) return RTMI_OK;
    RTMI_GUARD_BEGIN
    (void)hipGetLastError();
    int rc = check_view(vp, tile);
    if (rc != RTMI_OK) return rc;
    HIPCHK(hipSetDevice(s->device));
    const uint32_t S = vp->samples_per_pixel, m = ad->min_samples, p = ad->pass_samples;
    const uint32_t npix = (uint32_t)((uint64_t)tile->nrows * vp->width);
    if (vp->maxdepth == 0) {  // every sample is black: zero variance, every pixel stops at m
        HIPCHK(hipMemsetAsync(accum, 0, (size_t)npix * sizeof(float4), ust));
        HIPCHK(hipMemsetAsync(sumsq, 0, (size_t)npix * sizeof(float4), ust));
        HIPCHK(hipMemsetD32Async((hipDeviceptr_t)counts, (int)m, npix, ust));
        if (out) HIPCHK(hipMemsetAsync(out, 0, (size_t)npix * sizeof(float4), ust));
        HIPCHK(hipStreamSynchronize(ust));
        ad->passes = 1; ad->samples = (uint64_t)npix * m;
        return RTMI_OK;
    }
    const uint32_t nblk = (npix + RTMI_ADAPT_BLOCK - 1) / RTMI_ADAPT_BLOCK;
    HIPCHK(s->alist[0].ensure(npix));
    HIPCHK(s->alist[1].ensure(npix));
    HIPCHK(s->ablk.ensure((size_t)nblk + 1));
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    HIPCHK(hipEventCreate(&ev0));
    struct EvGuard { hipEvent_t& a; hipEvent_t& b; ~EvGuard() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); } } evg{ev0, ev1};
    HIPCHK(hipEventCreate(&ev1));
    HIPCHK(hipEventRecord(ev0, ust));
    const unsigned ew_blocks = (unsigned)(s->num_cu * 8);
    hipLaunchKernelGGL(k_adapt_init, dim3(std::min<unsigned>(ew_blocks, (npix + 255) / 256)), dim3(256), 0, ust, npix, s->alist[0].p);
    HIPCHK(hipGetLastError());
    uint32_t n0 = 0, k = m, nact = npix, cur = 0, streams = 0;
    for (;;) {
        const ListPass lp{s->alist[cur].p, nact, sumsq, counts};
        rtmi_stats_t ps;
        rc = render_tile(s, vp, seed, tile, n0, k, accum, out, ust, &ps, &lp);
        if (rc != RTMI_OK) return rc;
        ad->passes++;
        ad->samples += (uint64_t)nact * k;
        if (stats) {
            add_counters(*stats, ps);
            stats->trace_ms += ps.trace_ms; stats->trace_launches += ps.trace_launches;
            stats->primary_ms += ps.primary_ms; stats->bounce_ms += ps.bounce_ms; stats->pipeline = ps.pipeline;
        }
        streams = std::max(streams, ps.streams);
        const uint32_t n = n0 + k;
        // the stop rule on the pass's pixels; at n == S they all stop, and the survivors' count is the unconverged pixels
        const unsigned nb = (nact + RTMI_ADAPT_BLOCK - 1) / RTMI_ADAPT_BLOCK;
        hipLaunchKernelGGL(k_adapt_count, dim3(nb), dim3(RTMI_ADAPT_BLOCK), 0, ust, s->alist[cur].p, nact, accum, sumsq, n,
                           ad->rel_tol, ad->abs_tol, s->ablk.p);
        hipLaunchKernelGGL(k_adapt_scan, dim3(1), dim3(256), 0, ust, s->ablk.p, (uint32_t)nb);
        if (n < S)
            hipLaunchKernelGGL(k_adapt_scatter, dim3(nb), dim3(RTMI_ADAPT_BLOCK), 0, ust, s->alist[cur].p, nact, accum, sumsq, n,
                               ad->rel_tol, ad->abs_tol, s->ablk.p, s->alist[cur ^ 1].p);
        HIPCHK(hipGetLastError());
        uint32_t next = 0;
        HIPCHK(hipMemcpyAsync(&next, s->ablk.p + nb, sizeof(uint32_t), hipMemcpyDeviceToHost, ust));
        HIPCHK(hipStreamSynchronize(ust));
        if (n >= S) { ad->unconverged = next; break; }
        if (next == 0) break;
        nact = next; cur ^= 1u; n0 = n; k = std::min(p, S - n);
    }
    HIPCHK(hipEventRecord(ev1, ust));
    HIPCHK(hipEventSynchronize(ev1));
    float kernel_ms = 0.f;
    HIPCHK(hipEventElapsedTime(&kernel_ms, ev0, ev1));
    if (stats) { stats->kernel_ms = kernel_ms; stats->streams = streams; }
    return RTMI_OK;
    RTMI_GUARD_END
}

int rtmi_render_adaptive_device(rtmi_scene_t* s, const rtmi_viewport_t* vp, uint64_t seed, const rtmi_tile_t* tile,
                                rtmi_adaptive_t* ad, void* accum_device, void* sumsq_device, void* counts_device, void* out_device,
                                void* hip_stream, rtmi_stats_t* stats) {
    if (stats) memset(stats, 0, sizeof(*stats));
    const void* bufs[4] = {accum_device, sumsq_device, counts_device, out_device};
    const int rc = check_adaptive(s, vp, ad, bufs, 4, true);
    if (rc != RTMI_OK) return rc;
    if (!tile) return fail(RTMI_ERR_INVALID, "NULL argument (tile)");
    return render_adaptive(s, vp, seed, tile, ad, (float4*)accum_device, (float4*)sumsq_device, (uint32_t*)counts_device,
                           (float4*)out_device, (hipStream_t)hip_stream, stats);
}

// Host variant: accum and sumsq stay on the device; out and counts are copied back once at the end.
int rtmi_render_adaptive(rtmi_scene_t* s, const rtmi_viewport_t* vp, uint64_t seed, uint32_t row0, uint32_t nrows,
                         rtmi_adaptive_t* ad, float* out_host, uint32_t* counts_host, rtmi_stats_t* stats) {
    if (stats) memset(stats, 0, sizeof(*stats));
    const void* bufs[2] = {out_host, counts_host};
    const int rc0 = check_adaptive(s, vp, ad, bufs, 2, false);
    if (rc0 != RTMI_OK) return rc0;
    ad->passes = 0; ad->unconverged = 0; ad->samples = 0;
    const uint64_t npix = (uint64_t)nrows * vp->width;
    if (npix == 0) return RTMI_OK;
    if ((uint64_t)row0 + nrows > vp->height) return fail(RTMI_ERR_INVALID, "row range outside the viewport");
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(s->acc.ensure(npix));
    HIPCHK(s->asq.ensure(npix));
    HIPCHK(s->acnt.ensure(npix));
    HIPCHK(s->tile.ensure(npix));
    const rtmi_tile_t tile{row0, nrows, nrows, 0u};
    int rc = render_adaptive(s, vp, seed, &tile, ad, s->acc.p, s->asq.p, s->acnt.p, s->tile.p, nullptr, stats);
    if (rc != RTMI_OK) return rc;
    HIPCHK(hipMemcpy(out_host, s->tile.p, npix * sizeof(float4), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(counts_host, s->acnt.p, npix * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return RTMI_OK;
}

// ---------------------------------------------------------------- batches of views
// Checks of the views entry points, before any HIP call and before the scene is used: the arguments, the shared fields of
// the views (the first view that differs is named), every check check_view makes for one view, the size of the stacked
// image and (tile != nullptr, nrows >= 1) the tile against it.  stack receives the stacked viewport: view 0 with
// height = nviews * height.
static int check_views(rtmi_scene_t* s, const rtmi_viewport_t* vps, const uint64_t* seeds, uint32_t nviews, const rtmi_tile_t* tile,
                       const void* out, rtmi_viewport_t& stack) {
    if (!s) return fail(RTMI_ERR_INVALID, "NULL argument (scene)");
    if (!vps || !seeds) return fail(RTMI_ERR_INVALID, "NULL argument (viewports or seeds)");
    if (!out) return fail(RTMI_ERR_INVALID, "NULL argument (output)");
    if (nviews == 0) return fail(RTMI_ERR_INVALID, "nviews must be >= 1");
    const rtmi_viewport_t& v0 = vps[0];
    for (uint32_t k = 1; k < nviews; k++) {
        const rtmi_viewport_t& v = vps[k];
        const char* field = v.width != v0.width ? "width" : v.height != v0.height ? "height" : v.maxdepth != v0.maxdepth ? "maxdepth"
                          : v.samples_per_pixel != v0.samples_per_pixel ? "samples_per_pixel" : nullptr;
        if (field)
            return fail(RTMI_ERR_INVALID, "view " + std::to_string(k) + ": " + field +
                                              " differs from view 0 (the views share width, height, maxdepth and samples_per_pixel)");
    }
    const rtmi_tile_t one_row{0u, 1u, 1u, 0u};
    int rc = check_view(&v0, &one_row);  // what it checks of a view are the shared fields: view 0 speaks for all
    if (rc != RTMI_OK) return fail(rc, "view 0: " + g_err);
    if ((uint64_t)nviews * v0.height * v0.width >= (1ull << 32)) return fail(RTMI_ERR_UNSUPPORTED, "more than 2^32 pixels in the stack of views");
    stack = v0;
    stack.height = nviews * v0.height;
    if (tile && tile->nrows != 0) {
        rc = check_view(&stack, tile);
        if (rc != RTMI_OK) return fail(rc, "stack of " + std::to_string(nviews) + " views: " + g_err);
    }
    return RTMI_OK;
}
// The view table of a call into s->hvcams (the host copy render_tile uploads), once the previous call's upload from it has
// completed
static int set_views(rtmi_scene* s, const rtmi_viewport_t* vps, const uint64_t* seeds, uint32_t nviews) {
    HIPCHK(hipSetDevice(s->device));
    if (s->vcams_ev) HIPCHK(hipEventSynchronize(s->vcams_ev));
    s->hvcams.resize(nviews);
    for (uint32_t k = 0; k < nviews; k++) {
        const rtmi_viewport_t& v = vps[k];
        VCam& c = s->hvcams[k];
        c.orig = make_float4(v.orig[0], v.orig[1], v.orig[2], 0.f);
        c.cam = make_float4(v.cam[0], v.cam[1], v.cam[2], 0.f);
        c.vu = make_float4(v.vu[0], v.vu[1], v.vu[2], 0.f);
        c.vv = make_float4(v.vv[0], v.vv[1], v.vv[2], 0.f);
        c.seed = seeds[k];
        c.pad[0] = c.pad[1] = 0u;
    }
    return RTMI_OK;
}

int rtmi_render_views_device(rtmi_scene_t* s, const rtmi_viewport_t* vps, const uint64_t* seeds, uint32_t nviews,
                             const rtmi_tile_t* tile, void* out_device, void* hip_stream, rtmi_stats_t* stats) {
    if (stats) memset(stats, 0, sizeof(*stats));
    if (!tile) return fail(RTMI_ERR_INVALID, "NULL argument (tile)");
    rtmi_viewport_t stack;
    const int rc = check_views(s, vps, seeds, nviews, tile, out_device, stack);
    if (rc != RTMI_OK) return rc;
    if (tile->nrows == 0) return RTMI_OK;
    // One view has nothing to batch: it is rtmi_render_tile_device's call, on the FRAME kernels (which keep the camera in
    // their launch constants instead of loading it from the table: 0.9 % of a config-3 frame)
    if (nviews == 1) return render_tile(s, &vps[0], seeds[0], tile, 0u, vps[0].samples_per_pixel, nullptr, out_device, hip_stream, stats);
    RTMI_GUARD_BEGIN
    const int rc1 = set_views(s, vps, seeds, nviews);
    if (rc1 != RTMI_OK) return rc1;
    return render_tile(s, &stack, 0u, tile, 0u, stack.samples_per_pixel, nullptr, out_device, hip_stream, stats, nullptr, nviews);
    RTMI_GUARD_END
}

int rtmi_render_views(rtmi_scene_t* s, const rtmi_viewport_t* vps, const uint64_t* seeds, uint32_t nviews, float* out_host,
                      rtmi_stats_t* stats) {
    if (stats) memset(stats, 0, sizeof(*stats));
    rtmi_viewport_t stack;
    const int rc0 = check_views(s, vps, seeds, nviews, nullptr, out_host, stack);
    if (rc0 != RTMI_OK) return rc0;
    const uint64_t npix = (uint64_t)stack.height * stack.width;
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(s->tile.ensure(npix));
    const rtmi_tile_t tile{0u, stack.height, stack.height, 0u};
    const int rc = rtmi_render_views_device(s, vps, seeds, nviews, &tile, s->tile.p, nullptr, stats);
    if (rc != RTMI_OK) return rc;
    HIPCHK(hipMemcpy(out_host, s->tile.p, npix * sizeof(float4), hipMemcpyDeviceToHost));
    return RTMI_OK;
}

int rtmi_render(rtmi_scene_t* s, const rtmi_viewport_t* vp, uint64_t seed, uint32_t row0, uint32_t nrows,
                float* out_host, rtmi_stats_t* stats) {
    if (!s || !vp || !out_host) return fail(RTMI_ERR_INVALID, "NULL argument");
    HIPCHK(hipSetDevice(s->device));
    const uint64_t npix = (uint64_t)nrows * vp->width;
    if (npix == 0) { if (stats) memset(stats, 0, sizeof(*stats)); return RTMI_OK; }
    if ((uint64_t)row0 + nrows > vp->height) return fail(RTMI_ERR_INVALID, "row range outside the viewport");
    HIPCHK(s->tile.ensure(npix));
    int rc = rtmi_render_device(s, vp, seed, row0, nrows, s->tile.p, nullptr, stats);
    if (rc != RTMI_OK) return rc;
    HIPCHK(hipMemcpy(out_host, s->tile.p, npix * sizeof(float4), hipMemcpyDeviceToHost));
    return RTMI_OK;
}

// Direct (xGMI) access from the scene's device to `root`, asked for ONCE per (device, root) pair and remembered on the
// handle: hipDeviceEnablePeerAccess answers hipErrorPeerAccessAlreadyEnabled from the second call on and leaves that
// error pending for the thread's next hipGetLastError() poll (the launch checks of rtmi_render_tile_device).  Whatever the
// answer, the pending error is cleared here; a refusal is recorded (peer_ok = 0, peer_msg) -- hipMemcpyPeerAsync still
// works then, staged by the runtime, and rtmi_render_frame_multi reports it instead of running slowly in silence.
static hipError_t ensure_peer_access(rtmi_scene* sc, int root) {
    if (sc->peer_root == root) return hipSuccess;
    sc->peer_root = root;
    sc->peer_msg.clear();
    if (sc->device == root) { sc->peer_ok = 1; return hipSuccess; }
    const hipError_t pe = hipDeviceEnablePeerAccess(root, 0);
    (void)hipGetLastError();
    sc->peer_ok = (pe == hipSuccess || pe == hipErrorPeerAccessAlreadyEnabled) ? 1 : 0;
    if (!sc->peer_ok) sc->peer_msg = hipGetErrorString(pe);
    return hipSuccess;
}

// Development/test aid (not in rtmi.h): run the peer-access step for `scene` against `root_device` again, as a second
// frame would, and report what is pending afterwards (0 = nothing).  forget != 0 drops the cached answer first.
int rtmi_debug_peer_access(rtmi_scene_t* s, int root_device, int forget, int* peer_ok, int* pending_error) {
    if (!s) return fail(RTMI_ERR_INVALID, "scene is NULL");
    HIPCHK(hipSetDevice(s->device));
    if (forget) s->peer_root = -1;
    HIPCHK(ensure_peer_access(s, root_device));
    if (peer_ok) *peer_ok = s->peer_ok;
    if (pending_error) *pending_error = (int)hipGetLastError();
    return RTMI_OK;
}

int rtmi_render_frame_multi(rtmi_scene_t* const* scenes, uint32_t nscenes, const rtmi_viewport_t* vp, uint64_t seed,
                            uint32_t stripe_rows, uint32_t flags, void* out_host, void* out_device, rtmi_stats_t* stats) {
    if (!scenes || nscenes == 0 || !vp) return fail(RTMI_ERR_INVALID, "NULL argument");
    if (nscenes > 64) return fail(RTMI_ERR_UNSUPPORTED, "more than 64 scene handles");
    for (uint32_t i = 0; i < nscenes; i++) {
        if (!scenes[i]) return fail(RTMI_ERR_INVALID, "scene handle is NULL");
        for (uint32_t j = 0; j < i; j++)
            if (scenes[j] == scenes[i]) return fail(RTMI_ERR_INVALID, "the same scene handle is listed twice (one render in flight per handle)");
    }
    if (!out_host && !out_device) return fail(RTMI_ERR_INVALID, "out_host and out_device are both NULL");
    if (vp->width == 0 || vp->height == 0) return fail(RTMI_ERR_INVALID, "empty viewport");
    if (flags & ~(uint32_t)(RTMI_FRAME_RGB8 | RTMI_FRAME_RCCL)) return fail(RTMI_ERR_INVALID, "unknown flag");
    RTMI_GUARD_BEGIN
    const bool use_rccl = (flags & RTMI_FRAME_RCCL) != 0;
    Rccl* rccl = nullptr;
    if (use_rccl) {
        // one communicator rank per scene handle: RCCL wants every rank on a device of its own
        for (uint32_t i = 0; i < nscenes; i++)
            for (uint32_t j = 0; j < i; j++)
                if (scenes[j]->device == scenes[i]->device)
                    return fail(RTMI_ERR_UNSUPPORTED, "RTMI_FRAME_RCCL needs every scene handle on a device of its own (RCCL refuses two ranks on one GPU)");
        rccl = rccl_api();
        if (!rccl) return fail(RTMI_ERR_UNSUPPORTED, "RTMI_FRAME_RCCL: librccl.so.1 could not be loaded");
    }
    const uint32_t W = vp->width, H = vp->height, n = nscenes;
    const uint32_t S = stripe_rows ? stripe_rows : 16u;
    const bool rgb8 = (flags & RTMI_FRAME_RGB8) != 0;
    const uint32_t px = rgb8 ? 3u : 16u;
    // rows of scene i: stripes i, i+n, i+2n, ... of S rows (the last stripe of the image may be short)
    std::vector<uint32_t> rows(n, 0);
    for (uint32_t k = 0; (uint64_t)k * S < H; k++) rows[k % n] += std::min<uint32_t>(S, H - k * S);
    const uint32_t mr = *std::max_element(rows.begin(), rows.end());
    rtmi_scene* root = scenes[0];
    HIPCHK(hipSetDevice(root->device));
    HIPCHK(root->mstage.ensure((size_t)n * mr * W * px));
    if (!out_device) { HIPCHK(root->mframe.ensure((size_t)H * W * px)); }
    uint8_t* frame = out_device ? (uint8_t*)out_device : root->mframe.p;

    // ---- fan-out: one host thread per scene handle renders its tile and sends the band to the root device
    std::vector<int> rcs(n, RTMI_OK);
    std::vector<std::string> errs(n);
    std::vector<rtmi_stats_t> sts(n);
    using clk = std::chrono::steady_clock;
    auto ms_since = [](clk::time_point t0) { return std::chrono::duration<double, std::milli>(clk::now() - t0).count(); };
    auto work_body = [&](uint32_t i) {
        rtmi_scene* sc = scenes[i];
        rtmi_stats_t& st = sts[i];
        auto bail = [&](int rc, const std::string& msg) { rcs[i] = rc; errs[i] = msg; };
        hipError_t e = hipSetDevice(sc->device);
        if (e == hipSuccess) e = ensure_peer_access(sc, root->device);  // once per (device, root) pair, cached on the handle
        const int peer = sc->peer_ok;
        if (rows[i] == 0) { st.peer_access = peer; return; }
        if (e == hipSuccess && !sc->mstream) e = hipStreamCreateWithFlags(&sc->mstream, hipStreamNonBlocking);
        // (a gather sends the same count from every rank: the band buffers then hold the padded band of `mr` rows)
        if (e == hipSuccess) e = sc->tile.ensure((size_t)(use_rccl ? mr : rows[i]) * W);
        if (e == hipSuccess && rgb8) e = sc->qbytes.ensure((size_t)(use_rccl ? mr : rows[i]) * W * 3);
        if (e != hipSuccess) return bail(hip_code(e), std::string("rtmi_render_frame_multi: ") + hipGetErrorString(e));
        const rtmi_tile_t tile{i * S, rows[i], S, n * S};
        const clk::time_point t0 = clk::now();
        int rc = rtmi_render_tile_device(sc, vp, seed, &tile, sc->tile.p, sc->mstream, &st);
        if (rc != RTMI_OK) return bail(rc, g_err);
        st.render_ms = ms_since(t0);
        st.peer_access = peer;
        const void* band = sc->tile.p;
        const clk::time_point t1 = clk::now();
        if (rgb8) {
            hipLaunchKernelGGL(k_quantize, dim3((unsigned)(sc->num_cu * 8)), dim3(256), 0, sc->mstream, (uint64_t)rows[i] * W,
                               (const float4*)sc->tile.p, sc->qbytes.p);
            band = sc->qbytes.p;
        }
        if (use_rccl) {  // the bands cross together below, in ONE ncclGather; here only the quantisation is awaited
            e = hipStreamSynchronize(sc->mstream);
            if (e != hipSuccess) return bail(hip_code(e), std::string("rtmi_render_frame_multi: ") + hipGetErrorString(e));
            return;
        }
        // the single crossing of this band: its own link to the root (a plain device copy when both are one device)
        e = hipMemcpyPeerAsync(root->mstage.p + (size_t)i * mr * W * px, root->device, band, sc->device, (size_t)rows[i] * W * px, sc->mstream);
        if (e == hipSuccess) e = hipStreamSynchronize(sc->mstream);
        if (e != hipSuccess) return bail(hip_code(e), std::string("rtmi_render_frame_multi: band copy: ") + hipGetErrorString(e));
        st.band_copy_ms = ms_since(t1);
    };
    // no C++ exception leaves a worker thread (std::terminate) or crosses the ABI
    auto work = [&](uint32_t i) {
        memset(&sts[i], 0, sizeof(rtmi_stats_t));
        try { work_body(i); }
        catch (const std::bad_alloc&) { rcs[i] = RTMI_ERR_OOM; try { errs[i] = "host allocation failed"; } catch (...) {} }
        catch (...) { rcs[i] = RTMI_ERR_INVALID; try { errs[i] = "internal error"; } catch (...) {} }
    };
    if (n == 1) work(0);
    else {
        struct Joiner {  // joins what was started, also when starting a later thread throws
            std::vector<std::thread> th;
            ~Joiner() { for (auto& t : th) if (t.joinable()) t.join(); }
        } pool;
        pool.th.reserve(n);
        for (uint32_t i = 0; i < n; i++) pool.th.emplace_back(work, i);
    }
    std::string warn;
    for (uint32_t i = 0; i < n; i++) {
        if (rcs[i] != RTMI_OK) return fail(rcs[i], "scene " + std::to_string(i) + ": " + errs[i]);
        if (!scenes[i]->peer_ok && warn.empty())
            warn = "warning: device " + std::to_string(scenes[i]->device) + " has no peer access to root device " + std::to_string(root->device) +
                   " (" + scenes[i]->peer_msg + "): its band is staged by the runtime, see rtmi_stats_t.peer_access / band_copy_ms";
    }
    if (use_rccl) {
        // ---- ONE ncclGather over the scenes' devices (rccl.h ncclGather): every rank sends its padded band, the
        //      root receives them rank-major into the staging buffer the de-interleave kernel reads.  Communicators are
        //      made once per device list (ncclCommInitAll) and kept on the root handle.
        std::vector<int> devs(n);
        for (uint32_t i = 0; i < n; i++) devs[i] = scenes[i]->device;
        if (root->comm_devices != devs) {
            for (ncclComm_t c : root->comms) (void)rccl->CommDestroy(c);
            root->comms.assign(n, nullptr);
            root->comm_devices.clear();
            const ncclResult_t r = rccl->CommInitAll(root->comms.data(), (int)n, devs.data());
            if (r != ncclSuccess) { root->comms.clear(); return fail(RTMI_ERR_DEVICE, std::string("ncclCommInitAll: ") + rccl->GetErrorString(r)); }
            root->comm_devices = devs;
        }
        const clk::time_point t1 = clk::now();
        const size_t count = (size_t)mr * W * px;  // bytes per rank
        ncclResult_t r = rccl->GroupStart();
        for (uint32_t i = 0; i < n && r == ncclSuccess; i++) {
            rtmi_scene* sc = scenes[i];
            HIPCHK(hipSetDevice(sc->device));
            if (!sc->mstream) HIPCHK(hipStreamCreateWithFlags(&sc->mstream, hipStreamNonBlocking));
            if (rows[i] == 0) { HIPCHK(sc->tile.ensure((size_t)mr * W)); if (rgb8) HIPCHK(sc->qbytes.ensure((size_t)mr * W * 3)); }
            const void* band = rgb8 ? (const void*)sc->qbytes.p : (const void*)sc->tile.p;
            r = rccl->Gather(band, i == 0 ? (void*)root->mstage.p : nullptr, count, ncclUint8, 0, root->comms[i], sc->mstream);
        }
        const ncclResult_t r2 = rccl->GroupEnd();
        if (r == ncclSuccess) r = r2;
        if (r != ncclSuccess) return fail(RTMI_ERR_DEVICE, std::string("ncclGather: ") + rccl->GetErrorString(r));
        for (uint32_t i = 0; i < n; i++) {
            HIPCHK(hipSetDevice(scenes[i]->device));
            HIPCHK(hipStreamSynchronize(scenes[i]->mstream));
            sts[i].band_copy_ms = ms_since(t1);
        }
    }
    // ---- root: de-interleave the stripes into the frame
    HIPCHK(hipSetDevice(root->device));
    if (!root->mstream) HIPCHK(hipStreamCreateWithFlags(&root->mstream, hipStreamNonBlocking));
    const clk::time_point t2 = clk::now();
    hipLaunchKernelGGL(k_deinterleave, dim3((unsigned)(root->num_cu * 8)), dim3(256), 0, root->mstream, root->mstage.p, frame, W, H, S, n, mr, px);
    HIPCHK(hipGetLastError());
    if (out_host) HIPCHK(hipMemcpyAsync(out_host, frame, (size_t)H * W * px, hipMemcpyDeviceToHost, root->mstream));
    HIPCHK(hipStreamSynchronize(root->mstream));
    sts[0].deinterleave_ms = ms_since(t2);
    if (stats) memcpy(stats, sts.data(), sizeof(rtmi_stats_t) * n);
    g_err = warn;  // RTMI_OK with a non-empty rtmi_last_error(): the frame is right, a link is slow
    return RTMI_OK;
    RTMI_GUARD_END
}

int rtmi_trace(rtmi_scene_t* s, uint64_t n, const float* orig4, const float* dir4, uint32_t* tri, float* t,
               uint32_t* face, rtmi_stats_t* stats) {
    if (!s) return fail(RTMI_ERR_INVALID, "scene is NULL");
    if (stats) memset(stats, 0, sizeof(*stats));
    if (n == 0) return RTMI_OK;
    if (!orig4 || !dir4 || !tri || !t || !face) return fail(RTMI_ERR_INVALID, "NULL argument");
    if (n >= (1ull << 31)) return fail(RTMI_ERR_UNSUPPORTED, "more than 2^31 rays per call");
    RTMI_GUARD_BEGIN
    HIPCHK(hipSetDevice(s->device));
    Work& w = s->w[0];
    int rc = ensure_workspace(w, (size_t)n, 1);
    if (rc != RTMI_OK) return rc;
    hipStream_t st = s->istream[0];
    HIPCHK(hipMemcpyAsync(w.qo[0].p, orig4, n * 16, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(w.qd[0].p, dir4, n * 16, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(w.ctrl.p, 0, sizeof(DCtrl), st));
    hipLaunchKernelGGL(k_set_count, dim3(1), dim3(1), 0, st, w.ctrl.p, (uint32_t)n);
    HIPCHK(hipEventRecord(w.ev[0], st));
    s->active_streams = 1;
    launch_trace(s, w, st, w.qo[0].p, w.qd[0].p, 0, (s->options & RTMI_OPT_COUNTERS) != 0, w.ev[1]);
    HIPCHK(hipGetLastError());
    std::vector<uint32_t> tf(n);
    HIPCHK(hipMemcpyAsync(tf.data(), w.hit_tf.p, n * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(t, w.hit_t.p, n * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (uint64_t i = 0; i < n; i++) { tri[i] = tf[i] & 0x3FFFFFFFu; face[i] = tf[i] >> 30; }
    // face encoding of the ABI: 0 front 1 back 2 edge-front 3 edge-back (bit0 = back, bit1 = edge)
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, w.ev[0], w.ev[1]));
    DCtrl h;
    HIPCHK(hipMemcpyAsync(&h, w.ctrl.p, sizeof(DCtrl), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (stats) {
        add_counters(*stats, ctrl_counters(h));
        stats->kernel_ms = ms; stats->trace_ms = ms; stats->trace_launches = 1; stats->streams = 1;
    }
    return RTMI_OK;
    RTMI_GUARD_END
}

// ---------------------------------------------------------------- any-hit occlusion (rtmi_occluded*)
// Checks that come before any HIP call and before the scene is used (a CPU-only caller reaches them).  The buffers are
// compared as the byte ranges the call reads and writes (16 n, 16 n, 4 n in; n out).
static int check_occluded(const rtmi_scene_t* s, uint64_t n, const void* orig4, const void* dir4, const void* tmax, const void* occ,
                          rtmi_stats_t* stats, bool& empty) {
    if (stats) memset(stats, 0, sizeof(*stats));
    empty = false;
    if (!s) return fail(RTMI_ERR_INVALID, "occluded: NULL argument (scene)");
    if (n == 0) { empty = true; return RTMI_OK; }
    if (!orig4 || !dir4 || !occ) return fail(RTMI_ERR_INVALID, "occluded: NULL argument (orig4, dir4 and occluded are required)");
    const uint64_t m = std::min<uint64_t>(n, 1ull << 40);  // (a count that is refused below anyway: the sizes must not wrap)
    const uintptr_t o0 = (uintptr_t)occ, o1 = o0 + m;
    const struct { const void* p; uint64_t bytes; const char* name; } in[3] = {{orig4, m * 16, "orig4"}, {dir4, m * 16, "dir4"}, {tmax, m * 4, "tmax"}};
    for (const auto& b : in)
        if (b.p && o0 < (uintptr_t)b.p + b.bytes && (uintptr_t)b.p < o1)
            return fail(RTMI_ERR_INVALID, std::string("occluded: the output must not alias an input (") + b.name + ")");
    if (n >= (1ull << 31)) return fail(RTMI_ERR_UNSUPPORTED, "occluded: more than 2^31 rays per call");
    return RTMI_OK;
}

// The rays (device memory) -> one byte per ray, on stream st with ctrl->count[0] = n set there (launch_occluded does the
// scene dispatch).  w.ev[0] / w.ev[1] bracket the walk kernel, as in rtmi_trace.
static int enqueue_occluded(rtmi_scene* s, Work& w, hipStream_t st, uint64_t n, const float4* qo, const float4* qd, const float* tmax,
                            uint8_t* occ) {
    s->active_streams = 1;
    if (!occluded_anyhit(s)) {
        const int rc = ensure_workspace(w, (size_t)n, 1);
        if (rc != RTMI_OK) return rc;
    }
    HIPCHK(hipMemsetAsync(w.ctrl.p, 0, sizeof(DCtrl), st));
    hipLaunchKernelGGL(k_set_count, dim3(1), dim3(1), 0, st, w.ctrl.p, (uint32_t)n);
    HIPCHK(hipEventRecord(w.ev[0], st));
    launch_occluded(s, w, st, n, qo, qd, tmax, occ, 0, w.ev[1]);
    HIPCHK(hipGetLastError());
    return RTMI_OK;
}

// After the stream is drained: the control block's counters and the walk kernel's time
static int collect_occluded(Work& w, hipStream_t st, rtmi_stats_t* stats, float kernel_ms) {
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, w.ev[0], w.ev[1]));
    DCtrl h;
    HIPCHK(hipMemcpyAsync(&h, w.ctrl.p, sizeof(DCtrl), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (stats) {
        add_counters(*stats, ctrl_counters(h));
        stats->kernel_ms = kernel_ms < 0.f ? ms : kernel_ms; stats->trace_ms = ms; stats->trace_launches = 1; stats->streams = 1;
    }
    return RTMI_OK;
}

int rtmi_occluded_device(rtmi_scene_t* s, uint64_t n, const void* orig4_device, const void* dir4_device, const void* tmax_device,
                         void* occluded_device, void* hip_stream, rtmi_stats_t* stats) {
    bool empty;
    int rc = check_occluded(s, n, orig4_device, dir4_device, tmax_device, occluded_device, stats, empty);
    if (rc != RTMI_OK || empty) return rc;
    RTMI_GUARD_BEGIN
    (void)hipGetLastError();
    HIPCHK(hipSetDevice(s->device));
    Work& w = s->w[0];
    hipStream_t st = s->istream[0], ust = (hipStream_t)hip_stream;
    // the library's stream starts after whatever the caller queued on its stream, and that stream waits for it
    HIPCHK(hipEventRecord(s->fork_ev, ust));
    HIPCHK(hipStreamWaitEvent(st, s->fork_ev, 0));
    rc = enqueue_occluded(s, w, st, n, (const float4*)orig4_device, (const float4*)dir4_device, (const float*)tmax_device,
                          (uint8_t*)occluded_device);
    if (rc != RTMI_OK) return rc;
    HIPCHK(hipEventRecord(s->join_ev[0], st));
    HIPCHK(hipStreamWaitEvent(ust, s->join_ev[0], 0));
    HIPCHK(hipEventRecord(s->end_ev, ust));
    HIPCHK(hipEventSynchronize(s->end_ev));
    float kernel_ms = 0.f;
    HIPCHK(hipEventElapsedTime(&kernel_ms, s->fork_ev, s->end_ev));
    return collect_occluded(w, st, stats, kernel_ms);
    RTMI_GUARD_END
}

int rtmi_occluded(rtmi_scene_t* s, uint64_t n, const float* orig4, const float* dir4, const float* tmax, uint8_t* occluded,
                  rtmi_stats_t* stats) {
    bool empty;
    int rc = check_occluded(s, n, orig4, dir4, tmax, occluded, stats, empty);
    if (rc != RTMI_OK || empty) return rc;
    RTMI_GUARD_BEGIN
    (void)hipGetLastError();
    HIPCHK(hipSetDevice(s->device));
    Work& w = s->w[0];
    rc = ensure_workspace(w, (size_t)n, 1);
    if (rc != RTMI_OK) return rc;
    HIPCHK(s->occ_out.ensure(n));
    if (tmax) HIPCHK(s->occ_tmax.ensure(n));
    hipStream_t st = s->istream[0];
    HIPCHK(hipMemcpyAsync(w.qo[0].p, orig4, n * 16, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(w.qd[0].p, dir4, n * 16, hipMemcpyHostToDevice, st));
    if (tmax) HIPCHK(hipMemcpyAsync(s->occ_tmax.p, tmax, n * 4, hipMemcpyHostToDevice, st));
    rc = enqueue_occluded(s, w, st, n, w.qo[0].p, w.qd[0].p, tmax ? s->occ_tmax.p : nullptr, s->occ_out.p);
    if (rc != RTMI_OK) return rc;
    HIPCHK(hipMemcpyAsync(occluded, s->occ_out.p, n, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return collect_occluded(w, st, stats, -1.f);
    RTMI_GUARD_END
}

// ---------------------------------------------------------------- explicit rays (rtmi_render_rays*, rtmi_trace_device)
// Buffers of a call as the byte ranges it reads and writes; a null pointer takes no part.  Returns the first pair that overlaps.
struct ByteRange { const void* p; uint64_t bytes; const char* name; };
static bool ranges_overlap(const ByteRange* r, size_t n, size_t& a, size_t& b) {
    for (a = 0; a < n; a++)
        for (b = a + 1; b < n; b++)
            if (r[a].p && r[b].p && (uintptr_t)r[a].p < (uintptr_t)r[b].p + r[b].bytes && (uintptr_t)r[b].p < (uintptr_t)r[a].p + r[a].bytes)
                return true;
    return false;
}

// ---- box lights on explicit rays and in the bake (rtmi_render_rays_lit*, rtmi_bake_lit*; lit.hpp)
// The lit variants run rtmi_render_lit*'s passes on stream 0's shadow buffers (rtmi_scene::ShadowBuf): THE site that sizes them for
// a call whose batches hold B rays of depth maxdepth.  Every queue of the walk holds B * nlights entries, the direct stack B *
// maxdepth; the walk's event pairs: one per pass, and one more for the walk of a bake's element candidates.
static bool lit_rays_from_hits(const rtmi_scene* s) { return s->lit_from_hits && !s->root_is_leaf; }
static int ensure_lit_rays(rtmi_scene* s, size_t B, uint32_t maxdepth, const LitArgs& la) {
    rtmi_scene::ShadowBuf& b = s->shadow[0];
    const size_t nq = B * la.nlights;
    const bool from_hits = lit_rays_from_hits(s);
    HIPCHK(b.qo.ensure(nq)); HIPCHK(b.qd.ensure(nq)); HIPCHK(b.tmax.ensure(nq)); HIPCHK(b.lw.ensure(nq)); HIPCHK(b.occ.ensure(nq));
    HIPCHK(b.slot.ensure(nq)); HIPCHK(b.dstack.ensure(B * std::max(maxdepth, 1u)));
    HIPCHK(b.walk.ctrl.ensure(1));
    if (nq && (!occluded_anyhit(s) || from_hits)) { HIPCHK(b.walk.hit_tf.ensure(nq)); HIPCHK(b.walk.hit_t.ensure(nq)); }
    if (nq && from_hits) HIPCHK(b.walk.fb.ensure(b.walk.hit_tf.n));  // the hybrid pass's fallback list, as long as the hit records
    while (b.walk.pass_ev.size() < 2 * ((size_t)maxdepth + 1)) {
        hipEvent_t e;
        HIPCHK(hipEventCreate(&e));
        b.walk.pass_ev.push_back(e);
    }
    return RTMI_OK;
}
// Pass `pass` of a batch of nb explicit rays after its closest-hit launch, where launch_shade stands in the plain calls:
// enqueue_batch's lit arm with the RAYS kernels.  (qo, qd): the pass's queue; keys: the batch's RNG keys or null.
static int lit_rays_pass(rtmi_scene* s, Work& w, hipStream_t st, const DView& dv, uint64_t seed, uint32_t pix0, uint32_t nb, uint32_t pass,
                         const LitArgs& la, const float4* qo, const float4* qd, const uint32_t* keys, float4* scol) {
    rtmi_scene::ShadowBuf& sb = s->shadow[0];
    const int a = pass & 1, b = a ^ 1;
    const dim3 ew_grid((unsigned)(s->num_cu * 8)), ew_block(256);
    // sb.walk.ctrl->count[pass + 1] (zero since the batch's memset) is the compaction's counter and then the walk's ray count
    if (dv.maxdepth - pass - 1u != 0u && la.nlights != 0u) {
        if (lit_surfaces(s))
            hipLaunchKernelGGL(k_lit_rays_surf_explicit, ew_grid, ew_block, 0, st, s->d, dv, seed, pix0, nb, (int)pass, la, qo, qd, w.qpath[a].p,
                               w.hit_tf.p, w.hit_t.p, w.ctrl.p, sb.qo.p, sb.qd.p, sb.tmax.p, sb.lw.p, sb.slot.p, sb.walk.ctrl.p, keys, s->smoothtab,
                               s->textab, s->nmaptab);
        else
            hipLaunchKernelGGL(k_lit_rays_explicit, ew_grid, ew_block, 0, st, s->d, dv, seed, pix0, nb, (int)pass, la, qo, qd, w.qpath[a].p,
                               w.hit_tf.p, w.hit_t.p, w.ctrl.p, sb.qo.p, sb.qd.p, sb.tmax.p, sb.lw.p, sb.slot.p, sb.walk.ctrl.p, keys);
        HIPCHK(hipEventRecord(sb.walk.pass_ev[2 * pass], st));
        launch_occluded(s, sb.walk, st, (uint64_t)nb * la.nlights, sb.qo.p, sb.qd.p, sb.tmax.p, sb.occ.p, (int)pass + 1,
                        sb.walk.pass_ev[2 * pass + 1], lit_rays_from_hits(s));
        HIPCHK(hipGetLastError());
    } else {  // no candidates (the exhausted level, or no lights): no walk, an empty event pair
        HIPCHK(hipEventRecord(sb.walk.pass_ev[2 * pass], st));
        HIPCHK(hipEventRecord(sb.walk.pass_ev[2 * pass + 1], st));
    }
    if (lit_surfaces(s))
        hipLaunchKernelGGL(k_shade_lit_surf_explicit, ew_grid, ew_block, 0, st, s->d, dv, seed, pix0, nb, (int)pass, s->envtab, la.nlights, qo, qd,
                           w.qpath[a].p, w.hit_tf.p, w.hit_t.p, sb.slot.p, sb.occ.p, sb.lw.p, w.qo[b].p, w.qd[b].p, w.qpath[b].p, w.mstack.p,
                           sb.dstack.p, scol, w.ctrl.p, keys, s->smoothtab, s->textab, w.cstack.p, s->nmaptab);
    else
        hipLaunchKernelGGL(s->has_env ? k_shade_lit_explicit<true> : k_shade_lit_explicit<false>, ew_grid, ew_block, 0, st, s->d, dv, seed, pix0,
                           nb, (int)pass, s->envtab, la.nlights, qo, qd, w.qpath[a].p, w.hit_tf.p, w.hit_t.p, sb.slot.p, sb.occ.p, sb.lw.p,
                           w.qo[b].p, w.qd[b].p, w.qpath[b].p, w.mstack.p, sb.dstack.p, scol, w.ctrl.p, keys);
    HIPCHK(hipGetLastError());
    return RTMI_OK;
}
// After a batch's stream has finished it: the walks' control block (the live candidates in rays, the work counters) and their
// event pairs [first_pair, end_pair).
static int lit_rays_collect(rtmi_scene* s, hipStream_t st, uint32_t first_pair, uint32_t end_pair, rtmi_stats_t& sum, float& trace_ms,
                            uint32_t& launches) {
    Work& sw = s->shadow[0].walk;
    DCtrl hs;
    HIPCHK(hipMemcpyAsync(&hs, sw.ctrl.p, sizeof(DCtrl), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    add_counters(sum, ctrl_counters(hs));
    for (uint32_t k = first_pair; k < end_pair; k++) {
        float pm = 0.f;
        HIPCHK(hipEventElapsedTime(&pm, sw.pass_ev[2 * k], sw.pass_ev[2 * k + 1]));
        launches++;
        trace_ms += pm;
    }
    return RTMI_OK;
}

// Checks that come before any HIP call (a CPU-only caller reaches them); only the last one reads the scene.
static int check_rays(const rtmi_scene_t* s, uint64_t n, const void* orig4, const void* dir4, const void* keys, const rtmi_rays_t* rp,
                      const rtmi_rays_out_t* out, rtmi_stats_t* stats, bool& empty) {
    if (stats) memset(stats, 0, sizeof(*stats));
    empty = false;
    if (!s) return fail(RTMI_ERR_INVALID, "render_rays: NULL argument (scene)");
    if (!rp) return fail(RTMI_ERR_INVALID, "render_rays: NULL argument (rays)");
    if (!out) return fail(RTMI_ERR_INVALID, "render_rays: NULL argument (out)");
    if (rp->group == 0) return fail(RTMI_ERR_INVALID, "render_rays: group must be >= 1");
    if (rp->flags & ~(uint32_t)RTMI_RAYS_MAKE_RAY) return fail(RTMI_ERR_INVALID, "render_rays: unknown flag bits");
    if (n % rp->group != 0) return fail(RTMI_ERR_INVALID, "render_rays: n must be a multiple of group");
    if (n == 0) { empty = true; return RTMI_OK; }
    if (!orig4) return fail(RTMI_ERR_INVALID, "render_rays: NULL argument (orig4)");
    if (!dir4) return fail(RTMI_ERR_INVALID, "render_rays: NULL argument (dir4)");
    if (!out->color && !out->mean && !out->albedo && !out->normal && !out->ids)
        return fail(RTMI_ERR_INVALID, "render_rays: all five outputs are NULL");
    const uint64_t m = std::min<uint64_t>(n, 1ull << 40), g = m / rp->group;  // (a count that is refused below anyway: the sizes must not wrap)
    const ByteRange r[8] = {{orig4, m * 16, "orig4"}, {dir4, m * 16, "dir4"}, {keys, m * 8, "keys"}, {out->color, m * 16, "color"},
                            {out->mean, g * 16, "mean"}, {out->albedo, g * 16, "albedo"}, {out->normal, g * 16, "normal"}, {out->ids, g * 4, "ids"}};
    size_t a, b;
    if (ranges_overlap(r, 8, a, b))
        return fail(RTMI_ERR_INVALID, std::string("render_rays: buffers overlap (") + r[a].name + " and " + r[b].name + ")");
    if (!keys && (uint64_t)rp->pixel0 + n / rp->group - 1 >= (1ull << 32))
        return fail(RTMI_ERR_INVALID, "render_rays: pixel0 + n / group - 1 must stay below 2^32 (the RNG key is 32 bits)");
    if (n >= (1ull << 31)) return fail(RTMI_ERR_UNSUPPORTED, "render_rays: more than 2^31 rays per call");
    if (rp->maxdepth > RTMI_MAX_PASSES) return fail(RTMI_ERR_UNSUPPORTED, "render_rays: maxdepth above 32");
    if (rp->group > 65536u) return fail(RTMI_ERR_UNSUPPORTED, "render_rays: group above 65536");
    if ((out->albedo || out->normal || out->ids) && s->d.nspheres)
        return fail(RTMI_ERR_UNSUPPORTED, "render_rays: no guide buffers (albedo, normal, ids) for scenes with analytic spheres");
    return RTMI_OK;
}

// Both variants.  Batches of whole groups on the library's stream 0, each the per-pass pipeline with the rays themselves as
// queue 0: k_rays_begin, then per pass the scene's closest-hit launch and k_shade_rays (after pass 0: k_features for the
// guides), then k_accum for the means.  Device variant: the rays, keys and outputs are the caller's buffers, used in place
// (shade_hit writes the sample colours straight into `color` when it is asked for).  Host variant: a batch's rays are staged
// in the workspace queue, its keys and group outputs in the host variants' per-pixel buffers of the handle (alist[0], tile,
// acc, asq, acnt: no call keeps anything in them between calls), and copied out batch by batch.
static int render_rays(rtmi_scene_t* s, uint64_t n, const void* orig4, const void* dir4, const void* keys, uint64_t seed,
                       const rtmi_rays_t* rp, const rtmi_rays_out_t* out, void* hip_stream, rtmi_stats_t* stats, bool host,
                       const LitArgs* lit = nullptr) {
    bool empty;
    int rc = check_rays(s, n, orig4, dir4, keys, rp, out, stats, empty);
    if (rc != RTMI_OK || empty) return rc;
    RTMI_GUARD_BEGIN
    (void)hipGetLastError();
    HIPCHK(hipSetDevice(s->device));
    const uint32_t G = rp->group, maxdepth = rp->maxdepth;
    const bool guides = out->albedo || out->normal || out->ids;
    const bool shade = maxdepth != 0 && (out->color || out->mean);
    const bool make = (rp->flags & RTMI_RAYS_MAKE_RAY) != 0, counting = (s->options & RTMI_OPT_COUNTERS) != 0;
    Work& w = s->w[0];
    hipStream_t st = s->istream[0], ust = host ? st : (hipStream_t)hip_stream;
    // batches hold whole groups: batch_paths rounded down to a multiple of G, at least G
    const uint64_t B = std::min<uint64_t>(std::max<uint64_t>(s->tune.batch_paths / G * G, G), n), gB = B / G;
    if (shade || guides) {
        rc = ensure_workspace(w, (size_t)B, std::max(maxdepth, 1u));
        if (rc == RTMI_OK) rc = ensure_cstack(s, w);
        if (rc != RTMI_OK) return rc;
    }
    if (lit && shade) {  // rtmi_render_rays_lit*: the shadow queue, answers, slots and direct stack of a batch
        rc = ensure_lit_rays(s, (size_t)B, maxdepth, *lit);
        if (rc != RTMI_OK) return rc;
    }
    if (host) {
        if (keys && shade) HIPCHK(s->alist[0].ensure(2 * B));
        if (out->mean && shade) HIPCHK(s->tile.ensure(gB));
        if (out->albedo) HIPCHK(s->acc.ensure(gB));
        if (out->normal) HIPCHK(s->asq.ensure(gB));
        if (out->ids) HIPCHK(s->acnt.ensure(gB));
    }
    s->active_streams = 1;
    // the library's stream starts after whatever the caller queued on its stream, and that stream waits for it
    HIPCHK(hipEventRecord(s->fork_ev, ust));
    if (!host) HIPCHK(hipStreamWaitEvent(st, s->fork_ev, 0));
    if (maxdepth == 0) {  // project_ray returns black immediately (raytrace.rs:1261-1263)
        if (host) {
            if (out->color) memset(out->color, 0, n * 16);
            if (out->mean) memset(out->mean, 0, n / G * 16);
        } else {
            if (out->color) HIPCHK(hipMemsetAsync(out->color, 0, n * 16, st));
            if (out->mean) HIPCHK(hipMemsetAsync(out->mean, 0, n / G * 16, st));
        }
    }
    DView dv{};  // what shade_pass<Samp::RAYS> reads of it: the depth, and the group size with its divisor
    dv.maxdepth = maxdepth; dv.spp = G;
    view_set_divisors(dv);
    const dim3 ew_grid((unsigned)(s->num_cu * 8)), ew_block(256);
    const uint32_t npass = shade ? maxdepth : guides ? 1u : 0u;
    rtmi_stats_t sum{};
    float trace_ms = 0.f;
    uint32_t launches = 0;
    for (uint64_t base = 0; base < n && npass; base += B) {
        const uint32_t nb = (uint32_t)std::min<uint64_t>(B, n - base), ng = nb / G;
        const uint64_t gbase = base / G;
        const float4 *qo = (const float4*)orig4 + base, *qd = (const float4*)dir4 + base;
        const uint32_t* kq = keys && shade ? (const uint32_t*)keys + 2 * base : nullptr;
        float4 *mean = out->mean ? (float4*)out->mean + gbase : nullptr, *albedo = out->albedo ? (float4*)out->albedo + gbase : nullptr,
               *normal = out->normal ? (float4*)out->normal + gbase : nullptr;
        uint32_t* ids = out->ids ? (uint32_t*)out->ids + gbase : nullptr;
        float4* scol = out->color && shade ? (float4*)out->color + base : w.scol.p;
        if (host) {
            HIPCHK(hipMemcpyAsync(w.qo[0].p, qo, (size_t)nb * 16, hipMemcpyHostToDevice, st));
            HIPCHK(hipMemcpyAsync(w.qd[0].p, qd, (size_t)nb * 16, hipMemcpyHostToDevice, st));
            if (kq) HIPCHK(hipMemcpyAsync(s->alist[0].p, kq, (size_t)nb * 8, hipMemcpyHostToDevice, st));
            qo = w.qo[0].p; qd = w.qd[0].p; kq = kq ? s->alist[0].p : nullptr;
            scol = w.scol.p;
            mean = mean ? s->tile.p : nullptr; albedo = albedo ? s->acc.p : nullptr; normal = normal ? s->asq.p : nullptr;
            ids = ids ? s->acnt.p : nullptr;
        }
        HIPCHK(hipMemsetAsync(w.ctrl.p, 0, sizeof(DCtrl), st));
        if (lit && shade) HIPCHK(hipMemsetAsync(s->shadow[0].walk.ctrl.p, 0, sizeof(DCtrl), st));
        hipLaunchKernelGGL(k_rays_begin, ew_grid, ew_block, 0, st, nb, make ? qd : nullptr, w.qd[0].p, w.qpath[0].p, w.ctrl.p);
        HIPCHK(hipGetLastError());
        if (make) qd = w.qd[0].p;
        for (uint32_t pass = 0; pass < npass; pass++) {
            const int a = pass & 1;
            const float4 *pqo = pass ? w.qo[a].p : qo, *pqd = pass ? w.qd[a].p : qd;  // pass 0 traces the rays where they are
            HIPCHK(hipEventRecord(w.pass_ev[2 * pass], st));
            launch_trace(s, w, st, pqo, pqd, (int)pass, counting, w.pass_ev[2 * pass + 1]);
            HIPCHK(hipGetLastError());
            if (pass == 0 && guides)  // before pass 1 rewrites the hit records
                launch_features(s, ew_grid, ew_block, st, ng, G, w.hit_tf.p, w.hit_t.p, (float*)albedo, (float*)normal, ids, 0u, ng, 1u, 0u, pqo, pqd);
            if (shade && lit) {
                rc = lit_rays_pass(s, w, st, dv, seed, (uint32_t)(rp->pixel0 + gbase), nb, pass, *lit, pqo, pqd, kq, scol);
                if (rc != RTMI_OK) return rc;
            } else if (shade) {
                launch_shade(s, w, st, Samp::RAYS, dv, seed, (uint32_t)(rp->pixel0 + gbase), nb, pass, pqo, pqd, scol, SLOW_OFF, kq);
            }
            HIPCHK(hipGetLastError());
        }
        if (shade && mean)
            hipLaunchKernelGGL(k_accum, ew_grid, ew_block, 0, st, ng, G, scol, (float*)mean, 0u, ng, 1u, 0u, make_fastdiv(ng));
        HIPCHK(hipGetLastError());
        if (host) {
            if (out->color && shade) HIPCHK(hipMemcpyAsync((float4*)out->color + base, scol, (size_t)nb * 16, hipMemcpyDeviceToHost, st));
            if (mean && shade) HIPCHK(hipMemcpyAsync((float4*)out->mean + gbase, mean, (size_t)ng * 16, hipMemcpyDeviceToHost, st));
            if (albedo) HIPCHK(hipMemcpyAsync((float4*)out->albedo + gbase, albedo, (size_t)ng * 16, hipMemcpyDeviceToHost, st));
            if (normal) HIPCHK(hipMemcpyAsync((float4*)out->normal + gbase, normal, (size_t)ng * 16, hipMemcpyDeviceToHost, st));
            if (ids) HIPCHK(hipMemcpyAsync((uint32_t*)out->ids + gbase, ids, (size_t)ng * 4, hipMemcpyDeviceToHost, st));
        }
        // the batch's counters and the time of every pass's closest-hit launch; the next batch reuses the workspace
        DCtrl h;
        HIPCHK(hipMemcpyAsync(&h, w.ctrl.p, sizeof(DCtrl), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        add_counters(sum, ctrl_counters(h));
        for (uint32_t pass = 0; pass < npass; pass++) {
            float pm = 0.f;
            HIPCHK(hipEventElapsedTime(&pm, w.pass_ev[2 * pass], w.pass_ev[2 * pass + 1]));
            launches++;
            trace_ms += pm;
            if (s->verbose) fprintf(stderr, "[rtmi] rays batch@%llu pass %u: %u rays, trace %.3f ms\n", (unsigned long long)base, pass, h.count[pass], pm);
        }
        if (lit && shade) {  // the shadow rays' walks, one event pair per pass
            rc = lit_rays_collect(s, st, 0u, npass, sum, trace_ms, launches);
            if (rc != RTMI_OK) return rc;
        }
    }
    if (!host) {
        HIPCHK(hipEventRecord(s->join_ev[0], st));
        HIPCHK(hipStreamWaitEvent(ust, s->join_ev[0], 0));
    }
    HIPCHK(hipEventRecord(s->end_ev, ust));
    HIPCHK(hipEventSynchronize(s->end_ev));
    float kernel_ms = 0.f;
    HIPCHK(hipEventElapsedTime(&kernel_ms, s->fork_ev, s->end_ev));
    if (stats) {
        add_counters(*stats, sum);
        stats->kernel_ms = kernel_ms; stats->trace_ms = trace_ms; stats->trace_launches = launches; stats->streams = 1;
        stats->pipeline = 1u;
    }
    return RTMI_OK;
    RTMI_GUARD_END
}

int rtmi_render_rays_device(rtmi_scene_t* s, uint64_t n, const void* orig4_device, const void* dir4_device, const void* keys_device,
                            uint64_t seed, const rtmi_rays_t* rays, const rtmi_rays_out_t* out_device, void* hip_stream,
                            rtmi_stats_t* stats) {
    return render_rays(s, n, orig4_device, dir4_device, keys_device, seed, rays, out_device, hip_stream, stats, false);
}

int rtmi_render_rays(rtmi_scene_t* s, uint64_t n, const float* orig4, const float* dir4, const uint32_t* keys, uint64_t seed,
                     const rtmi_rays_t* rays, const rtmi_rays_out_t* out_host, rtmi_stats_t* stats) {
    return render_rays(s, n, orig4, dir4, keys, seed, rays, out_host, nullptr, stats, true);
}

// rtmi_render_rays_lit*: rtmi_render_rays*'s checks, then rtmi_render_lit*'s of its parameters, then its scene refusals; all before
// any HIP call.  (An empty call returns where rtmi_render_rays* returns.)
static int render_rays_lit(rtmi_scene_t* s, uint64_t n, const void* orig4, const void* dir4, const void* keys, uint64_t seed,
                           const rtmi_rays_t* rp, const rtmi_lit_t* lit, const rtmi_rays_out_t* out, void* hip_stream, rtmi_stats_t* stats,
                           bool host) {
    bool empty;
    int rc = check_rays(s, n, orig4, dir4, keys, rp, out, stats, empty);
    if (rc != RTMI_OK || empty) return rc;
    rc = check_lit_params(lit);
    if (rc != RTMI_OK) return rc;
    rc = refuse_scene_lit(s, lit->flags);
    if (rc != RTMI_OK) return rc;
    const LitArgs la = lit_args(*lit);
    return render_rays(s, n, orig4, dir4, keys, seed, rp, out, hip_stream, stats, host, &la);
}

int rtmi_render_rays_lit_device(rtmi_scene_t* s, uint64_t n, const void* orig4_device, const void* dir4_device, const void* keys_device,
                                uint64_t seed, const rtmi_rays_t* rays, const rtmi_lit_t* lit, const rtmi_rays_out_t* out_device,
                                void* hip_stream, rtmi_stats_t* stats) {
    return render_rays_lit(s, n, orig4_device, dir4_device, keys_device, seed, rays, lit, out_device, hip_stream, stats, false);
}

int rtmi_render_rays_lit(rtmi_scene_t* s, uint64_t n, const float* orig4, const float* dir4, const uint32_t* keys, uint64_t seed,
                         const rtmi_rays_t* rays, const rtmi_lit_t* lit, const rtmi_rays_out_t* out_host, rtmi_stats_t* stats) {
    return render_rays_lit(s, n, orig4, dir4, keys, seed, rays, lit, out_host, nullptr, stats, true);
}

// ---------------------------------------------------------------- light bake (rtmi_bake*, bake.hpp)
void rtmi_bake_defaults(rtmi_bake_t* p) {
    if (!p) return;
    p->mode = RTMI_BAKE_POINTS; p->rays = 64; p->maxdepth = 4; p->pixel0 = 0; p->flags = 0;
    p->bias = 0.001f;  // the reference's bounce offset (raytrace.rs:284-296), along the normal as rtmi_render_ao*'s
}

// Checks that come before any HIP call and before the scene is used (a CPU-only caller reaches them).
static int check_bake(const rtmi_scene_t* s, uint64_t M, const void* pos4, const void* nrm4, const rtmi_bake_t* bp, const rtmi_bake_out_t* out,
                      rtmi_stats_t* stats, bool& empty, bool lit_call = false, const void* direct = nullptr) {
    if (stats) memset(stats, 0, sizeof(*stats));
    empty = false;
    if (!s) return fail(RTMI_ERR_INVALID, "bake: NULL argument (scene)");
    if (!bp) return fail(RTMI_ERR_INVALID, "bake: NULL argument (rtmi_bake_t)");
    if (!out) return fail(RTMI_ERR_INVALID, "bake: NULL argument (out)");
    if (bp->mode != RTMI_BAKE_POINTS && bp->mode != RTMI_BAKE_TRIANGLES) return fail(RTMI_ERR_INVALID, "bake: unknown mode");
    if (bp->rays == 0) return fail(RTMI_ERR_INVALID, "bake: rays must be >= 1");
    if (bp->flags != 0) return fail(RTMI_ERR_INVALID, "bake: flags must be 0");
    if (!std::isfinite(bp->bias)) return fail(RTMI_ERR_INVALID, "bake: bias must be finite");
    if (M == 0) { empty = true; return RTMI_OK; }
    if (!pos4) return fail(RTMI_ERR_INVALID, "bake: NULL argument (pos4)");
    if (!nrm4) return fail(RTMI_ERR_INVALID, "bake: NULL argument (nrm4)");
    if (!out->light && !out->open && !out->orig && !out->dir && !direct)
        return fail(RTMI_ERR_INVALID, lit_call ? "bake: all five outputs are NULL" : "bake: all four outputs are NULL");
    // (counts that are refused below anyway: the sizes must not wrap)
    const uint64_t m = std::min<uint64_t>(M, 1ull << 40), n = m * std::min<uint32_t>(bp->rays, 65537u);
    const ByteRange r[7] = {{pos4, m * (bp->mode == RTMI_BAKE_TRIANGLES ? 48u : 16u), "pos4"}, {nrm4, m * 16, "nrm4"}, {out->light, m * 16, "light"},
                            {out->open, m * 4, "open"}, {out->orig, n * 16, "orig"}, {out->dir, n * 16, "dir"}, {direct, m * 16, "direct"}};
    size_t a, b;
    if (ranges_overlap(r, 7, a, b))
        return fail(RTMI_ERR_INVALID, std::string("bake: buffers overlap (") + r[a].name + " and " + r[b].name + ")");
    if ((uint64_t)bp->pixel0 + M - 1 >= (1ull << 32))
        return fail(RTMI_ERR_INVALID, "bake: pixel0 + M - 1 must stay below 2^32 (the RNG key is 32 bits)");
    if (bp->rays > 65536u) return fail(RTMI_ERR_UNSUPPORTED, "bake: rays above 65536");
    if (bp->maxdepth > RTMI_MAX_PASSES) return fail(RTMI_ERR_UNSUPPORTED, "bake: maxdepth above 32");
    if (M >= (1ull << 31) || M * bp->rays >= (1ull << 31)) return fail(RTMI_ERR_UNSUPPORTED, "bake: M * rays must stay below 2^31");
    return RTMI_OK;
}

// Both variants.  render_rays()'s batch loop with k_bake_rays where k_rays_begin stands: batches of whole elements on the
// library's stream 0, per batch k_bake_rays, then per pass the scene's closest-hit launch and k_shade_rays (after pass 0:
// k_bake_open), then k_accum for light.  Device variant: the elements and outputs are the caller's buffers, used in place; with
// orig / dir given the rays are written there and pass 0 traces them there.  Host variant: a batch's elements are staged in
// the host variants' per-pixel buffers of the handle (acc: pos4, asq: nrm4; tile: light, acnt: open; no call keeps anything in
// them between calls), its rays in the workspace queue, copied out before pass 2 reuses that queue.
static int bake(rtmi_scene_t* s, uint64_t M, const void* pos4, const void* nrm4, uint64_t seed, const rtmi_bake_t* bp,
                const rtmi_bake_out_t* out, void* hip_stream, rtmi_stats_t* stats, bool host, const LitArgs* lit = nullptr,
                void* direct_out = nullptr) {
    bool empty;
    int rc = check_bake(s, M, pos4, nrm4, bp, out, stats, empty, lit != nullptr, direct_out);
    if (rc != RTMI_OK || empty) return rc;
    RTMI_GUARD_BEGIN
    (void)hipGetLastError();
    HIPCHK(hipSetDevice(s->device));
    const uint32_t K = bp->rays, maxdepth = bp->maxdepth;
    const bool tri = bp->mode == RTMI_BAKE_TRIANGLES;
    const uint32_t pstride = tri ? 3u : 1u;  // float4 of pos4 per element
    const bool shade = maxdepth != 0 && out->light, want_rays = out->orig || out->dir;
    const bool traced = shade || out->open, counting = (s->options & RTMI_OPT_COUNTERS) != 0;
    // rtmi_bake_lit*: the elements' own candidates, their walk and fold (with no light, direct is zeros and nothing is launched)
    const bool want_direct = lit && direct_out, direct_walk = want_direct && lit->nlights != 0u;
    const uint64_t n = M * K;
    Work& w = s->w[0];
    hipStream_t st = s->istream[0], ust = host ? st : (hipStream_t)hip_stream;
    // batches hold whole elements: batch_paths rounded down to a multiple of K, at least K
    const uint64_t B = std::min<uint64_t>(std::max<uint64_t>(s->tune.batch_paths / K * K, K), n), mB = B / K;
    if (traced || want_rays || direct_walk) {
        rc = ensure_workspace(w, (size_t)B, std::max(maxdepth, 1u));
        if (rc == RTMI_OK) rc = ensure_cstack(s, w);
        if (rc != RTMI_OK) return rc;
    }
    if (lit && (shade || direct_walk)) {  // the shadow queue, answers, slots and direct stack of a batch
        rc = ensure_lit_rays(s, (size_t)B, maxdepth, *lit);
        if (rc != RTMI_OK) return rc;
    }
    if (host) {
        HIPCHK(s->acc.ensure(mB * pstride));
        HIPCHK(s->asq.ensure(mB));
        if (shade || direct_walk) HIPCHK(s->tile.ensure(mB));
        if (out->open) HIPCHK(s->acnt.ensure(mB));
    }
    s->active_streams = 1;
    // the library's stream starts after whatever the caller queued on its stream, and that stream waits for it
    HIPCHK(hipEventRecord(s->fork_ev, ust));
    if (!host) HIPCHK(hipStreamWaitEvent(st, s->fork_ev, 0));
    if (maxdepth == 0 && out->light) {  // project_ray returns black immediately (raytrace.rs:1261-1263)
        if (host) memset(out->light, 0, M * 16);
        else HIPCHK(hipMemsetAsync(out->light, 0, M * 16, st));
    }
    if (want_direct && !direct_walk) {  // no light: d_k = (0, 0, 0, 0) for every k
        if (host) memset(direct_out, 0, M * 16);
        else HIPCHK(hipMemsetAsync(direct_out, 0, M * 16, st));
    }
    DView dv{};  // what shade_pass<Samp::RAYS> reads of it: the depth, and the group size with its divisor
    dv.maxdepth = maxdepth; dv.spp = K;
    view_set_divisors(dv);
    const dim3 ew_grid((unsigned)(s->num_cu * 8)), ew_block(256);
    const uint32_t npass = shade ? maxdepth : traced ? 1u : 0u, epb = bake_step_elems(K);
    const FastDiv dK = make_fastdiv(K);
    const bool lit_walks = lit && (shade || direct_walk);
    rtmi_stats_t sum{};
    float trace_ms = 0.f;
    uint32_t launches = 0;
    for (uint64_t base = 0; base < n && (traced || want_rays || direct_walk); base += B) {
        const uint32_t nb = (uint32_t)std::min<uint64_t>(B, n - base), mb = nb / K;
        const uint64_t mbase = base / K;
        const float4 *pos = (const float4*)pos4 + mbase * pstride, *nrm = (const float4*)nrm4 + mbase;
        float4* light = shade ? (float4*)out->light + mbase : nullptr;
        float* open = out->open ? (float*)out->open + mbase : nullptr;
        float4 *qo = out->orig && !host ? (float4*)out->orig + base : w.qo[0].p, *qd = out->dir && !host ? (float4*)out->dir + base : w.qd[0].p;
        if (host) {
            HIPCHK(hipMemcpyAsync(s->acc.p, pos, (size_t)mb * pstride * 16, hipMemcpyHostToDevice, st));
            HIPCHK(hipMemcpyAsync(s->asq.p, nrm, (size_t)mb * 16, hipMemcpyHostToDevice, st));
            pos = s->acc.p; nrm = s->asq.p;
            light = light ? s->tile.p : nullptr;
            open = open ? (float*)s->acnt.p : nullptr;
        }
        HIPCHK(hipMemsetAsync(w.ctrl.p, 0, sizeof(DCtrl), st));
        const dim3 gen_grid(std::min<unsigned>((unsigned)(s->num_cu * 8), (mb + epb - 1u) / epb));
        if (lit_walks) HIPCHK(hipMemsetAsync(s->shadow[0].walk.ctrl.p, 0, sizeof(DCtrl), st));
        if (direct_walk) {
            // The elements' own candidates, before the gather paths use the shadow buffers and the sample colours: the live ones
            // into the shadow queue counted in the walk's count[RTMI_MAX_PASSES] (no path level's: those are 1 .. maxdepth - 1),
            // their walk, d_k into the workspace's sample colours, k_accum's fold into direct (host: staged in `tile`, which
            // light's fold rewrites after the copy).
            rtmi_scene::ShadowBuf& sb = s->shadow[0];
            float4* direct = host ? s->tile.p : (float4*)direct_out + mbase;
            if (tri)
                hipLaunchKernelGGL(k_bake_lit_rays<true>, gen_grid, ew_block, 0, st, mb, K, dK, epb, pos, nrm, seed, (uint32_t)(bp->pixel0 + mbase),
                                   *lit, sb.qo.p, sb.qd.p, sb.tmax.p, sb.lw.p, sb.slot.p, sb.walk.ctrl.p, (int)RTMI_MAX_PASSES);
            else
                hipLaunchKernelGGL(k_bake_lit_rays<false>, gen_grid, ew_block, 0, st, mb, K, dK, epb, pos, nrm, seed, (uint32_t)(bp->pixel0 + mbase),
                                   *lit, sb.qo.p, sb.qd.p, sb.tmax.p, sb.lw.p, sb.slot.p, sb.walk.ctrl.p, (int)RTMI_MAX_PASSES);
            HIPCHK(hipGetLastError());
            HIPCHK(hipEventRecord(sb.walk.pass_ev[2 * maxdepth], st));
            launch_occluded(s, sb.walk, st, (uint64_t)nb * lit->nlights, sb.qo.p, sb.qd.p, sb.tmax.p, sb.occ.p, (int)RTMI_MAX_PASSES,
                            sb.walk.pass_ev[2 * maxdepth + 1], lit_rays_from_hits(s));
            HIPCHK(hipGetLastError());
            hipLaunchKernelGGL(k_bake_lit_resolve, ew_grid, ew_block, 0, st, nb, lit->nlights, sb.slot.p, sb.occ.p, sb.lw.p, w.scol.p);
            hipLaunchKernelGGL(k_accum, ew_grid, ew_block, 0, st, mb, K, w.scol.p, (float*)direct, 0u, mb, 1u, 0u, make_fastdiv(mb));
            HIPCHK(hipGetLastError());
            if (host) HIPCHK(hipMemcpyAsync((float4*)direct_out + mbase, direct, (size_t)mb * 16, hipMemcpyDeviceToHost, st));
        }
        const bool gather = traced || want_rays;  // false with direct alone: no gather ray is made
        if (gather && tri)
            hipLaunchKernelGGL(k_bake_rays<true>, gen_grid, ew_block, 0, st, mb, K, dK, epb, pos, nrm, seed, (uint32_t)(bp->pixel0 + mbase), bp->bias,
                               qo, qd, w.qpath[0].p, w.ctrl.p);
        else if (gather)
            hipLaunchKernelGGL(k_bake_rays<false>, gen_grid, ew_block, 0, st, mb, K, dK, epb, pos, nrm, seed, (uint32_t)(bp->pixel0 + mbase), bp->bias,
                               qo, qd, w.qpath[0].p, w.ctrl.p);
        HIPCHK(hipGetLastError());
        if (host) {  // before pass 2 writes its queue over them
            if (out->orig) HIPCHK(hipMemcpyAsync((float4*)out->orig + base, qo, (size_t)nb * 16, hipMemcpyDeviceToHost, st));
            if (out->dir) HIPCHK(hipMemcpyAsync((float4*)out->dir + base, qd, (size_t)nb * 16, hipMemcpyDeviceToHost, st));
        }
        for (uint32_t pass = 0; pass < npass; pass++) {
            const int a = pass & 1;
            const float4 *pqo = pass ? w.qo[a].p : qo, *pqd = pass ? w.qd[a].p : qd;  // pass 0 traces the rays where they are
            HIPCHK(hipEventRecord(w.pass_ev[2 * pass], st));
            launch_trace(s, w, st, pqo, pqd, (int)pass, counting, w.pass_ev[2 * pass + 1]);
            HIPCHK(hipGetLastError());
            if (pass == 0 && open)  // before pass 1 rewrites the hit records
                hipLaunchKernelGGL(k_bake_open, dim3(std::min<unsigned>((unsigned)(s->num_cu * 8), (mb + RTMI_BAKE_OPEN_ELEMS - 1u) / RTMI_BAKE_OPEN_ELEMS)),
                                   ew_block, 0, st, mb, K, w.hit_tf.p, open);
            if (shade && lit) {
                rc = lit_rays_pass(s, w, st, dv, seed, (uint32_t)(bp->pixel0 + mbase), nb, pass, *lit, pqo, pqd, nullptr, w.scol.p);
                if (rc != RTMI_OK) return rc;
            } else if (shade) {
                launch_shade(s, w, st, Samp::RAYS, dv, seed, (uint32_t)(bp->pixel0 + mbase), nb, pass, pqo, pqd, w.scol.p, SLOW_OFF);
            }
            HIPCHK(hipGetLastError());
        }
        if (shade) hipLaunchKernelGGL(k_accum, ew_grid, ew_block, 0, st, mb, K, w.scol.p, (float*)light, 0u, mb, 1u, 0u, make_fastdiv(mb));
        HIPCHK(hipGetLastError());
        if (host) {
            if (shade) HIPCHK(hipMemcpyAsync((float4*)out->light + mbase, light, (size_t)mb * 16, hipMemcpyDeviceToHost, st));
            if (open) HIPCHK(hipMemcpyAsync((float*)out->open + mbase, open, (size_t)mb * 4, hipMemcpyDeviceToHost, st));
        }
        // the batch's counters and the time of every pass's closest-hit launch; the next batch reuses the workspace
        DCtrl h;
        HIPCHK(hipMemcpyAsync(&h, w.ctrl.p, sizeof(DCtrl), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (npass) add_counters(sum, ctrl_counters(h));
        for (uint32_t pass = 0; pass < npass; pass++) {
            float pm = 0.f;
            HIPCHK(hipEventElapsedTime(&pm, w.pass_ev[2 * pass], w.pass_ev[2 * pass + 1]));
            launches++;
            trace_ms += pm;
            if (s->verbose) fprintf(stderr, "[rtmi] bake batch@%llu pass %u: %u rays, trace %.3f ms\n", (unsigned long long)base, pass, h.count[pass], pm);
        }
        if (lit_walks) {  // the shadow rays' walks: one event pair per pass of the gather paths, the elements' own at [maxdepth]
            rc = lit_rays_collect(s, st, shade ? 0u : maxdepth, direct_walk ? maxdepth + 1u : maxdepth, sum, trace_ms, launches);
            if (rc != RTMI_OK) return rc;
        }
    }
    if (!host) {
        HIPCHK(hipEventRecord(s->join_ev[0], st));
        HIPCHK(hipStreamWaitEvent(ust, s->join_ev[0], 0));
    }
    HIPCHK(hipEventRecord(s->end_ev, ust));
    HIPCHK(hipEventSynchronize(s->end_ev));
    float kernel_ms = 0.f;
    HIPCHK(hipEventElapsedTime(&kernel_ms, s->fork_ev, s->end_ev));
    if (stats) {
        add_counters(*stats, sum);
        stats->kernel_ms = kernel_ms; stats->trace_ms = trace_ms; stats->trace_launches = launches; stats->streams = 1;
        stats->pipeline = 1u;
    }
    return RTMI_OK;
    RTMI_GUARD_END
}

int rtmi_bake_device(rtmi_scene_t* s, uint64_t M, const void* pos4_device, const void* nrm4_device, uint64_t seed, const rtmi_bake_t* bake_params,
                     const rtmi_bake_out_t* out_device, void* hip_stream, rtmi_stats_t* stats) {
    return bake(s, M, pos4_device, nrm4_device, seed, bake_params, out_device, hip_stream, stats, false);
}

int rtmi_bake(rtmi_scene_t* s, uint64_t M, const float* pos4, const float* nrm4, uint64_t seed, const rtmi_bake_t* bake_params,
              const rtmi_bake_out_t* out_host, rtmi_stats_t* stats) {
    return bake(s, M, pos4, nrm4, seed, bake_params, out_host, nullptr, stats, true);
}

// rtmi_bake_lit*: rtmi_bake*'s checks (direct among the outputs), then rtmi_render_lit*'s of its parameters, then its scene
// refusals; all before any HIP call.  (An empty call returns where rtmi_bake* returns.)
static_assert(offsetof(rtmi_bake_lit_out_t, direct) == sizeof(rtmi_bake_out_t) && offsetof(rtmi_bake_lit_out_t, dir) == offsetof(rtmi_bake_out_t, dir),
              "rtmi_bake_lit_out_t begins with rtmi_bake_out_t");
static int bake_lit(rtmi_scene_t* s, uint64_t M, const void* pos4, const void* nrm4, uint64_t seed, const rtmi_bake_t* bp, const rtmi_lit_t* lit,
                    const rtmi_bake_lit_out_t* out, void* hip_stream, rtmi_stats_t* stats, bool host) {
    rtmi_bake_out_t plain{};
    if (out) { plain.light = out->light; plain.open = out->open; plain.orig = out->orig; plain.dir = out->dir; }
    bool empty;
    int rc = check_bake(s, M, pos4, nrm4, bp, out ? &plain : nullptr, stats, empty, true, out ? out->direct : nullptr);
    if (rc != RTMI_OK || empty) return rc;
    rc = check_lit_params(lit);
    if (rc != RTMI_OK) return rc;
    rc = refuse_scene_lit(s, lit->flags);
    if (rc != RTMI_OK) return rc;
    const LitArgs la = lit_args(*lit);
    return bake(s, M, pos4, nrm4, seed, bp, &plain, hip_stream, stats, host, &la, out->direct);
}

int rtmi_bake_lit_device(rtmi_scene_t* s, uint64_t M, const void* pos4_device, const void* nrm4_device, uint64_t seed, const rtmi_bake_t* bake_params,
                         const rtmi_lit_t* lit, const rtmi_bake_lit_out_t* out_device, void* hip_stream, rtmi_stats_t* stats) {
    return bake_lit(s, M, pos4_device, nrm4_device, seed, bake_params, lit, out_device, hip_stream, stats, false);
}

int rtmi_bake_lit(rtmi_scene_t* s, uint64_t M, const float* pos4, const float* nrm4, uint64_t seed, const rtmi_bake_t* bake_params,
                  const rtmi_lit_t* lit, const rtmi_bake_lit_out_t* out_host, rtmi_stats_t* stats) {
    return bake_lit(s, M, pos4, nrm4, seed, bake_params, lit, out_host, nullptr, stats, true);
}

// rtmi_trace on device buffers: the rays are read where they are, one closest-hit launch, one elementwise kernel
int rtmi_trace_device(rtmi_scene_t* s, uint64_t n, const void* orig4_device, const void* dir4_device, void* tri_device, void* t_device,
                      void* face_device, void* hip_stream, rtmi_stats_t* stats) {
    if (stats) memset(stats, 0, sizeof(*stats));
    if (!s) return fail(RTMI_ERR_INVALID, "trace_device: NULL argument (scene)");
    if (n == 0) return RTMI_OK;
    if (!orig4_device || !dir4_device || !tri_device || !t_device || !face_device)
        return fail(RTMI_ERR_INVALID, "trace_device: NULL argument (orig4, dir4, tri, t and face are required)");
    const uint64_t m = std::min<uint64_t>(n, 1ull << 40);
    const ByteRange r[5] = {{orig4_device, m * 16, "orig4"}, {dir4_device, m * 16, "dir4"}, {tri_device, m * 4, "tri"}, {t_device, m * 4, "t"},
                            {face_device, m * 4, "face"}};
    size_t a, b;
    if (ranges_overlap(r, 5, a, b))
        return fail(RTMI_ERR_INVALID, std::string("trace_device: buffers overlap (") + r[a].name + " and " + r[b].name + ")");
    if (n >= (1ull << 31)) return fail(RTMI_ERR_UNSUPPORTED, "trace_device: more than 2^31 rays per call");
    RTMI_GUARD_BEGIN
    (void)hipGetLastError();
    HIPCHK(hipSetDevice(s->device));
    Work& w = s->w[0];
    int rc = ensure_workspace(w, (size_t)n, 1);
    if (rc != RTMI_OK) return rc;
    hipStream_t st = s->istream[0], ust = (hipStream_t)hip_stream;
    HIPCHK(hipEventRecord(s->fork_ev, ust));
    HIPCHK(hipStreamWaitEvent(st, s->fork_ev, 0));
    HIPCHK(hipMemsetAsync(w.ctrl.p, 0, sizeof(DCtrl), st));
    hipLaunchKernelGGL(k_set_count, dim3(1), dim3(1), 0, st, w.ctrl.p, (uint32_t)n);
    HIPCHK(hipEventRecord(w.ev[0], st));
    s->active_streams = 1;
    launch_trace(s, w, st, (const float4*)orig4_device, (const float4*)dir4_device, 0, (s->options & RTMI_OPT_COUNTERS) != 0, w.ev[1]);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_unpack_hits, dim3((unsigned)std::min<uint64_t>((n + 255) / 256, (uint64_t)s->num_cu * 8)), dim3(256), 0, st, (uint32_t)n,
                       w.hit_tf.p, w.hit_t.p, (uint32_t*)tri_device, (float*)t_device, (uint32_t*)face_device);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(s->join_ev[0], st));
    HIPCHK(hipStreamWaitEvent(ust, s->join_ev[0], 0));
    HIPCHK(hipEventRecord(s->end_ev, ust));
    HIPCHK(hipEventSynchronize(s->end_ev));
    float kernel_ms = 0.f;
    HIPCHK(hipEventElapsedTime(&kernel_ms, s->fork_ev, s->end_ev));
    return collect_occluded(w, st, stats, kernel_ms);
    RTMI_GUARD_END
}

// ---------------------------------------------------------------- per-ray records (k_trace_record, trace_oct.hpp W_RECORD)
// Scenes and modes whose rays k_trace_oct<COUNT, false> traces; RTMI_OK or RTMI_ERR_UNSUPPORTED with the reason.  Host only.
static int records_supported(const rtmi_scene* s) {
    if (s->root_is_leaf) return fail(RTMI_ERR_UNSUPPORTED, "records: the tree is a single leaf (k_trace_linear), not an octree walk");
    if (!s->octree) return fail(RTMI_ERR_UNSUPPORTED, "records: the tree is not an exact octree (" + s->why_generic + "), k_trace_oct does not run");
    if (s->options & RTMI_OPT_GENERIC) return fail(RTMI_ERR_UNSUPPORTED, "records: RTMI_OPT_GENERIC selects the generic kernel");
    if (s->options & RTMI_OPT_BVH) return fail(RTMI_ERR_UNSUPPORTED, "records: RTMI_OPT_BVH traces a BVH, not the octree");
    if (s->options & RTMI_OPT_FAST) return fail(RTMI_ERR_UNSUPPORTED, "records: RTMI_OPT_FAST is not the reference's walk");
    if (s->d.nspheres) return fail(RTMI_ERR_UNSUPPORTED, "records: the scene has analytic spheres (a flat list outside the tree)");
    return RTMI_OK;
}

// The rays are in w.qo[0] / w.qd[0] and ctrl->count[0] = n on stream st.  Launch 1 records the counters of every ray; the
// host scans the leaf counts into offsets; launch 2 (only when leaf_ids is given) walks the same rays again and writes
// their leaf ids.  The walk is deterministic: launch 2 must find the counts of launch 1 again (checked).
static int run_records(rtmi_scene* s, Work& w, hipStream_t st, uint64_t n, rtmi_ray_record_t* recs, uint32_t* leaf_ids,
                       uint64_t leaf_cap, uint64_t* leaf_total, rtmi_stats_t* stats) {
    HIPCHK(s->rec_cnt.ensure(5 * n));
    OctArgs a{};
    a.qo = w.qo[0].p; a.qd = w.qd[0].p; a.hit_tf = w.hit_tf.p; a.hit_t = w.hit_t.p; a.pass = 0;
    a.vote_s = s->vote[0]; a.vote_l = s->vote[1];
    const int refill = (int)s->tune.refill_min0, xcd = (int)(s->tune.xcd_aware % 3u);
    s->active_streams = 1;
    auto launch = [&](const RecArgs& ra) {
        hipLaunchKernelGGL(k_trace_record, oct_grid(s), dim3(64), oct_launch_lds(s, true), st, s->d, a, w.ctrl.p, refill, xcd, ra);
    };
    HIPCHK(hipEventRecord(w.ev[0], st));
    launch(RecArgs{s->rec_cnt.p, nullptr, nullptr, 0ull});
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(w.ev[1], st));
    std::vector<uint32_t> cnt(5 * n), tf(n);
    std::vector<float> ht(n);
    std::vector<float4> ro(n), rd(n);
    HIPCHK(hipMemcpyAsync(cnt.data(), s->rec_cnt.p, cnt.size() * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(tf.data(), w.hit_tf.p, n * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(ht.data(), w.hit_t.p, n * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(ro.data(), w.qo[0].p, n * 16, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(rd.data(), w.qd[0].p, n * 16, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, w.ev[0], w.ev[1]));
    std::vector<unsigned long long> first(n);
    uint64_t total = 0;
    for (uint64_t i = 0; i < n; i++) { first[i] = total; total += cnt[5 * i + 4]; }
    *leaf_total = total;
    if (leaf_ids && leaf_cap < total)
        return fail(RTMI_ERR_INVALID, "leaf_ids holds " + std::to_string(leaf_cap) + " ids, the call needs " + std::to_string(total));
    if (leaf_ids && total > 0) {
        HIPCHK(s->rec_first.ensure(n));
        HIPCHK(s->rec_ids.ensure(total));
        HIPCHK(hipMemcpyAsync(s->rec_first.p, first.data(), n * 8, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemsetAsync(w.ctrl.p, 0, sizeof(DCtrl), st));
        hipLaunchKernelGGL(k_set_count, dim3(1), dim3(1), 0, st, w.ctrl.p, (uint32_t)n);
        HIPCHK(hipEventRecord(w.ev[0], st));
        launch(RecArgs{s->rec_cnt.p, s->rec_first.p, s->rec_ids.p, (unsigned long long)total});
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(w.ev[1], st));
        std::vector<uint32_t> ids(total), cnt2(5 * n);
        HIPCHK(hipMemcpyAsync(ids.data(), s->rec_ids.p, total * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(cnt2.data(), s->rec_cnt.p, cnt2.size() * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        float ms2 = 0.f;
        HIPCHK(hipEventElapsedTime(&ms2, w.ev[0], w.ev[1]));
        ms += ms2;
        if (cnt2 != cnt) return fail(RTMI_ERR_DEVICE, "records: the leaf-id launch walked differently from the counting launch");
        for (uint64_t k = 0; k < total; k++) {  // (inner record << 3) | octant -> index in rtmi_scene_create's boxes
            const uint64_t j = ids[k];
            if (j >= s->leaf_box.size() || s->leaf_box[j] == 0xFFFFFFFFu)
                return fail(RTMI_ERR_DEVICE, "records: leaf id " + std::to_string(j) + " names no leaf of the tree");
            ids[k] = s->leaf_box[j];
        }
        memcpy(leaf_ids, ids.data(), total * 4);
    }
    if (stats) memset(stats, 0, sizeof(*stats));
    rtmi_stats_t sum{};
    for (uint64_t i = 0; i < n; i++) {
        rtmi_ray_record_t& r = recs[i];
        memcpy(r.orig, &ro[i], 16);
        memcpy(r.dir, &rd[i], 16);
        r.tri = tf[i] & 0x3FFFFFFFu;
        r.face = tf[i] >> 30;
        r.t = ht[i];
        const uint32_t* c = &cnt[5 * i];
        r.box_tests = c[0]; r.tri_tests = c[1]; r.full_tests = c[2]; r.nodes = c[3]; r.nleaves = c[4];
        r.leaf_first = first[i];
        sum.box_tests += c[0]; sum.tri_tests += c[1]; sum.full_tests += c[2]; sum.nodes += c[3]; sum.leaves += c[4];
    }
    if (stats) {
        *stats = sum;
        stats->rays = n;
        stats->kernel_ms = ms; stats->trace_ms = ms;
        stats->trace_launches = leaf_ids && total > 0 ? 2u : 1u;
        stats->streams = 1;
    }
    return RTMI_OK;
}

int rtmi_trace_records(rtmi_scene_t* s, uint64_t n, const float* orig4, const float* dir4, rtmi_ray_record_t* recs,
                       uint32_t* leaf_ids, uint64_t leaf_cap, uint64_t* leaf_total, rtmi_stats_t* stats) {
    if (stats) memset(stats, 0, sizeof(*stats));
    if (!s) return fail(RTMI_ERR_INVALID, "scene is NULL");
    if (!leaf_total) return fail(RTMI_ERR_INVALID, "leaf_total is NULL");
    *leaf_total = 0;
    if (n == 0) return RTMI_OK;
    if (!orig4 || !dir4) return fail(RTMI_ERR_INVALID, "NULL rays");
    if (!recs) return fail(RTMI_ERR_INVALID, "recs is NULL");
    if (n >= (1ull << 31)) return fail(RTMI_ERR_UNSUPPORTED, "more than 2^31 rays per call");
    int rc = records_supported(s);
    if (rc != RTMI_OK) return rc;
    RTMI_GUARD_BEGIN
    (void)hipGetLastError();
    HIPCHK(hipSetDevice(s->device));
    Work& w = s->w[0];
    rc = ensure_workspace(w, (size_t)n, 1);
    if (rc != RTMI_OK) return rc;
    hipStream_t st = s->istream[0];
    HIPCHK(hipMemcpyAsync(w.qo[0].p, orig4, n * 16, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(w.qd[0].p, dir4, n * 16, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(w.ctrl.p, 0, sizeof(DCtrl), st));
    hipLaunchKernelGGL(k_set_count, dim3(1), dim3(1), 0, st, w.ctrl.p, (uint32_t)n);
    HIPCHK(hipGetLastError());
    return run_records(s, w, st, n, recs, leaf_ids, leaf_cap, leaf_total, stats);
    RTMI_GUARD_END
}

int rtmi_primary_records(rtmi_scene_t* s, const rtmi_viewport_t* vp, uint64_t seed, uint32_t row0, uint32_t nrows,
                         uint32_t sample, rtmi_ray_record_t* recs, uint32_t* leaf_ids, uint64_t leaf_cap,
                         uint64_t* leaf_total, rtmi_stats_t* stats) {
    if (stats) memset(stats, 0, sizeof(*stats));
    if (!s || !vp) return fail(RTMI_ERR_INVALID, "NULL argument (scene or viewport)");
    if (!leaf_total) return fail(RTMI_ERR_INVALID, "leaf_total is NULL");
    *leaf_total = 0;
    if (vp->width == 0 || vp->height == 0) return fail(RTMI_ERR_INVALID, "empty viewport");
    if (vp->samples_per_pixel == 0) return fail(RTMI_ERR_INVALID, "samples_per_pixel must be >= 1");
    if (sample >= vp->samples_per_pixel) return fail(RTMI_ERR_INVALID, "sample must be < samples_per_pixel");
    if ((uint64_t)row0 + nrows > vp->height) return fail(RTMI_ERR_INVALID, "row range outside the viewport");
    if (nrows == 0) return RTMI_OK;
    if (!recs) return fail(RTMI_ERR_INVALID, "recs is NULL");
    if ((uint64_t)vp->width * vp->height >= (1ull << 32)) return fail(RTMI_ERR_UNSUPPORTED, "more than 2^32 pixels");
    const uint64_t n = (uint64_t)nrows * vp->width;
    if (n >= (1ull << 31)) return fail(RTMI_ERR_UNSUPPORTED, "more than 2^31 rays per call");
    if (sample & RTMI_KEY_JITTER) return fail(RTMI_ERR_UNSUPPORTED, "sample above 2^31");
    int rc = records_supported(s);
    if (rc != RTMI_OK) return rc;
    RTMI_GUARD_BEGIN
    (void)hipGetLastError();
    HIPCHK(hipSetDevice(s->device));
    Work& w = s->w[0];
    rc = ensure_workspace(w, (size_t)n, 1);
    if (rc != RTMI_OK) return rc;
    hipStream_t st = s->istream[0];
    // the rows as one tile of one stream, sample `sample` of the frame's spp: k_gen_samples makes the renderer's rays
    DView dv;
    dv.orig = mk(vp->orig[0], vp->orig[1], vp->orig[2]);
    dv.cam = mk(vp->cam[0], vp->cam[1], vp->cam[2]);
    dv.vu = mk(vp->vu[0], vp->vu[1], vp->vu[2]);
    dv.vv = mk(vp->vv[0], vp->vv[1], vp->vv[2]);
    dv.width = vp->width; dv.height = vp->height; dv.maxdepth = vp->maxdepth; dv.spp = 1;
    dv.row0 = row0; dv.stripe_rows = nrows; dv.stripe_step = 0;
    view_set_sampling(dv, sample, vp->samples_per_pixel);
    dv.sub_mul = 1; dv.sub_off = 0;
    view_set_divisors(dv);
    HIPCHK(hipMemsetAsync(w.ctrl.p, 0, sizeof(DCtrl), st));
    hipLaunchKernelGGL(k_gen_samples, dim3((unsigned)(s->num_cu * 8)), dim3(256), 0, st, dv, seed, 0u, (uint32_t)n, w.qo[0].p, w.qd[0].p,
                       w.qpath[0].p, w.ctrl.p);
    HIPCHK(hipGetLastError());
    return run_records(s, w, st, n, recs, leaf_ids, leaf_cap, leaf_total, stats);
    RTMI_GUARD_END
}

// Test hook (not in rtmi.h): n / d as the kernels compute it for launch-constant divisors (FastDiv, shade.hpp), evaluated on
// the host with the same inline functions; needs no device.
uint32_t rtmi_debug_fastdiv(uint32_t n, uint32_t d) { return fdiv(n, make_fastdiv(d)); }

// Test hook (not in rtmi.h): the exact-octree form rtmi_scene_create would upload for a tree (same arguments), built on
// the host; needs no device.  sizes4 <- (fnodes records of 16 B, reference blocks, wlinks words, FN_WIDE boxes); the arrays
// (fnodes: 4 x sizes4[0] words, oblocks: 4 x sizes4[1], wlinks: sizes4[2]) are filled when not NULL -- call once with
// NULL arrays for the sizes.  RTMI_ERR_UNSUPPORTED (and the reason in rtmi_last_error) when the tree is no exact octree.
int rtmi_debug_oct_form(const rtmi_box_t* boxes, uint64_t nboxes, const uint32_t* tri_refs, uint64_t nrefs, uint64_t ntris,
                        uint32_t* fnodes, uint32_t* oblocks, uint32_t* wlinks, uint64_t* sizes4) {
    if (!boxes || nboxes < 1 || !sizes4 || (nrefs > 0 && !tri_refs)) return fail(RTMI_ERR_INVALID, "NULL argument");
    if (nboxes >= (1ull << 32) || nrefs >= (1ull << 32)) return fail(RTMI_ERR_UNSUPPORTED, "tree too large for 32-bit indices");
    RTMI_GUARD_BEGIN
    std::vector<uint32_t> depth;
    uint32_t max_inner_depth = 0;
    const std::string bad = validate_tree(boxes, nboxes, tri_refs, nrefs, ntris, depth, max_inner_depth);
    if (!bad.empty()) return fail(RTMI_ERR_INVALID, bad);
    OctForm f;
    build_oct_form(boxes, nboxes, tri_refs, ntris, depth, f);
    if (f.fn.empty()) return fail(RTMI_ERR_UNSUPPORTED, f.why);
    sizes4[0] = f.fn.size(); sizes4[1] = f.ob.size(); sizes4[2] = f.wl.size(); sizes4[3] = f.nwide;
    if (fnodes) memcpy(fnodes, f.fn.data(), f.fn.size() * sizeof(uint4));
    if (oblocks) memcpy(oblocks, f.ob.data(), f.ob.size() * sizeof(uint4));
    if (wlinks && !f.wl.empty()) memcpy(wlinks, f.wl.data(), f.wl.size() * sizeof(uint32_t));
    return RTMI_OK;
    RTMI_GUARD_END
}

// Test hook (not in rtmi.h): the ABI status and message a HIP runtime failure `hip_error` is reported as.
int rtmi_debug_status_of(int hip_error) {
    HIPCHK((hipError_t)hip_error);
    return RTMI_OK;
}

// Development aid (not in rtmi.h): step statistics of the last counting render/trace, the first n <= RTMI_NDBG entries.
int rtmi_debug_counters_n(rtmi_scene_t* s, unsigned long long* out, int n) {
    if (!s || !out) return fail(RTMI_ERR_INVALID, "NULL argument");
    if (n < 0 || n > RTMI_NDBG) return fail(RTMI_ERR_INVALID, "counter count out of range");
    HIPCHK(hipSetDevice(s->device));
    memset(out, 0, n * sizeof(unsigned long long));
    for (int k = 0; k < RTMI_MAX_STREAMS; k++) {
        DCtrl h;
        HIPCHK(hipMemcpy(&h, s->w[k].ctrl.p, sizeof(DCtrl), hipMemcpyDeviceToHost));
        for (int j = 0; j < n; j++) out[j] += h.dbg[j];
    }
    return RTMI_OK;
}
int rtmi_debug_counters(rtmi_scene_t* s, unsigned long long* out16) { return rtmi_debug_counters_n(s, out16, 16); }

// Test hook (not in rtmi.h): the packet cull of k_path_primary evaluated on the host with the kernel's own functions
// (trace_oct.hpp).  rays: n >= 1 rays (o.xyzw, d.xyzw: 8 floats each), the first one is the reference; recs: m plane records
// (incenter.xyz, r2, norm.xyz, material: 8 floats each).  on <- 1 when culling is on for the packet; cull[j] <- 1 when
// the predicate rejects record j for the whole packet (0 for all when it is off).  Needs no device.
int rtmi_debug_packet_cull(const float* rays, uint32_t n, const float* recs, uint64_t m, int* on, uint8_t* cull) {
    if (!rays || n < 1 || !on || (m > 0 && (!recs || !cull))) return fail(RTMI_ERR_INVALID, "NULL argument");
    auto f4 = [](const float* v) { return make_float4(v[0], v[1], v[2], v[3]); };
    Packet p{};
    p.ox = rays[0]; p.oy = rays[1]; p.oz = rays[2];
    p.dx = rays[4]; p.dy = rays[5]; p.dz = rays[6];
    bool ok = true;
    uint32_t mo = 0u, md = 0u;  // maxima as bit patterns, like the kernel's reduction
    for (uint32_t i = 0; i < n; i++) {
        float so, sd;
        ok &= packet_spread(p, f4(rays + 8 * i), f4(rays + 8 * i + 4), so, sd);
        uint32_t bo, bd;
        memcpy(&bo, &so, 4); memcpy(&bd, &sd, 4);
        mo = std::max(mo, bo); md = std::max(md, bd);
    }
    float so, sd;
    memcpy(&so, &mo, 4); memcpy(&sd, &md, 4);
    *on = ok && packet_finish(p, so, sd) ? 1 : 0;
    for (uint64_t j = 0; j < m; j++) cull[j] = *on && packet_culls(p, f4(recs + 8 * j), f4(recs + 8 * j + 4)) ? 1 : 0;
    return RTMI_OK;
}

// Development aid (not in rtmi.h): the block cull of k_trace_oct on the host with the kernel's own functions (trace_oct.hpp).
// recs: m plane records (incenter.xyz, r2, norm.xyz, material: 8 floats each; record 0 is the sentinel); blocks: nb blocks of
// 4 indices into recs in the form of oblocks (0: padding; a 4th word of 0 or with bit 31 set ends a list); rays: n rays
// (o.xyzw, d.xyzw).  records (8 words per block, or NULL) <- the cull records; rayok[i] (or NULL) <- block_cull_ray of ray i;
// out[b n + i] (or NULL) <- bit 0: the half-line misses the box, bit 1: the sign certificate holds, bit 2: block b is
// culled for ray i.  Needs no device.
int rtmi_debug_block_cull(const float* recs, uint64_t m, const uint32_t* blocks, uint64_t nb, const float* rays, uint64_t n,
                          uint32_t* records, uint8_t* rayok, uint8_t* out) {
    if (!recs || m < 1 || (nb > 0 && !blocks) || (n > 0 && !rays)) return fail(RTMI_ERR_INVALID, "NULL argument");
    RTMI_GUARD_BEGIN
    std::vector<uint4> hoc, hb(nb);
    std::vector<float4> hp(2 * m);
    if (nb) memcpy(hb.data(), blocks, nb * sizeof(uint4));
    memcpy(hp.data(), recs, m * 8 * sizeof(float));
    build_block_cull(hb.data(), nb, hp.data(), m, hoc);
    if (records && nb) memcpy(records, hoc.data(), hoc.size() * sizeof(uint4));
    std::vector<uint8_t> ok(n);
    std::vector<float> inv(3 * n);
    for (uint64_t i = 0; i < n; i++) {
        const float* v = rays + 8 * i;
        ok[i] = block_cull_ray(make_float4(v[0], v[1], v[2], v[3]), make_float4(v[4], v[5], v[6], v[7])) ? 1 : 0;
        for (int k = 0; k < 3; k++) inv[3 * i + k] = 1.f / v[4 + k];  // make_rayk
        if (rayok) rayok[i] = ok[i];
    }
    if (out)
        for (uint64_t b = 0; b < nb; b++)
            for (uint64_t i = 0; i < n; i++) {
                const float* v = rays + 8 * i;
                const uint4 c0 = hoc[2 * b], c1 = hoc[2 * b + 1];
                const uint32_t parts = block_cull_parts(c0, c1, v[0], v[1], v[2], v[4], v[5], v[6], inv[3 * i], inv[3 * i + 1], inv[3 * i + 2]);
                const bool cut = ok[i] && block_culls(c0, c1, v[0], v[1], v[2], v[4], v[5], v[6], inv[3 * i], inv[3 * i + 1], inv[3 * i + 2]);
                out[b * n + i] = (uint8_t)(parts | (cut ? 4u : 0u));
            }
    return RTMI_OK;
    RTMI_GUARD_END
}

// Development aid (not in rtmi.h): what k_trace_oct culls by, on the host with the kernel's own functions -- the per-ray sign
// certificate and the packed box-only records.  recs, blocks, rays: as for rtmi_debug_block_cull; G: cells per face edge of
// the direction table.  Every output may be NULL: packed (4 words per block) <- the packed records; cert[i] <- ray i is
// certified; ncand[i] <- length of its cell's list (0 for a ray block_cull_ray refuses); cell[i] <- its cell; out[b n + i] <-
// bit 0: the half-line misses the packed box, bit 2: block b is culled for ray i; table (room for table_cap words) <- the
// direction table when it fits, *table_words <- its size in words.  Needs no device.
int rtmi_debug_ray_cull(const float* recs, uint64_t m, const uint32_t* blocks, uint64_t nb, const float* rays, uint64_t n, uint32_t G,
                        uint32_t* packed, uint8_t* cert, uint32_t* ncand, uint32_t* cell, uint8_t* out, uint32_t* table,
                        uint64_t table_cap, uint64_t* table_words) {
    if (!recs || m < 1 || (nb > 0 && !blocks) || (n > 0 && !rays) || G < 8 || G > 1024) return fail(RTMI_ERR_INVALID, "NULL argument or G out of range");
    RTMI_GUARD_BEGIN
    std::vector<uint4> hoc, hpk, hb(nb);
    std::vector<float4> hp(2 * m);
    if (nb) memcpy(hb.data(), blocks, nb * sizeof(uint4));
    memcpy(hp.data(), recs, m * 8 * sizeof(float));
    build_block_cull(hb.data(), nb, hp.data(), m, hoc);
    pack_block_cull(hoc, hpk);
    if (packed && nb) memcpy(packed, hpk.data(), nb * sizeof(uint4));
    std::vector<uint32_t> hcert;
    CertStats st{};
    if (!build_ray_cert(hp.data(), m, G, SIZE_MAX, hcert, st)) return fail(RTMI_ERR_UNSUPPORTED, "direction table too large");
    if (table_words) *table_words = hcert.size();
    if (table && hcert.size() <= table_cap) memcpy(table, hcert.data(), hcert.size() * 4);
    std::vector<uint8_t> ok(n);
    for (uint64_t i = 0; i < n; i++) {
        const float* v = rays + 8 * i;
        const float4 o = make_float4(v[0], v[1], v[2], v[3]), d = make_float4(v[4], v[5], v[6], v[7]);
        uint32_t nc = 0;
        ok[i] = ray_sign_certified(hcert.data(), o, d, &nc) ? 1 : 0;
        if (cert) cert[i] = ok[i];
        if (ncand) ncand[i] = nc;
        if (cell) cell[i] = block_cull_ray(o, d) ? ray_cert_cell(G, d) : 0xFFFFFFFFu;
    }
    if (out) {
        std::vector<float> inv(3 * n);
        for (uint64_t i = 0; i < n; i++)
            for (int k = 0; k < 3; k++) inv[3 * i + k] = 1.f / rays[8 * i + 4 + k];  // make_rayk
        for (uint64_t b = 0; b < nb; b++)
            for (uint64_t i = 0; i < n; i++) {
                const float* v = rays + 8 * i;
                const bool miss = packed_block_miss(hpk[b], v[0], v[1], v[2], inv[3 * i], inv[3 * i + 1], inv[3 * i + 2]);
                out[b * n + i] = (uint8_t)((miss ? 1u : 0u) | (miss && ok[i] ? 4u : 0u));
            }
    }
    return RTMI_OK;
    RTMI_GUARD_END
}

// Development aid (not in rtmi.h): the direction table of a scene's sign certificate: out[0..5] = cells per face edge, distinct
// normals, list entries, longest list, table bytes, build time in microseconds (all 0: the block cull is off)
int rtmi_debug_cert_stats(const rtmi_scene_t* s, unsigned long long* out) {
    if (!s || !out) return fail(RTMI_ERR_INVALID, "NULL argument");
    const CertStats& c = s->cert_stats;
    out[0] = c.g; out[1] = c.normals; out[2] = c.entries; out[3] = c.longest; out[4] = c.bytes; out[5] = (unsigned long long)(c.seconds * 1e6);
    return RTMI_OK;
}

// Development aid (not in rtmi.h): the sign certificate alone, with its band as an argument (kappa = 0: CERT_KAPPA_PRIMARY,
// the band of k_path_primary's node cull).  recs, rays, G: as for rtmi_debug_ray_cull; cert[i] <- ray i is certified;
// ncand[i] (or NULL) <- length of its cell's list.  Needs no device.
int rtmi_debug_ray_cert_kappa(const float* recs, uint64_t m, const float* rays, uint64_t n, uint32_t G, float kappa, uint8_t* cert,
                              uint32_t* ncand) {
    if (!recs || m < 1 || (n > 0 && (!rays || !cert)) || G < 8 || G > 1024) return fail(RTMI_ERR_INVALID, "NULL argument or G out of range");
    RTMI_GUARD_BEGIN
    if (kappa == 0.f) kappa = CERT_KAPPA_PRIMARY;
    std::vector<float4> hp(2 * m);
    memcpy(hp.data(), recs, m * 8 * sizeof(float));
    std::vector<uint32_t> hcert;
    CertStats st{};
    if (!build_ray_cert(hp.data(), m, G, SIZE_MAX, hcert, st)) return fail(RTMI_ERR_UNSUPPORTED, "direction table too large");
    for (uint64_t i = 0; i < n; i++) {
        const float* v = rays + 8 * i;
        uint32_t nc = 0;
        cert[i] = ray_sign_certified(hcert.data(), make_float4(v[0], v[1], v[2], v[3]), make_float4(v[4], v[5], v[6], v[7]), &nc, kappa) ? 1 : 0;
        if (ncand) ncand[i] = nc;
    }
    return RTMI_OK;
    RTMI_GUARD_END
}

// Development aid (not in rtmi.h): rtmi_debug_ray_cert_kappa with the list walked an entry at a time
// (ray_sign_certified_ref): the referee of the batched walk.  Same arguments, same outputs.  Needs no device.
int rtmi_debug_ray_cert_ref(const float* recs, uint64_t m, const float* rays, uint64_t n, uint32_t G, float kappa, uint8_t* cert,
                            uint32_t* ncand) {
    if (!recs || m < 1 || (n > 0 && (!rays || !cert)) || G < 8 || G > 1024) return fail(RTMI_ERR_INVALID, "NULL argument or G out of range");
    RTMI_GUARD_BEGIN
    if (kappa == 0.f) kappa = CERT_KAPPA_PRIMARY;
    std::vector<float4> hp(2 * m);
    memcpy(hp.data(), recs, m * 8 * sizeof(float));
    std::vector<uint32_t> hcert;
    CertStats st{};
    if (!build_ray_cert(hp.data(), m, G, SIZE_MAX, hcert, st)) return fail(RTMI_ERR_UNSUPPORTED, "direction table too large");
    for (uint64_t i = 0; i < n; i++) {
        const float* v = rays + 8 * i;
        uint32_t nc = 0;
        cert[i] = ray_sign_certified_ref(hcert.data(), make_float4(v[0], v[1], v[2], v[3]), make_float4(v[4], v[5], v[6], v[7]), &nc, kappa) ? 1 : 0;
        if (ncand) ncand[i] = nc;
    }
    return RTMI_OK;
    RTMI_GUARD_END
}

// Development aid (not in rtmi.h): a scene's node cull records: out[0..2] = records, bytes, build time in microseconds (all 0:
// the node cull is off)
int rtmi_debug_node_cull_stats(const rtmi_scene_t* s, unsigned long long* out) {
    if (!s || !out) return fail(RTMI_ERR_INVALID, "NULL argument");
    out[0] = s->d.fcull ? s->node_cull_records : 0ull;
    out[1] = out[0] * 16ull;
    out[2] = s->d.fcull ? (unsigned long long)(s->node_cull_seconds * 1e6) : 0ull;
    return RTMI_OK;
}

// Development aid (not in rtmi.h): the node cull of k_trace_oct on the host with the kernel's own functions (trace_oct.hpp).
// boxes, tri_refs, ntris: a flattened tree as for rtmi_debug_oct_form; recs: ntris plane records (8 floats each, record 0
// the sentinel); rays: n rays (o.xyzw, d.xyzw); G: cells per face edge of the direction table.  *nrec <- inner records of the
// octree form (call with every array NULL for it).  Every array may be NULL: records (4 words per inner record, the index
// of `fnodes`) <- the packed node records; cert[i] <- ray i is certified; out[r n + i] <- bit 0: the half-line of ray i misses
// the packed box of record r, bit 2: the walk culls the subtree of r for ray i (bit 0 and certified).  Needs no device.
int rtmi_debug_node_cull_kappa(const rtmi_box_t* boxes, uint64_t nboxes, const uint32_t* tri_refs, uint64_t nrefs, uint64_t ntris,
                               const float* recs, const float* rays, uint64_t n, uint32_t G, uint64_t* nrec, uint32_t* records, uint8_t* cert,
                               uint8_t* out, float kappa);
int rtmi_debug_node_cull(const rtmi_box_t* boxes, uint64_t nboxes, const uint32_t* tri_refs, uint64_t nrefs, uint64_t ntris, const float* recs,
                         const float* rays, uint64_t n, uint32_t G, uint64_t* nrec, uint32_t* records, uint8_t* cert, uint8_t* out) {
    return rtmi_debug_node_cull_kappa(boxes, nboxes, tri_refs, nrefs, ntris, recs, rays, n, G, nrec, records, cert, out, CERT_KAPPA);
}
// ... and its twin with the certificate's band as an argument: kappa = 0 stands for CERT_KAPPA_PRIMARY, the band of
// k_path_primary's node cull (trace_oct.hpp)
int rtmi_debug_node_cull_kappa(const rtmi_box_t* boxes, uint64_t nboxes, const uint32_t* tri_refs, uint64_t nrefs, uint64_t ntris,
                               const float* recs, const float* rays, uint64_t n, uint32_t G, uint64_t* nrec, uint32_t* records, uint8_t* cert,
                               uint8_t* out, float kappa) {
    if (kappa == 0.f) kappa = CERT_KAPPA_PRIMARY;
    if (!boxes || nboxes < 1 || !recs || ntris < 1 || !nrec || (nrefs > 0 && !tri_refs) || (n > 0 && !rays) || G < 8 || G > 1024)
        return fail(RTMI_ERR_INVALID, "NULL argument or G out of range");
    if (nboxes >= (1ull << 32) || nrefs >= (1ull << 32)) return fail(RTMI_ERR_UNSUPPORTED, "tree too large for 32-bit indices");
    RTMI_GUARD_BEGIN
    std::vector<uint32_t> depth;
    uint32_t max_inner_depth = 0;
    const std::string bad = validate_tree(boxes, nboxes, tri_refs, nrefs, ntris, depth, max_inner_depth);
    if (!bad.empty()) return fail(RTMI_ERR_INVALID, bad);
    OctForm f;
    build_oct_form(boxes, nboxes, tri_refs, ntris, depth, f);
    if (f.fn.empty()) return fail(RTMI_ERR_UNSUPPORTED, f.why);
    *nrec = f.fn.size() / 2;
    if (!records && !cert && !out) return RTMI_OK;
    std::vector<float4> hp(2 * ntris);
    memcpy(hp.data(), recs, ntris * 8 * sizeof(float));
    std::vector<uint4> hoc, hnc, hnk;
    build_block_cull(f.ob.data(), f.ob.size(), hp.data(), ntris, hoc);
    build_node_cull(f.fn, f.wl, hoc, f.ob.size(), hnc);
    pack_block_cull(hnc, hnk);
    if (records && !hnk.empty()) memcpy(records, hnk.data(), hnk.size() * sizeof(uint4));
    std::vector<uint8_t> ok(n, 0);
    if (cert || out) {
        std::vector<uint32_t> hcert;
        CertStats st{};
        if (!build_ray_cert(hp.data(), ntris, G, SIZE_MAX, hcert, st)) return fail(RTMI_ERR_UNSUPPORTED, "direction table too large");
        for (uint64_t i = 0; i < n; i++) {
            const float* v = rays + 8 * i;
            ok[i] = ray_sign_certified(hcert.data(), make_float4(v[0], v[1], v[2], v[3]), make_float4(v[4], v[5], v[6], v[7]), nullptr, kappa) ? 1 : 0;
            if (cert) cert[i] = ok[i];
        }
    }
    if (out) {
        std::vector<float> inv(3 * n);
        for (uint64_t i = 0; i < n; i++)
            for (int k = 0; k < 3; k++) inv[3 * i + k] = 1.f / rays[8 * i + 4 + k];  // make_rayk
        for (uint64_t r = 0; r < hnk.size(); r++)
            for (uint64_t i = 0; i < n; i++) {
                const float* v = rays + 8 * i;
                const bool miss = packed_block_miss(hnk[r], v[0], v[1], v[2], inv[3 * i], inv[3 * i + 1], inv[3 * i + 2]);
                out[r * n + i] = (uint8_t)((miss ? 1u : 0u) | (miss && ok[i] ? 4u : 0u));
            }
    }
    return RTMI_OK;
    RTMI_GUARD_END
}

// Test hooks of the hybrid passes (not in rtmi.h; hybrid.hpp, bvh_fast.hpp).  None needs a device.
// rtmi_debug_hybrid_verify: the tree, plane records and rays as rtmi_debug_node_cull takes them, plus per ray a proposed hit
// (t, tri).  cert[i] <- ray i holds the certificate in the band k_hybrid_bvh uses and its origin is within the bound
// (*omax_out <- the scene's bound, may be NULL); out[i] <- what the guided descent and the
// list scan of k_oct_verify answer for the proposal (HV_OK = 0: confirmed; 1 absent child, 2 no collision, 3 tmin >= t, 4 the
// leaf's list lacks the triangle, 5 out of bounds), evaluated with the kernel's own function on the octree form
// rtmi_scene_create would upload.  A ray is accepted when cert[i] != 0 and out[i] == 0.
int rtmi_debug_hybrid_verify(const rtmi_box_t* boxes, uint64_t nboxes, const uint32_t* tri_refs, uint64_t nrefs, uint64_t ntris,
                             const float* recs, const float* rays, uint64_t n, uint32_t G, const float* t, const uint32_t* tri,
                             uint8_t* cert, uint8_t* out, float* omax_out) {
    if (!boxes || nboxes < 1 || !recs || ntris < 1 || (nrefs > 0 && !tri_refs) || (n > 0 && (!rays || !t || !tri || !cert || !out)) || G < 8 ||
        G > 1024)
        return fail(RTMI_ERR_INVALID, "NULL argument or G out of range");
    if (nboxes >= (1ull << 32) || nrefs >= (1ull << 32)) return fail(RTMI_ERR_UNSUPPORTED, "tree too large for 32-bit indices");
    RTMI_GUARD_BEGIN
    std::vector<uint32_t> depth;
    uint32_t max_inner_depth = 0;
    const std::string bad = validate_tree(boxes, nboxes, tri_refs, nrefs, ntris, depth, max_inner_depth);
    if (!bad.empty()) return fail(RTMI_ERR_INVALID, bad);
    OctForm f;
    build_oct_form(boxes, nboxes, tri_refs, ntris, depth, f);
    if (f.fn.empty()) return fail(RTMI_ERR_UNSUPPORTED, f.why);
    std::vector<float4> hp(2 * ntris);
    memcpy(hp.data(), recs, ntris * 8 * sizeof(float));
    std::vector<uint32_t> hcert;
    CertStats st{};
    if (!build_ray_cert(hp.data(), ntris, G, SIZE_MAX, hcert, st)) return fail(RTMI_ERR_UNSUPPORTED, "direction table too large");
    if (f.wl.empty()) f.wl.push_back(0u);
    float m = FLT_MAX;
    for (uint64_t k = 1; k < ntris; k++)
        m = std::min(m, ((std::fabs(recs[8 * k]) + std::fabs(recs[8 * k + 1])) + std::fabs(recs[8 * k + 2])) + std::sqrt(recs[8 * k + 3]));
    const float omax = hybrid_origin_max(m);
    if (omax_out) *omax_out = omax;
    for (uint64_t i = 0; i < n; i++) {
        const float* v = rays + 8 * i;
        const float4 o = make_float4(v[0], v[1], v[2], v[3]), d = make_float4(v[4], v[5], v[6], v[7]);
        cert[i] = (hybrid_origin_ok(o, omax) && ray_sign_certified(hcert.data(), o, d, nullptr, HYB_KAPPA)) ? 1 : 0;
        out[i] = (tri[i] == 0u || tri[i] >= ntris) ? (uint8_t)HV_BOUNDS
                                                   : (uint8_t)hybrid_verify(f.fn.data(), f.ob.data(), f.wl.data(), (uint32_t)(f.fn.size() / 2),
                                                                            (uint32_t)f.ob.size(), max_inner_depth + 1, boxes[0].len2, o, d, t[i], tri[i]);
    }
    return RTMI_OK;
    RTMI_GUARD_END
}
// rtmi_debug_hybrid_slab: n child boxes as (parent centre xyz, the children's half edge hc, octant) and n rays (o.xyz,
// d.xyz): tmin[i], hit[i] <- hybrid_child_slab with 1 / d as make_rayk forms it.
int rtmi_debug_hybrid_slab(const float* parent4, const uint32_t* oct, const float* rays6, uint64_t n, float* tmin, uint8_t* hit) {
    if (n > 0 && (!parent4 || !oct || !rays6 || !tmin || !hit)) return fail(RTMI_ERR_INVALID, "NULL argument");
    for (uint64_t i = 0; i < n; i++) {
        const float* p = parent4 + 4 * i;
        const float* r = rays6 + 6 * i;
        hit[i] = hybrid_child_slab(p[0], p[1], p[2], p[3], oct[i] & 7u, r[0], r[1], r[2], 1.f / r[3], 1.f / r[4], 1.f / r[5], tmin[i]) ? 1 : 0;
    }
    return RTMI_OK;
}
// rtmi_debug_hybrid_tie: a sequence of n passing triangles (t, tri) as a lane of k_hybrid_bvh meets them: flag <- the tie
// flag at the end (hybrid_tie_flag and the kernel's take rule), best_tri / best_t <- the lane's best.
int rtmi_debug_hybrid_tie(const float* t, const uint32_t* tri, uint64_t n, uint8_t* flag, uint32_t* best_tri, float* best_t) {
    if ((n > 0 && (!t || !tri)) || !flag || !best_tri || !best_t) return fail(RTMI_ERR_INVALID, "NULL argument");
    bool tie = false;
    float bt = INFINITY;
    uint32_t btri = 0u;
    for (uint64_t i = 0; i < n; i++) {
        tie = hybrid_tie_flag(tie, t[i], tri[i], bt, btri);
        const bool take = (t[i] < bt) | ((t[i] == bt) & (tri[i] < btri));  // bvh_walk's `take` for a finite time
        bt = take ? t[i] : bt;
        btri = take ? tri[i] : btri;
    }
    *flag = tie ? 1 : 0; *best_tri = btri; *best_t = bt;
    return RTMI_OK;
}
// rtmi_debug_record_boxes: n triangle records (the first 20 floats of rtmi_triangle_t each: incenter, norm, bounding_r2, sides,
// side_lens, edge_thickness).  corners9[i] <- the corners solved from record i's edge tests (absolute; zeros when the record
// is degenerate), box6[i] <- the BVH's clip box (lo.xyz, hi.xyz), derived[i] <- 1 when the corners entered it, 0 when it is
// the disc box, 2 when the record is not finite (no BVH).
int rtmi_debug_record_boxes(const float* recs20, uint64_t n, float* corners9, float* box6, uint8_t* derived) {
    if (n > 0 && (!recs20 || !corners9 || !box6 || !derived)) return fail(RTMI_ERR_INVALID, "NULL argument");
    for (uint64_t i = 0; i < n; i++) {
        rtmi_triangle_t t{};
        memcpy(&t, recs20 + 20 * i, 20 * sizeof(float));
        BBox b;
        b.reset();
        bool der = false;
        double c[3][3] = {};
        const bool ok = bvh_clip_box(t, b, der, c);
        for (int v = 0; v < 3; v++)
            for (int k = 0; k < 3; k++) corners9[9 * i + 3 * v + k] = der ? (float)((double)t.incenter[k] + c[v][k]) : 0.f;
        for (int k = 0; k < 3; k++) { box6[6 * i + k] = b.lo[k]; box6[6 * i + 3 + k] = b.hi[k]; }
        derived[i] = !ok ? 2 : (der ? 1 : 0);
    }
    return RTMI_OK;
}
// rtmi_debug_hybrid_counters: DCtrl::hyb of the scene's last render or trace call, summed over its streams (hybrid.hpp: what
// each of the RTMI_NHYB = 12 entries counts).  on <- 1 when the SCENE qualifies for hybrid passes; a launch on a workspace without a
// fallback list as long as its hit records (the shadow walks' own workspace in rtmi_render_shadowed*, which walks any-hit) still
// takes the one k_trace_oct launch.  The shadow workspaces of the lit, envlight and emissive calls have the list and take the
// hybrid pass: the function below reads their statistics.
int rtmi_debug_hybrid_counters(rtmi_scene_t* s, unsigned long long* out12, int* on) {
    if (!s || !out12) return fail(RTMI_ERR_INVALID, "NULL argument");
    HIPCHK(hipSetDevice(s->device));
    memset(out12, 0, RTMI_NHYB * sizeof(unsigned long long));
    for (int k = 0; k < RTMI_MAX_STREAMS; k++) {
        DCtrl h;
        HIPCHK(hipMemcpy(&h, s->w[k].ctrl.p, sizeof(DCtrl), hipMemcpyDeviceToHost));
        for (int j = 0; j < RTMI_NHYB; j++) out12[j] += h.hyb[j];
    }
    if (on) *on = (s->hybrid && s->octree && s->d.cert && s->bvh_ok && !s->root_is_leaf &&
                   !(s->options & (RTMI_OPT_GENERIC | RTMI_OPT_FAST | RTMI_OPT_BVH))) ? 1 : 0;
    return RTMI_OK;
}
// rtmi_debug_shadow_hybrid_counters: the same twelve entries of the shadow walks' own control blocks (shadow[k].walk.ctrl: the last
// batch of every stream of the scene's last rtmi_render_shadowed* / _lit* / _envlight* / _emissive* call), summed over the streams
// whose block is allocated; zeros where none is (no such call yet).  As in the function above, a stream the last call did not
// use keeps the block of the call that last used it: read it on a scene whose calls all ran on the same streams.
int rtmi_debug_shadow_hybrid_counters(rtmi_scene_t* s, unsigned long long* out12) {
    if (!s || !out12) return fail(RTMI_ERR_INVALID, "NULL argument");
    HIPCHK(hipSetDevice(s->device));
    memset(out12, 0, RTMI_NHYB * sizeof(unsigned long long));
    for (int k = 0; k < RTMI_MAX_STREAMS; k++) {
        if (!s->shadow[k].walk.ctrl.p) continue;
        DCtrl h;
        HIPCHK(hipMemcpy(&h, s->shadow[k].walk.ctrl.p, sizeof(DCtrl), hipMemcpyDeviceToHost));
        for (int j = 0; j < RTMI_NHYB; j++) out12[j] += h.hyb[j];
    }
    return RTMI_OK;
}

int rtmi_make_triangles(int device, const float* corners9_host, uint64_t n, const rtmi_triangle_t* proto, rtmi_triangle_t* out_host) {
    if (n == 0) return RTMI_OK;
    if (!corners9_host || !proto || !out_host) return fail(RTMI_ERR_INVALID, "NULL argument");
    if (n >= (1ull << 30)) return fail(RTMI_ERR_UNSUPPORTED, "more than 2^30 triangles");
    const int ndev = rtmi_device_count();
    if (ndev <= 0) return fail(RTMI_ERR_NO_DEVICE, "no HIP device visible: the MI355X kernels cannot run (there is no CPU fallback)");
    if (device < 0 || device >= ndev) return fail(RTMI_ERR_INVALID, "device index out of range");
    RTMI_GUARD_BEGIN
    HIPCHK(hipSetDevice(device));
    DevBuf<float> dpts, dout;
    DevBuf<uint32_t> dok;
    auto cleanup = [&]() { dpts.release(); dout.release(); dok.release(); };
    hipError_t e = dpts.ensure(n * 9);
    if (e == hipSuccess) e = dout.ensure(n * 20);
    if (e == hipSuccess) e = dok.ensure(n);
    if (e == hipSuccess) e = hipMemcpy(dpts.p, corners9_host, n * 9 * sizeof(float), hipMemcpyHostToDevice);
    std::vector<float> rec(n * 20);
    std::vector<uint32_t> ok(n);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_make_triangles, dim3((unsigned)std::min<uint64_t>((n + 255) / 256, 2048)), dim3(256), 0, nullptr, (uint32_t)n,
                           dpts.p, dout.p, dok.p);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(rec.data(), dout.p, n * 20 * sizeof(float), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(ok.data(), dok.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost);
    cleanup();
    if (e != hipSuccess) return fail(hip_code(e), std::string("rtmi_make_triangles: ") + hipGetErrorString(e));
    for (uint64_t i = 0; i < n; i++) {
        if (!ok[i]) return fail(RTMI_ERR_INVALID, "make_triangle: degenerate triangle " + std::to_string(i) + " (the reference panics at raytrace.rs:357)");
        rtmi_triangle_t t = *proto;
        const float* o = rec.data() + i * 20;
        memcpy(t.incenter, o, 12); memcpy(t.norm, o + 3, 12); t.bounding_r2 = o[6];
        memcpy(t.sides, o + 7, 36); memcpy(t.side_lens, o + 16, 12);
        out_host[i] = t;
    }
    return RTMI_OK;
    RTMI_GUARD_END
}

struct rtmi_builder {
    int device = 0;
    uint64_t ntris = 0;
    int num_cu = 256;
    DevBuf<float> tris;
    DevBuf<float4> geo;
    DevBuf<uint4> rng;
    DevBuf<uint2> items;
    DevBuf<uint32_t> cand;
    DevBuf<uint8_t> keep;
};

int rtmi_builder_create(int device, const float* tris15, uint64_t ntris, rtmi_builder_t** out) {
    if (!out) return fail(RTMI_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!tris15 || ntris == 0) return fail(RTMI_ERR_INVALID, "no triangles");
    if (ntris >= (1ull << 30)) return fail(RTMI_ERR_UNSUPPORTED, "more than 2^30 triangles");
    const int ndev = rtmi_device_count();
    if (ndev <= 0) return fail(RTMI_ERR_NO_DEVICE, "no HIP device visible: the MI355X kernels cannot run (there is no CPU fallback)");
    if (device < 0 || device >= ndev) return fail(RTMI_ERR_INVALID, "device index out of range");
    RTMI_GUARD_BEGIN
    HIPCHK(hipSetDevice(device));
    rtmi_builder* b = new rtmi_builder();
    b->device = device; b->ntris = ntris;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) b->num_cu = prop.multiProcessorCount;
    hipError_t e = b->tris.ensure(ntris * 15);
    if (e == hipSuccess) e = hipMemcpy(b->tris.p, tris15, ntris * 15 * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) { rtmi_builder_destroy(b); return fail(hip_code(e), std::string("rtmi_builder_create: ") + hipGetErrorString(e)); }
    *out = b;
    return RTMI_OK;
    RTMI_GUARD_END
}

int rtmi_builder_destroy(rtmi_builder_t* b) {
    if (!b) return RTMI_OK;
    (void)hipSetDevice(b->device);
    b->tris.release(); b->geo.release(); b->rng.release(); b->items.release(); b->cand.release(); b->keep.release();
    delete b;
    return RTMI_OK;
}

int rtmi_builder_filter(rtmi_builder_t* b, const rtmi_build_box_t* boxes, uint64_t nboxes, const uint32_t* cand, uint64_t ncand,
                        uint8_t* keep, uint64_t nkeep) {
    if (!b) return fail(RTMI_ERR_INVALID, "builder is NULL");
    if (nboxes == 0 || nkeep == 0) return RTMI_OK;
    if (!boxes || !cand || !keep) return fail(RTMI_ERR_INVALID, "NULL argument");
    if (nboxes >= (1ull << 32) || ncand >= (1ull << 32)) return fail(RTMI_ERR_UNSUPPORTED, "level too large for 32-bit indices");
    RTMI_GUARD_BEGIN
    // validate on the host: every range inside `cand` / `keep`, every candidate a triangle of the handle
    for (uint64_t k = 0; k < ncand; k++)
        if (cand[k] >= b->ntris) return fail(RTMI_ERR_INVALID, "candidate triangle index out of range");
    std::vector<float4> geo(nboxes);
    std::vector<uint4> rng(nboxes);
    std::vector<uint2> items;
    for (uint64_t i = 0; i < nboxes; i++) {
        const rtmi_build_box_t& bx = boxes[i];
        if ((uint64_t)bx.cand_first + bx.cand_count > ncand || bx.keep_first + bx.cand_count > nkeep)
            return fail(RTMI_ERR_INVALID, "box candidate range out of bounds");
        geo[i] = make_float4(bx.orig[0], bx.orig[1], bx.orig[2], bx.len2);
        rng[i] = make_uint4(bx.cand_first, bx.cand_count, (uint32_t)bx.keep_first, (uint32_t)(bx.keep_first >> 32));
        for (uint32_t lo = 0; lo < bx.cand_count; lo += 256) items.push_back(make_uint2((uint32_t)i, lo));
    }
    if (items.empty()) return RTMI_OK;
    if (items.size() >= (1ull << 32)) return fail(RTMI_ERR_UNSUPPORTED, "level too large");
    HIPCHK(hipSetDevice(b->device));
    HIPCHK(b->geo.ensure(nboxes)); HIPCHK(b->rng.ensure(nboxes)); HIPCHK(b->items.ensure(items.size()));
    HIPCHK(b->cand.ensure(ncand)); HIPCHK(b->keep.ensure(nkeep));
    HIPCHK(hipMemcpy(b->geo.p, geo.data(), nboxes * sizeof(float4), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(b->rng.p, rng.data(), nboxes * sizeof(uint4), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(b->items.p, items.data(), items.size() * sizeof(uint2), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(b->cand.p, cand, ncand * sizeof(uint32_t), hipMemcpyHostToDevice));
    // the caller's flags go up and come back: those outside every box's range return as they were
    HIPCHK(hipMemcpy(b->keep.p, keep, nkeep, hipMemcpyHostToDevice));
    const unsigned grid = (unsigned)std::min<uint64_t>(items.size(), (uint64_t)b->num_cu * 64);
    hipLaunchKernelGGL(k_box_contains, dim3(grid), dim3(256), 0, nullptr, b->tris.p, b->geo.p, b->rng.p, b->items.p, (uint32_t)items.size(),
                       b->cand.p, b->keep.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(keep, b->keep.p, nkeep, hipMemcpyDeviceToHost));
    return RTMI_OK;
    RTMI_GUARD_END
}

// ---------------------------------------------------------------- the a-trous denoiser (denoise.hpp)
void rtmi_denoise_defaults(rtmi_denoise_t* p) {
    if (!p) return;
    p->iterations = 3; p->flags = 0;
    p->sigma_color = 1.0f; p->sigma_normal = 0.5f; p->sigma_depth = 0.1f; p->sigma_albedo = INFINITY;
}

// Checks of the denoise entry points that come before any HIP call and before the scene is used (a CPU-only caller reaches
// them).  bufs: colour, albedo, normal, output.
static int check_denoise(const rtmi_scene_t* s, uint32_t width, uint32_t height, const void* const* bufs, const rtmi_denoise_t* p) {
    if (!s) return fail(RTMI_ERR_INVALID, "denoise: NULL argument (scene)");
    if (!p) return fail(RTMI_ERR_INVALID, "denoise: NULL argument (params)");
    static const char* const names[4] = {"color", "albedo", "normal", "out"};
    for (int k = 0; k < 4; k++)
        if (!bufs[k]) return fail(RTMI_ERR_INVALID, std::string("denoise: NULL argument (") + names[k] + ")");
    for (int k = 0; k < 3; k++)
        if (bufs[k] == bufs[3]) return fail(RTMI_ERR_INVALID, std::string("denoise: out must not alias ") + names[k] + " (the filter is never in place)");
    if (width == 0 || height == 0) return fail(RTMI_ERR_INVALID, "denoise: empty image (width or height is 0)");
    if ((uint64_t)width * height >= (1ull << 32)) return fail(RTMI_ERR_UNSUPPORTED, "denoise: more than 2^32 pixels");
    if (p->iterations == 0 || p->iterations > 8) return fail(RTMI_ERR_INVALID, "denoise: iterations must be 1..8");
    if (p->flags & ~(uint32_t)RTMI_DENOISE_DEMODULATE) return fail(RTMI_ERR_INVALID, "denoise: unknown flags");
    const float sg[4] = {p->sigma_color, p->sigma_normal, p->sigma_depth, p->sigma_albedo};
    static const char* const sn[4] = {"sigma_color", "sigma_normal", "sigma_depth", "sigma_albedo"};
    for (int k = 0; k < 4; k++)
        if (!(sg[k] > 0.f)) return fail(RTMI_ERR_INVALID, std::string("denoise: ") + sn[k] + " must be > 0 (+inf switches the term off)");
    return RTMI_OK;
}

// check_denoise plus the two images of the variance-guided filter.  bufs: colour, albedo, normal, output; var_out may be NULL.
static int check_denoise_var(const rtmi_scene_t* s, uint32_t width, uint32_t height, const void* const* bufs, const void* variance,
                             const void* var_out, const rtmi_denoise_t* p) {
    if (!s) return fail(RTMI_ERR_INVALID, "denoise: NULL argument (scene)");
    if (!p) return fail(RTMI_ERR_INVALID, "denoise: NULL argument (params)");
    if (!variance) return fail(RTMI_ERR_INVALID, "denoise: NULL argument (variance)");
    if (variance == bufs[3]) return fail(RTMI_ERR_INVALID, "denoise: out must not alias variance (the filter is never in place)");
    static const char* const names[3] = {"color", "albedo", "normal"};
    if (var_out) {
        for (int k = 0; k < 3; k++)
            if (var_out == bufs[k]) return fail(RTMI_ERR_INVALID, std::string("denoise: var_out must not alias ") + names[k]);
        if (var_out == variance) return fail(RTMI_ERR_INVALID, "denoise: var_out must not alias variance (the filter is never in place)");
        if (var_out == bufs[3]) return fail(RTMI_ERR_INVALID, "denoise: var_out must not alias out");
    }
    return check_denoise(s, width, height, bufs, p);
}

// The launches of one call of either filter, on `st`; variance == NULL: the plain one (var_out is NULL then).  Colour:
// iteration i reads what iteration i - 1 wrote (the first: color) and the last writes out, so out and the first image of the
// mode's scratch alternate backwards from out.  Variance: iteration i reads what iteration i - 1 wrote (the first: variance)
// into the scratch's second and third image in turn; the last writes var_out, or nothing.  The two filters keep their own
// scratch: a plain call on one stream and a variance-guided one on another do not meet.  The caller has checked the arguments.
static int enqueue_atrous(rtmi_scene* s, uint32_t W, uint32_t H, const float4* color, const float4* albedo, const float4* normal,
                          const float4* variance, const rtmi_denoise_t& p, float4* out, float4* var_out, hipStream_t st) {
    static constexpr decltype(&k_atrous<false, false>) kernels[2][2] = {{k_atrous<false, false>, k_atrous<false, true>},
                                                                        {k_atrous<true, false>, k_atrous<true, true>}};
    (void)hipGetLastError();
    const bool var = variance != nullptr;
    DevBuf<float4>& scratch = var ? s->dnv_scratch : s->dn_scratch;
    const uint32_t lds_max_step = var ? s->dnv_lds_max_step : s->dn_lds_max_step;
    const uint32_t n = p.iterations;
    const size_t npix = (size_t)W * H;
    if (n > 1) HIPCHK(scratch.ensure((var ? 3 : 1) * npix));
    const bool demod = (p.flags & RTMI_DENOISE_DEMODULATE) != 0;
    const uint32_t ntiles = ((W + DN_TW - 1) / DN_TW) * ((H + DN_TH - 1) / DN_TH);
    const dim3 grid(std::min<uint32_t>(ntiles, 1u << 20)), block(DN_TW * DN_TH);
    const float s2c = p.sigma_color * p.sigma_color;
    float scale = 1.f;  // 4^-i, exact
    const float4* src = color;
    const float4* vsrc = variance;
    for (uint32_t i = 0; i < n; i++, scale = scale * 0.25f) {
        float4* dst = ((n - 1 - i) & 1u) ? scratch.p : out;
        float4* vdst = !var || i == n - 1 ? var_out : scratch.p + (1 + (i & 1u)) * npix;
        const uint32_t step = 1u << i;
        // the colour width: plain, sigma_color^2 * 4^-i; variance-guided, sigma_color^2 at every iteration (times 1, exact)
        const DenoiseK k{p.sigma_normal * p.sigma_normal, p.sigma_depth, p.sigma_albedo * p.sigma_albedo, s2c * (var ? 1.f : scale)};
        const uint32_t fl = (demod && i == 0 ? DN_DEMOD_IN : 0u) | (demod && i == n - 1 ? DN_REMOD_OUT : 0u);
        const bool stage = step <= lds_max_step;
        const size_t lds = stage ? (size_t)(DN_TW + 4 * step) * (DN_TH + 4 * step) * (var ? 4 : 3) * sizeof(float4) : 0;
        hipLaunchKernelGGL(kernels[stage][var], grid, block, lds, st, W, H, step, src, vsrc, albedo, normal, dst, vdst, k, fl);
        HIPCHK(hipGetLastError());
        src = dst; vsrc = vdst;
    }
    return RTMI_OK;
}

// The host variants: the images (colour, albedo, normal and, variance-guided, variance) are copied into the mode's buffer of
// the handle, filtered there and the result(s) are copied out.  The caller has checked the arguments.
static int denoise_host(rtmi_scene* s, uint32_t W, uint32_t H, const void* const* bufs, const float* variance, const rtmi_denoise_t& p,
                        float* out, float* var_out) {
    const void* const in[4] = {bufs[0], bufs[1], bufs[2], variance};
    const size_t npix = (size_t)W * H, nin = variance ? 4 : 3;
    DevBuf<float4>& buf = variance ? s->dnv_host : s->dn_host;
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(buf.ensure((nin + (variance ? 2 : 1)) * npix));  // the inputs, the result and, variance-guided, var_out's
    float4* d = buf.p;
    for (size_t k = 0; k < nin; k++) HIPCHK(hipMemcpy(d + k * npix, in[k], npix * sizeof(float4), hipMemcpyHostToDevice));
    float4 *res = d + nin * npix, *vres = var_out ? res + npix : nullptr;
    const int rc = enqueue_atrous(s, W, H, d, d + npix, d + 2 * npix, variance ? d + 3 * npix : nullptr, p, res, vres, nullptr);
    if (rc != RTMI_OK) return rc;
    HIPCHK(hipMemcpy(out, res, npix * sizeof(float4), hipMemcpyDeviceToHost));
    if (var_out) HIPCHK(hipMemcpy(var_out, vres, npix * sizeof(float4), hipMemcpyDeviceToHost));
    return RTMI_OK;
}

int rtmi_denoise_device(rtmi_scene_t* s, uint32_t width, uint32_t height, const void* color_device, const void* albedo_device,
                        const void* normal_device, const rtmi_denoise_t* params, void* out_device, void* hip_stream) {
    RTMI_GUARD_BEGIN
    const void* const bufs[4] = {color_device, albedo_device, normal_device, out_device};
    const int rc = check_denoise(s, width, height, bufs, params);
    if (rc != RTMI_OK) return rc;
    HIPCHK(hipSetDevice(s->device));
    return enqueue_atrous(s, width, height, (const float4*)color_device, (const float4*)albedo_device, (const float4*)normal_device,
                          nullptr, *params, (float4*)out_device, nullptr, (hipStream_t)hip_stream);
    RTMI_GUARD_END
}

int rtmi_denoise(rtmi_scene_t* s, uint32_t width, uint32_t height, const float* color_host, const float* albedo_host,
                 const float* normal_host, const rtmi_denoise_t* params, float* out_host) {
    RTMI_GUARD_BEGIN
    const void* const bufs[4] = {color_host, albedo_host, normal_host, out_host};
    const int rc = check_denoise(s, width, height, bufs, params);
    if (rc != RTMI_OK) return rc;
    return denoise_host(s, width, height, bufs, nullptr, *params, out_host, nullptr);
    RTMI_GUARD_END
}

// Render, features over all samples and the filter, all on the handle's own device images; only the result crosses to the host.
int rtmi_render_denoised(rtmi_scene_t* s, const rtmi_viewport_t* vp, uint64_t seed, const rtmi_denoise_t* params, float* out_host,
                         rtmi_stats_t* stats) {
    if (stats) memset(stats, 0, sizeof(*stats));
    RTMI_GUARD_BEGIN
    if (!vp) return fail(RTMI_ERR_INVALID, "denoise: NULL argument (viewport)");
    static const char own[3] = {};  // stand for the handle's images in the checks: they exist and do not alias
    const void* const bufs[4] = {own, own + 1, own + 2, out_host};
    const int rc0 = check_denoise(s, vp->width, vp->height, bufs, params);
    if (rc0 != RTMI_OK) return rc0;
    const size_t npix = (size_t)vp->width * vp->height;
    const rtmi_tile_t tile{0u, vp->height, vp->height, 0u};
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(s->dn_host.ensure(4 * npix));
    float4* d = s->dn_host.p;
    int rc = rtmi_render_tile_device(s, vp, seed, &tile, d, nullptr, stats);
    if (rc != RTMI_OK) return rc;
    rc = rtmi_render_features_device(s, vp, seed, &tile, 0u, vp->samples_per_pixel, d + npix, d + 2 * npix, nullptr, nullptr, nullptr);
    if (rc != RTMI_OK) { if (stats) memset(stats, 0, sizeof(*stats)); return rc; }
    rc = enqueue_atrous(s, vp->width, vp->height, d, d + npix, d + 2 * npix, nullptr, *params, d + 3 * npix, nullptr, nullptr);
    if (rc != RTMI_OK) return rc;
    HIPCHK(hipMemcpy(out_host, d + 3 * npix, npix * sizeof(float4), hipMemcpyDeviceToHost));
    return RTMI_OK;
    RTMI_GUARD_END
}

// ---------------------------------------------------------------- variance-guided denoising (denoise.hpp)
void rtmi_denoise_var_defaults(rtmi_denoise_t* p) {
    if (!p) return;
    p->iterations = 1; p->flags = 0;
    p->sigma_color = 3.0f; p->sigma_normal = 0.5f; p->sigma_depth = 0.1f; p->sigma_albedo = INFINITY;
}

int rtmi_variance_device(rtmi_scene_t* s, const void* accum_device, const void* sumsq_device, const void* counts_device,
                         uint64_t npixels, void* variance_device, void* hip_stream) {
    if (!s) return fail(RTMI_ERR_INVALID, "variance: NULL argument (scene)");
    if (npixels == 0) return RTMI_OK;
    if (!accum_device || !sumsq_device || !counts_device || !variance_device)
        return fail(RTMI_ERR_INVALID, "variance: NULL argument (accum, sumsq, counts and variance are required)");
    if (variance_device == accum_device || variance_device == sumsq_device || variance_device == counts_device)
        return fail(RTMI_ERR_INVALID, "variance: the output must not alias an input");
    HIPCHK(hipSetDevice(s->device));
    const unsigned grid = (unsigned)std::min<uint64_t>((npixels + 255) / 256, (uint64_t)s->num_cu * 8);
    hipLaunchKernelGGL(k_variance, dim3(grid), dim3(256), 0, (hipStream_t)hip_stream, (uint64_t)npixels, (const float4*)accum_device,
                       (const float4*)sumsq_device, (const uint32_t*)counts_device, (float4*)variance_device);
    HIPCHK(hipGetLastError());
    return RTMI_OK;
}

// Host variant: the moments are copied into the handle's own buffers, the kernel runs there and the image is copied out.
int rtmi_variance(rtmi_scene_t* s, const float* accum_host, const float* sumsq_host, const uint32_t* counts_host, uint64_t npixels,
                  float* variance_host) {
    RTMI_GUARD_BEGIN
    if (!s) return fail(RTMI_ERR_INVALID, "variance: NULL argument (scene)");
    if (npixels == 0) return RTMI_OK;
    if (!accum_host || !sumsq_host || !counts_host || !variance_host)
        return fail(RTMI_ERR_INVALID, "variance: NULL argument (accum, sumsq, counts and variance are required)");
    if ((const void*)variance_host == accum_host || (const void*)variance_host == sumsq_host || (const void*)variance_host == counts_host)
        return fail(RTMI_ERR_INVALID, "variance: the output must not alias an input");
    if (npixels >= (1ull << 32)) return fail(RTMI_ERR_UNSUPPORTED, "variance: more than 2^32 pixels in one host call");
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(s->dnv_host.ensure(3 * npixels));
    HIPCHK(s->dnv_cnt.ensure(npixels));
    float4* d = s->dnv_host.p;
    HIPCHK(hipMemcpy(d, accum_host, npixels * sizeof(float4), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d + npixels, sumsq_host, npixels * sizeof(float4), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(s->dnv_cnt.p, counts_host, npixels * sizeof(uint32_t), hipMemcpyHostToDevice));
    const int rc = rtmi_variance_device(s, d, d + npixels, s->dnv_cnt.p, npixels, d + 2 * npixels, nullptr);
    if (rc != RTMI_OK) return rc;
    HIPCHK(hipMemcpy(variance_host, d + 2 * npixels, npixels * sizeof(float4), hipMemcpyDeviceToHost));
    return RTMI_OK;
    RTMI_GUARD_END
}

int rtmi_denoise_var_device(rtmi_scene_t* s, uint32_t width, uint32_t height, const void* color_device, const void* albedo_device,
                            const void* normal_device, const void* variance_device, const rtmi_denoise_t* params, void* out_device,
                            void* var_out_device, void* hip_stream) {
    RTMI_GUARD_BEGIN
    const void* const bufs[4] = {color_device, albedo_device, normal_device, out_device};
    const int rc = check_denoise_var(s, width, height, bufs, variance_device, var_out_device, params);
    if (rc != RTMI_OK) return rc;
    HIPCHK(hipSetDevice(s->device));
    return enqueue_atrous(s, width, height, (const float4*)color_device, (const float4*)albedo_device, (const float4*)normal_device,
                          (const float4*)variance_device, *params, (float4*)out_device, (float4*)var_out_device, (hipStream_t)hip_stream);
    RTMI_GUARD_END
}

int rtmi_denoise_var(rtmi_scene_t* s, uint32_t width, uint32_t height, const float* color_host, const float* albedo_host,
                     const float* normal_host, const float* variance_host, const rtmi_denoise_t* params, float* out_host,
                     float* var_out_host) {
    RTMI_GUARD_BEGIN
    const void* const bufs[4] = {color_host, albedo_host, normal_host, out_host};
    const int rc = check_denoise_var(s, width, height, bufs, variance_host, var_out_host, params);
    if (rc != RTMI_OK) return rc;
    return denoise_host(s, width, height, bufs, variance_host, *params, out_host, var_out_host);
    RTMI_GUARD_END
}

// Adaptive render, variance image, features of the samples every pixel has and the filter, all on the handle's own device
// images (accum, sumsq, colour, variance, albedo, normal, result); only the result and the counts cross to the host.
int rtmi_render_adaptive_denoised(rtmi_scene_t* s, const rtmi_viewport_t* vp, uint64_t seed, rtmi_adaptive_t* ad,
                                  const rtmi_denoise_t* params, float* out_host, uint32_t* counts_host, rtmi_stats_t* stats) {
    if (stats) memset(stats, 0, sizeof(*stats));
    RTMI_GUARD_BEGIN
    static const char own[8] = {};  // stand for the handle's images in the checks: they exist and do not alias
    if (!s) return fail(RTMI_ERR_INVALID, "denoise: NULL argument (scene)");
    if (!vp) return fail(RTMI_ERR_INVALID, "denoise: NULL argument (viewport)");
    if (out_host && (const void*)out_host == (const void*)counts_host) return fail(RTMI_ERR_INVALID, "denoise: out must not alias counts");
    const void* const dbufs[4] = {own, own + 1, own + 2, out_host};
    int rc = check_denoise_var(s, vp->width, vp->height, dbufs, own + 3, nullptr, params);
    if (rc != RTMI_OK) return rc;
    const void* abufs[4] = {own + 4, own + 5, own + 6, own + 7};
    rc = check_adaptive(s, vp, ad, abufs, 4, true);
    if (rc != RTMI_OK) return rc;
    const rtmi_tile_t tile{0u, vp->height, vp->height, 0u};
    rtmi_viewport_t v1;
    bool empty;
    rc = check_features(s, vp, &tile, 0u, ad->min_samples, own, own + 1, nullptr, v1, &empty);
    if (rc != RTMI_OK) return rc;
    rc = check_view(vp, &tile);
    if (rc != RTMI_OK) return rc;
    if (s->d.nspheres)
        return fail(RTMI_ERR_UNSUPPORTED, "denoise: the scene has analytic spheres (a build-defined primitive without feature buffers)");
    const size_t npix = (size_t)vp->width * vp->height;
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(s->dnv_host.ensure(7 * npix));
    HIPCHK(s->dnv_cnt.ensure(npix));
    float4* d = s->dnv_host.p;
    float4 *accum = d, *sumsq = d + npix, *color = d + 2 * npix, *var = d + 3 * npix, *alb = d + 4 * npix, *nrm = d + 5 * npix, *res = d + 6 * npix;
    rc = rtmi_render_adaptive_device(s, vp, seed, &tile, ad, accum, sumsq, s->dnv_cnt.p, color, nullptr, stats);
    if (rc != RTMI_OK) return rc;
    rc = rtmi_variance_device(s, accum, sumsq, s->dnv_cnt.p, npix, var, nullptr);
    if (rc == RTMI_OK) rc = rtmi_render_features_device(s, vp, seed, &tile, 0u, ad->min_samples, alb, nrm, nullptr, nullptr, nullptr);
    if (rc == RTMI_OK) rc = enqueue_atrous(s, vp->width, vp->height, color, alb, nrm, var, *params, res, nullptr, nullptr);
    if (rc != RTMI_OK) { if (stats) memset(stats, 0, sizeof(*stats)); return rc; }
    HIPCHK(hipMemcpy(out_host, res, npix * sizeof(float4), hipMemcpyDeviceToHost));
    if (counts_host) HIPCHK(hipMemcpy(counts_host, s->dnv_cnt.p, npix * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return RTMI_OK;
    RTMI_GUARD_END
}

int rtmi_quantize_device(rtmi_scene_t* s, const void* rgba_device, uint64_t npixels, void* rgb_device, void* hip_stream) {
    if (!s) return fail(RTMI_ERR_INVALID, "scene is NULL");
    if (npixels == 0) return RTMI_OK;
    if (!rgba_device || !rgb_device) return fail(RTMI_ERR_INVALID, "NULL argument");
    HIPCHK(hipSetDevice(s->device));
    hipLaunchKernelGGL(k_quantize, dim3((unsigned)(s->num_cu * 8)), dim3(256), 0, (hipStream_t)hip_stream, (uint64_t)npixels,
                       (const float4*)rgba_device, (uint8_t*)rgb_device);
    HIPCHK(hipGetLastError());
    return RTMI_OK;
}

int rtmi_quantize(rtmi_scene_t* s, const float* rgba_host, uint64_t npixels, uint8_t* rgb_host) {
    if (!s) return fail(RTMI_ERR_INVALID, "scene is NULL");
    if (npixels == 0) return RTMI_OK;
    if (!rgba_host || !rgb_host) return fail(RTMI_ERR_INVALID, "NULL argument");
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(s->tile.ensure(npixels));
    HIPCHK(s->qbytes.ensure(npixels * 3));
    HIPCHK(hipMemcpy(s->tile.p, rgba_host, npixels * 16, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_quantize, dim3((unsigned)(s->num_cu * 8)), dim3(256), 0, nullptr, (uint64_t)npixels, s->tile.p, s->qbytes.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(rgb_host, s->qbytes.p, npixels * 3, hipMemcpyDeviceToHost));
    return RTMI_OK;
}

}  // extern "C"
