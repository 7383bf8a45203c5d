// trace_oct.hpp — the closest-hit kernel for trees that are exact octrees
// (what build_bounding_box produces, raytrace_lib/src/raytrace.rs:795-845;
// checked box by box in rtmi_scene_create, otherwise the generic kernel of
// rtmi_device.hip runs).  Included by rtmi_device.hip.
//
// Same traversal order and skip rule as get_object_intersection_for_ray
// (raytrace.rs:909-1010), restructured for a 64-lane wavefront:
//
//  * one lane = one ray, lanes are PERSISTENT: a lane that finishes pulls the
//    next queued ray (wave ballot + prefix sum over the idle lanes, one atomic
//    per refill), so a wave stays full until the queue is empty;
//  * a lane is in one of two working states, SELECT (at an inner box: pop
//    finished frames, pick the next child) or LEAF (scan one 16-B block of
//    triangle references).  Each iteration the wave runs the step that the
//    majority of its lanes wait for (weighted 3 : 2 towards SELECT, whose
//    step is the cheaper one), instead of serialising nested loops;
//  * LAZY CHILD SELECTION instead of a sort.  The reference sorts the <= 8
//    colliding children by tmin (stable insertion sort, raytrace.rs:941-947)
//    and folds over them.  Visiting "the smallest tmin not visited yet, lowest
//    index on ties" one child at a time is the same order, and a ray enters
//    only ~1.4 children of a box on average, so the kernel never sorts: every
//    SELECT step recomputes the 8 implicit child slabs of the current box
//    (6 plane pairs + 8 max3/min3, nothing loaded but the box's own 32-B
//    record), masks out absent and already visited children, takes the
//    minimum and applies the skip rule to it.  Half the VALU work of the
//    previous sort-then-recheck form (rank sort 105 + recheck 25 per child);
//  * child boxes are implicit: the 8 children of a box share 2 candidate
//    planes per axis (centre +- half/2).  The child centres are recomputed
//    with the builder's own expression (orig + (+-newlen2), raytrace.rs:816-824)
//    and were verified bitwise at scene creation;
//  * the Triangle::intersects edge part (3 half-plane dots, 4 more records)
//    is needed by ~4 % of the plane tests.  It is DEFERRED: the plane tests of
//    a block run branch-free for all lanes, a lane remembers its candidate and
//    the edge part runs once per step for all lanes that have one;
//  * the stack of frames lives in LDS, [level][word][lane], 2 words per frame
//    (record index | flags << 22, best t): a lane only ever touches its own
//    bank;
//  * nothing but the ray, the current frame, the running best and the leaf
//    cursor is carried from step to step, and the loop has ONE back edge:
//    hipcc copies every loop-carried register that is written inside nested
//    divergent branches into a temporary and back ("the
//    instruction diet").
//
// Records (HBM, served from L2 / Infinity Cache):
//   fnodes  : 2 x uint4 (32 B) per INNER box: (cx, cy, cz, present mask | leaf mask << 8 | FN_WIDE)
//             (first inner child's record, first block of the first leaf child, 8 x u8 block offsets of the leaf
//             children).  The inner children of a box are consecutive records in octant order, so a child's record
//             follows from the masks with a popcount.  Leaves have no record; a leaf child's first block is the
//             smallest first block among the box's leaf children + a byte offset per octant.  A box whose leaf children
//             start more than 255 blocks apart (FN_WIDE) keeps 8 explicit 32-bit block indices in `wlinks` instead (one
//             more dependent load).
//   oblocks : uint4 blocks of triangle indices of a leaf list, in list order.  The list ends at the first index 0
//             (the sentinel triangle is never in a tree, raytrace.rs:791) or after a full block whose 4th
//             index has bit 31 set.  Each DISTINCT list is stored once (leaves with the same list share its blocks), so
//             a list's first block is its identity -- what the leaf memo of oct_walk compares.
//   ocull   : per reference block, same index, a record by which k_trace_oct rejects the whole block for a ray ("Block cull"
//             below); null: no block cull.  With `cert`: one uint4 (16 B), a bf16 box around the block's triangles; without:
//             2 x uint4 (32 B), an f32 box and a box around the triangles' normals.
//   cert    : the distinct normals of the scene binned by ray direction; a ray uses the 16-B records only when it is certified
//             against its cell's list ("Sign certificate per ray" below); null: the scene has too many distinct normals for
//             the table (or no block cull).
//   fcull   : per record of `fnodes`, same index, one uint4 (16 B) in the form of a packed ocull record: a bf16 box around every
//             block box below that inner box, by which a certified ray rejects the whole subtree ("Node cull" below); null:
//             no node cull (always when `cert` is null).
#pragma once

namespace rtmi {

enum : uint32_t { M_IDLE = 0, M_SELECT = 1, M_LEAF = 2, M_SHADE = 3 };

// What a lane does when its ray's root frame is finished -- the three kernels share one walk (oct_walk):
//   W_TRACE    k_trace_oct     rays come from a queue, the closest hit goes to hit_tf / hit_t (one launch per bounce pass,
//                              shaded by k_shade; rtmi_trace)
//   W_PRIMARY  k_path_primary  pixel_ray() is evaluated by the lane that takes the path (no ray queue for primary rays),
//                              the finished ray is shaded IN the kernel (color_ray, shade.hpp): terminal paths write their
//                              sample colour, bounce rays are compacted into the bounce queue (ballot + prefix sum, one
//                              atomic per wave).  Whole-wave refills keep the samples of a pixel in lockstep.  A wave whose
//                              primary rays hit a mirror (at least a.minpl lanes) traces their reflections ITSELF, as the same
//                              packet, and queues what follows them for pass 2 ("Mirror paths in place").
//   W_SLOW     k_path_slow     the slow-path queue (SlowQ, rtmi_device.hip: rays with an exactly-zero direction component,
//                              ~150 x the work of an ordinary ray), one path per WAVE at a time (lane 0): the lane traces
//                              the path's ray, shades it in place and -- when the path goes on -- re-seeds ITSELF with the
//                              next bounce ray, until the path ends (the recursion project_ray -> color_ray -> project_ray,
//                              raytrace.rs:1233-1251, :1256-1295, without pass boundaries).  Such a ray runs at the speed
//                              of a lone lane while the ordinary passes go on beside it on their own stream.
//   W_RECORD   k_trace_record  W_TRACE's queue and exact walk (COUNT, not FAST), and per ray a record of what the walk did:
//                              its work counters (cnt[] from the moment the lane takes the ray until it finishes it) and,
//                              when RecArgs::lids is given, the leaves it entered in visiting order, each as
//                              (inner record << 3) | octant (rtmi_trace_records / rtmi_primary_records)
// Shading in the path kernels is a third step kind ("exchange"): finished lanes wait in M_SHADE until `refill_min` lanes
// are finished or idle (or nothing else is left to do), then they are shaded together and, in the same step, every lane
// without a ray takes one from the queue.  The arithmetic per path is k_shade's (same device functions), so the image is
// bit-identical; only which lane evaluates it, and when, differs.
//   W_OCCL     k_occluded_oct  W_TRACE's queue and walk as an ANY-HIT query (rtmi_occluded*): every ray has a
//                              limit tmax, and the answer is 1 iff the closest hit's t < tmax.  The running best only ever
//                              moves to a smaller t, so a lane retires its ray with 1 as soon as its running best -- or the
//                              leaf accumulator that the merge would put there -- is < tmax; a ray that never gets there is
//                              walked to the end exactly like W_TRACE's and answers 0.  One byte per ray is written.
enum : int { W_TRACE = 0, W_PRIMARY = 1, W_SLOW = 2, W_RECORD = 3, W_OCCL = 4 };

struct OctArgs {
    // W_TRACE
    const float4* qo; const float4* qd; uint32_t* hit_tf; float* hit_t; int pass;
    // W_PRIMARY / W_SLOW
    DView v; uint64_t seed; uint32_t pix0, npaths;
    float4* bqo; float4* bqd; uint32_t* bqpath;  // bounce queue: filled by W_PRIMARY (ctrl->count[1] entries), drained by pass 1's k_trace_oct
    uint16_t* mstack; float4* scol;
    SlowQ slow;       // W_PRIMARY: where zero-component rays go (cap == 0: nowhere, they are traced in place); W_SLOW: the queue
    uint32_t slow_k;  // W_SLOW: which consumer launch this is (its range and cursor in the control block)
    int vote_s, vote_l;  // weights of the SELECT / LEAF vote (3 : 2)
    int pcull;           // W_PRIMARY: packet cull on (RTMI_PACKET_CULL, read at scene creation)
    int bcn;             // W_TRACE: cull records a LEAF step reads and blocks it may skip, 2..4 (RTMI_BLOCK_CULL_N)
    // W_PRIMARY, mirror paths continued in place (RTMI_MIRROR_INPLACE): the pass-2 queue (ping-pong buffer 0, ctrl->count[2]
    // entries; pass 1's k_shade appends to it behind them) and the least number of a wave's mirror lanes for which the wave
    // traces their reflections itself (0: never)
    float4* b2qo; float4* b2qd; uint32_t* b2qpath;
    int minpl;
};

// W_RECORD's outputs, per queued ray i: rcnt[5 i .. 5 i + 4] = box_tests, tri_tests, full_tests, nodes, leaves of that ray;
// lids (null: counts only) receives its leaf ids at [lfirst[i], lfirst[i] + leaves), never at or past lcap
struct RecArgs {
    uint32_t* rcnt;
    const unsigned long long* lfirst;
    uint32_t* lids;
    unsigned long long lcap;
};

// W_OCCL's buffers, per queued ray i: tmax[i] (null: +inf for every ray) in, occ[i] = 0 or 1 out
struct OcclArgs {
    const float* tmax;
    uint8_t* occ;
};

// Frame of an inner box: node = index of its record; w = visited octants (bits 0-7) | O_DONE | O_HAS;
// t = best hit time inside this box's subtree so far (what the sibling-local skip rule compares against,
// raytrace.rs:965).  Which triangle that was is NOT kept per frame: the ray keeps one running best (t, tri)
// over its leaf results in visiting order.  That equals the reference's nested per-box merge also when hit
// times are NaN: a NaN leaf result is only ever taken by a frame (or by the running best) that has no hit
// yet, it then blocks every later sibling at every level it reaches (`tmin < NaN` is false), and a frame
// that already has a hit drops it (`NaN < t` is false) exactly like the running best does.
#define O_DONE 0x100u
#define O_HAS 0x200u
#define FN_WIDE 0x10000u

// v_max3_f32 / v_min3_f32: max(max(a,b),c) with fmaxf's NaN rule (a NaN operand is ignored), one instruction
// instead of the two v_max + canonicalising moves hipcc emits for nested fmaxf.
__device__ inline float max3f(float a, float b, float c) {
    float d;
    asm("v_max3_f32 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
    return d;
}
__device__ inline float min3f(float a, float b, float c) {
    float d;
    asm("v_min3_f32 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
    return d;
}

// 16-byte record at a 32-bit byte offset from a wave-uniform base: the `global_load_dwordx4 v, v_off, s[base]` form, one
// VALU instruction for the address instead of a 64-bit shift and add (rtmi_scene_create checks that every array of the
// octree form is smaller than 4 GiB)
template <typename T>
__device__ inline T ld_off32(const T* base, uint32_t byte_off) {
    return *reinterpret_cast<const T*>(reinterpret_cast<const char*>(base) + (size_t)byte_off);
}

// ---- Packet cull (W_PRIMARY, DESIGN.md 4.1 "Packet cull"; rtmi_debug_packet_cull runs the same functions on the host).
// A whole-wave refill of k_path_primary gives the 64 lanes samples of one pixel: nearly the same ray.  The refill records
// a reference ray (o0, d0) -- the first lane's that took one -- and bounds so >= |o_i - o0|, sd >= |d_i - d0| over those
// lanes (L1 norms, >= the Euclidean ones, rounded up).  A LEAF step whose lanes all stand at the same block then tests
// each of its 4 triangles ONCE against the packet: packet_culls() proves that the exact plane test rejects it for every ray
// of the packet, and only the triangles it cannot reject get the exact test.  Only IEEE + - * / and sqrtf, so host and
// device compute the same bits.
struct Packet {
    float ox, oy, oz, dx, dy, dz;  // reference ray
    float so, sd;                  // spreads of origin and direction
    float eabs;                    // K (2 so + |o0|) (1 + K) + 1e-18: the ray-only absolute terms of the bound on |q - c|
    float dhi, dinv;               // |d0| (1 + K); 1 / min_i |d_i|, rounded up
    float pad;
};
// W_PRIMARY's LDS header, in front of the frame stack (a constant address): the packet of the last whole-wave refill, and
// what only the exchange step reads -- the pass-2 queue and the in-place threshold of OctArgs (b2qo, b2qd, b2qpath, minpl).
// Kept out of registers: as kernel arguments they are 7 more SGPRs live over the whole loop, and the SGPR spills then take a
// second VGPR, which hipcc wins back by spilling VGPRs inside the LEAF step.
struct PrimHdr {
    Packet pk;
    unsigned long long q2[3];  // pass-2 queue: origins, directions, paths
    uint32_t minpl;            // least number of mirror lanes that a wave continues in place (65: never)
    // Node cull of the primary kernels: byte offset of DScene::fcull from DScene::fnodes (rtmi_scene_create keeps the node
    // cull records behind the node records in one buffer), 0: no node cull.  Read in the SELECT step, where a pointer of
    // its own would be two more scalar registers live over the whole loop.
    uint32_t foff;
    // The last whole-list cull of the LEAF step: blocks [llo, lhi & 0x7FFFFFFF) of a list and, per reference (bit 4 j + k:
    // reference k of block llo + j), the references that survive it (fast build; bit 31 of lhi: the list ends among
    // these blocks) or that it culls (counting build: the range is emptied whenever the packet changes)
    unsigned long long lmask;
    uint32_t llo, lhi;
    // The direction table (DScene::cert) for the certificate of a lane that takes a ray: read per lane where it is used,
    // so that the table's addresses are vector arithmetic of the exchange step and hold no scalar register
    unsigned long long cert;
    unsigned long long pad;
};
#define PK_K 1e-5f  // relative slack: ~170 x the float rounding of any bound below
// One ray of the packet: its spreads against the reference.  False: this ray turns culling off for the packet (nonzero
// lane 3, huge coordinates, a direction outside the pixel's cone, NaN).
__host__ __device__ inline bool packet_spread(const Packet& p, float4 o, float4 d, float& so, float& sd) {
    so = ((fabsf(o.x - p.ox) + fabsf(o.y - p.oy)) + fabsf(o.z - p.oz)) * (1.f + PK_K);
    sd = ((fabsf(d.x - p.dx) + fabsf(d.y - p.dy)) + fabsf(d.z - p.dz)) * (1.f + PK_K);
    return (o.w == 0.f) & (d.w == 0.f) & (so <= 1e15f) & (sd <= 1.f / 64.f);
}
// The packet from the wave maxima of the spreads; false: no culling for it
__host__ __device__ inline bool packet_finish(Packet& p, float so, float sd) {
    p.so = so; p.sd = sd;
    const float o1 = (fabsf(p.ox) + fabsf(p.oy)) + fabsf(p.oz);
    const float dl = sqrtf((p.dx * p.dx + p.dy * p.dy) + p.dz * p.dz);
    const float dlo = dl * (1.f - PK_K) - sd;
    p.eabs = (PK_K * ((so + so) + o1)) * (1.f + PK_K) + 1e-18f;
    p.dhi = dl * (1.f + PK_K);
    p.dinv = (1.f / dlo) * (1.f + PK_K);
    p.pad = 0.f;
    return (o1 <= 1e15f) & (dlo >= 0.25f) & (dl <= 4.f);
}
// True: the exact plane test of the LEAF step (tri_test's `t < 0`, `l2 > r2`) rejects the triangle with plane record
// (p0, p1) for EVERY ray (o_i, d_i) of the packet.  The argument: den_i is certified nonzero with margin,
// so t_i is finite; if a ray passed, its point q = o_i + t d_i would be within emax of the incenter c (rounding of p, ip and
// l2 included) and |t| <= tmax; but q is at least dist(c, line0) - so - |t| sd from c.  Rejected when that exceeds emax.
__host__ __device__ inline bool packet_culls(const Packet& p, float4 p0, float4 p1) {
    const float wx = p0.x - p.ox, wy = p0.y - p.oy, wz = p0.z - p.oz;
    const float c1 = (fabsf(wx) + fabsf(wy)) + fabsf(wz);  // >= |c - o0|
    // den: |n.d0| > 2 X, X >= the spread and rounding of n.d_i, so every |den_i| > X >= max(K |n| |d0|, 1e-30)
    const float den0 = ((p1.x * p.dx + p1.y * p.dy) + p1.z * p.dz);
    const float nn = (fabsf(p1.x) + fabsf(p1.y)) + fabsf(p1.z);
    const float X = (nn * (p.sd + PK_K * (p.dhi + p.sd))) * (1.f + PK_K) + 1e-30f;
    // distance: line0 must pass c farther than emax + so + tmax sd (+ the rounding of the cross product)
    const float rho = sqrtf(p0.w);
    const float emax = (rho + (PK_K * (c1 + p.so) + p.eabs)) * (1.f + PK_K);
    const float tmax = (((emax + c1) + p.so) * p.dinv) * (1.f + PK_K);
    const float lreq = (((emax + p.so) + tmax * p.sd) + PK_K * c1) * (1.f + PK_K);
    const float cx = wy * p.dz - wz * p.dy, cy = wz * p.dx - wx * p.dz, cz = wx * p.dy - wy * p.dx;
    const float x2 = (cx * cx + cy * cy) + cz * cz;  // |(c - o0) x d0|^2 = (dist(c, line0) |d0|)^2
    const float y = lreq * p.dhi;
    return (c1 <= 1e15f) & (nn <= 1e15f) & (fabsf(den0) > X + X) & (x2 > (y * y) * (1.f + PK_K));
}

// ---- Block cull (W_TRACE, DESIGN.md 4.1 "Block cull"; rtmi_debug_block_cull runs the same functions on the host).
// Bounce rays share nothing, so their bound is static: rtmi_scene_create stores one 32-B record per reference block (DScene::
// ocull, the block's index), two uint4:
//   c0 = (lo.x, lo.y, lo.z, hi.x)   c1 = (hi.y, hi.z, nlo.xyz | nhi.x << 24, nhi.y | nhi.z << 8 | flags << 16)
// [lo, hi]: the box of the incenter spheres of the block's real references, each grown by rho K + K (|c|_1 + rho), rounded
// outward; [nlo, nhi]: the box of their unit normals in units of 1/127 (int8), rounded outward.  block_culls() proves that
// the exact plane test rejects all of them for one ray; a lane then skips the block at the cost of two loads.  Only IEEE
// + - * /, min and max.
#define BC_END 1u    // this block ends its list (oblocks: `blk.w == 0 || blk.w >> 31`)
#define BC_NEVER 2u  // a record of the block is outside the ranges of the proof: never culled
#define BC_K 1e-5f
// A ray the cull may be used for: lane 3 zero, |o|_1 <= 1e15, every direction component nonzero with
// 1e-10 <= max |d_k| <= 1e10 and min |d_k| >= 2^-40 max |d_k| (so every 1 / d_k is finite and the t of a reference whose
// den the certificate bounds is < 1e30).  A NaN anywhere gives false.
__host__ __device__ inline bool block_cull_ray(float4 o, float4 d) {
    const float ax = fabsf(d.x), ay = fabsf(d.y), az = fabsf(d.z);
    const float dmax = fmaxf(fmaxf(ax, ay), az), dmin = fminf(fminf(ax, ay), az);
    const float o1 = (fabsf(o.x) + fabsf(o.y)) + fabsf(o.z);
    // (fmaxf / fminf skip a NaN operand: each component is compared on its own)
    return (o.w == 0.f) & (d.w == 0.f) & (o1 <= 1e15f) & (ax > 0.f) & (ay > 0.f) & (az > 0.f) & (ax <= 1e10f) & (ay <= 1e10f) &
           (az <= 1e10f) & (dmax >= 1e-10f) & (dmin >= 0x1p-40f * dmax);
}
// (b) of the predicate, and the whole predicate of the packed records below: the half-line t >= 0 of a ray that
// block_cull_ray() accepts (ix, iy, iz = 1 / d as the walk keeps them) misses the box [lo, hi] grown by K |o|_1.
__host__ __device__ inline bool block_slab_miss(float lox, float loy, float loz, float hix, float hiy, float hiz, float ox, float oy,
                                                float oz, float ix, float iy, float iz) {
    const float e = BC_K * ((fabsf(ox) + fabsf(oy)) + fabsf(oz));
    const float x0 = ((lox - e) - ox) * ix, x1 = ((hix + e) - ox) * ix;
    const float y0 = ((loy - e) - oy) * iy, y1 = ((hiy + e) - oy) * iy;
    const float z0 = ((loz - e) - oz) * iz, z1 = ((hiz + e) - oz) * iz;
    // a NaN end (inf - inf, 0 * inf) must not be skipped by min / max: it turns the test off
    const bool num = (x0 == x0) & (x1 == x1) & (y0 == y0) & (y1 == y1) & (z0 == z0) & (z1 == z1);
    const float tn = fmaxf(fmaxf(fminf(x0, x1), fminf(y0, y1)), fminf(z0, z1));
    const float tf = fminf(fminf(fmaxf(x0, x1), fmaxf(y0, y1)), fmaxf(z0, z1));
    return num & ((tf < 0.f) | (tn - tf > BC_K * (fabsf(tn) + fabsf(tf))));
}
__host__ __device__ inline float bc_bits_float(uint32_t u) {
#ifdef __HIP_DEVICE_COMPILE__
    return __uint_as_float(u);
#else
    float v; memcpy(&v, &u, 4); return v;
#endif
}
// The 32-B record (scenes without a direction table, and rtmi_debug_block_cull; scenes with one use the packed records below).
// Bit 0: (b) the half-line t >= 0 misses the box; bit 1: (a) no norm . dir of the block can be zero.  For a ray that
// block_cull_ray() accepts (ix, iy, iz = 1 / d as the walk keeps them).
__host__ __device__ inline uint32_t block_cull_parts(uint4 c0, uint4 c1, float ox, float oy, float oz, float dx, float dy, float dz,
                                                     float ix, float iy, float iz) {
    auto s8 = [](uint32_t w, int sh) { return (float)((int32_t)(w << (24 - sh)) >> 24); };
    // (a) sign certificate over the normal box, in units of 1/127: L <= 127 u . d <= H for every unit normal u of the block
    const float d1 = (fabsf(dx) + fabsf(dy)) + fabsf(dz);
    const float ax0 = s8(c1.z, 0) * dx, ax1 = s8(c1.z, 24) * dx;
    const float ay0 = s8(c1.z, 8) * dy, ay1 = s8(c1.w, 0) * dy;
    const float az0 = s8(c1.z, 16) * dz, az1 = s8(c1.w, 8) * dz;
    const float L = (fminf(ax0, ax1) + fminf(ay0, ay1)) + fminf(az0, az1);
    const float H = (fmaxf(ax0, ax1) + fmaxf(ay0, ay1)) + fmaxf(az0, az1);
    const float m = 0.127f * d1;  // 1e-3 |d|_1 in the same units
    const bool sign = (L > m) | (H < -m);
    const bool miss = block_slab_miss(bc_bits_float(c0.x), bc_bits_float(c0.y), bc_bits_float(c0.z), bc_bits_float(c0.w),
                                      bc_bits_float(c1.x), bc_bits_float(c1.y), ox, oy, oz, ix, iy, iz);
    return (miss ? 1u : 0u) | (sign ? 2u : 0u);
}
__host__ __device__ inline bool block_culls(uint4 c0, uint4 c1, float ox, float oy, float oz, float dx, float dy, float dz, float ix,
                                            float iy, float iz) {
    return (block_cull_parts(c0, c1, ox, oy, oz, dx, dy, dz, ix, iy, iz) == 3u) & !((c1.w >> 16) & BC_NEVER);
}

// ---- Packed cull record (DScene::ocull, one uint4 = 16 B per reference block; DESIGN.md 4.1 "Sign certificate per ray"):
//   x = lo.x | lo.y << 16   y = lo.z | hi.x << 16   z = hi.y | hi.z << 16   (bf16: the upper half of an f32)   w = flags
// The box is the f32 box of build_block_cull with lo rounded toward -inf and hi toward +inf, so it contains that box and
// parts (ii) / (iii) of the proof hold for it.  A never-cull block has the box [-inf, +inf], which no half-line misses (and
// keeps BC_NEVER in w for the host); a block without a real reference keeps an empty box.  The normal box is gone: that no
// norm . dir of the SCENE is zero is certified once per ray (ray_sign_certified), and only such a ray reads these records.
__host__ __device__ inline bool packed_block_miss(uint4 c, float ox, float oy, float oz, float ix, float iy, float iz) {
    return block_slab_miss(bc_bits_float(c.x << 16), bc_bits_float(c.x & 0xFFFF0000u), bc_bits_float(c.y << 16),
                           bc_bits_float(c.y & 0xFFFF0000u), bc_bits_float(c.z << 16), bc_bits_float(c.z & 0xFFFF0000u), ox, oy, oz, ix,
                           iy, iz);
}

// ---- Node cull (W_TRACE, DESIGN.md 4.1 "Node cull"; rtmi_debug_node_cull runs the same functions on the host).  DScene::fcull
// holds one packed record per inner box: the union of the f32 block boxes of every leaf list below the box, packed like a
// block's (lo toward -inf, hi toward +inf; a never-cull block below: [-inf, +inf]; no real reference below: the empty box).
// When the half-line of a certified ray misses that box (packed_block_miss, the predicate of the block cull), it misses
// every block box inside it, so every reference of the subtree fails the exact plane test and the subtree's walk ends
// without a hit: the SELECT step that first visits the box marks its frame done instead of choosing a child, which is the
// state that walk leaves behind.  The reference's collides() would have entered the box -- it walks boxes behind the
// origin too -- but nothing it does there reaches the result.
// The primary kernels of such a scene (k_path_primary*_cull, PNCULL below) do the same for primary rays and for the mirror
// reflections they trace in place: the camera is outside the scene, and most of the cubes a primary ray crosses hold
// nothing near it.  Their certificate has a band of its own (CERT_KAPPA_PRIMARY) and sits in bit 30 of `path`.

// ---- Sign certificate per ray (W_TRACE; rtmi_debug_ray_cert runs the same function on the host).  norm . dir belongs to the
// ray and the triangle, not to the block: rtmi_scene_create bins the scene's distinct normals by direction cell (a cube map
// folded by d -> -d, G x G cells per face; build_ray_cert), a cell lists every normal u with |u . d| <= tau |d|_1 for some d
// of the cell.  Table (words): G, first word of the index lists, first word of the normals, 1 = 32-bit indices (else 16-bit),
// then 3 G G + 1 list offsets.  A normal is (n.xyz as in the plane record, |n|_1).
#define CERT_TAU 1e-4     // an unlisted normal has |u . d| > tau |d|_1 for every direction of the cell
#define CERT_KAPPA 1e-6f  // a listed normal must have |den| > kappa |n|_1 |d|_1 (rounding of den: < 4e-7 of that product)
#define CERT_CAP 64u      // a longer list refuses the ray
// The band of k_path_primary's certificate (DESIGN.md 4.1 "Node cull for primary rays"): den of a listed normal is known bit
// for bit, so the band has nothing to absorb; it only has to keep t = num / den and every d_k * t finite, which any kappa
// above 6e-14 does.  The 64 samples of a pixel share a wave and a table cell: the wide band refuses one lane in every other
// pixel packet, and that lane then walks what the other 63 skip.
#ifndef CERT_KAPPA_PRIMARY  // (RTMI_DEVDEFS=-DCERT_KAPPA_PRIMARY=1e-6f builds the comparison of DESIGN.md 4.1)
#define CERT_KAPPA_PRIMARY 1e-9f
#endif
// The table cell of a direction that block_cull_ray() accepts
__host__ __device__ inline uint32_t ray_cert_cell(uint32_t G, float4 d) {
    const float ax = fabsf(d.x), ay = fabsf(d.y), az = fabsf(d.z);
    // the face of the largest component (a tie: either face lists what its border cells need), d / d_major = (1, a, b)
    const bool fx = (ax >= ay) & (ax >= az), fy = !fx & (ay >= az);
    const float dm = fx ? d.x : (fy ? d.y : d.z), da = fx ? d.y : (fy ? d.z : d.x), db = fx ? d.z : (fy ? d.x : d.y);
    const uint32_t face = fx ? 0u : (fy ? 1u : 2u);
    const float im = 1.f / dm, h = 0.5f * (float)G;
    const int gi = (int)((da * im + 1.f) * h), gj = (int)((db * im + 1.f) * h);
    const uint32_t i = (uint32_t)(gi < 0 ? 0 : (gi >= (int)G ? (int)G - 1 : gi)), j = (uint32_t)(gj < 0 ? 0 : (gj >= (int)G ? (int)G - 1 : gj));
    return (face * G + i) * G + j;
}
// How the list is walked (DESIGN.md 4.1 "Sign certificate per ray", the list walk).  The result is an AND of independent
// comparisons, so the batch size cannot change a bit of it; RTMI_DEVDEFS=-DCERT_BATCH=1 builds the comparison.
#ifndef CERT_BATCH  // entries of a list in flight together: their indices in one round trip, their normals in the next
#define CERT_BATCH 4  // (1: an entry at a time, two dependent round trips each; 8: k_trace_oct needs 92 VGPRs, 5 waves per SIMD)
#endif
// One listed normal against the ray: kd1 = kappa |d|_1, qd = 0 * d.w
__host__ __device__ __forceinline__ bool cert_entry_ok(float4 n, float4 d, float qd, float kd1) {
    const float den = (((0.f + n.x * d.x) + n.y * d.y) + n.z * d.z) + qd;  // `plane` of the LEAF step
    return fabsf(den) > n.w * kd1;
}
// Entries [beg, end) of the index lists, CERT_BATCH at a time.  A slot past the end of the list repeats the list's last
// entry: no index outside [beg, end) is read (the last list of the table ends where the index area ends), no normal is
// read through a word that is not an index, and testing an entry twice leaves the AND what it was.
template <bool WIDE>
__host__ __device__ __forceinline__ bool cert_walk(const uint32_t* __restrict__ cert, uint32_t beg, uint32_t end, float4 d, float qd, float kd1) {
    const uint32_t* const i32 = cert + cert[1];
    const uint16_t* const i16 = reinterpret_cast<const uint16_t*>(i32);
    const float4* const nrm = reinterpret_cast<const float4*>(cert + cert[2]);
    bool ok = true;
    // (left to itself hipcc vectorizes this loop 32 wide: k_trace_oct then needs 128 VGPRs and 1.2 KB of scratch)
#pragma clang loop vectorize(disable) interleave(disable) unroll(disable)
    for (uint32_t k = beg; k < end; k += CERT_BATCH) {
        uint32_t ix[CERT_BATCH];
        float4 n[CERT_BATCH];
#pragma unroll
        for (uint32_t j = 0; j < CERT_BATCH; j++) {
            const uint32_t kj = k + j < end ? k + j : end - 1u;
            ix[j] = WIDE ? i32[kj] : (uint32_t)i16[kj];
        }
#pragma unroll
        for (uint32_t j = 0; j < CERT_BATCH; j++) n[j] = nrm[ix[j]];
#pragma unroll
        for (uint32_t j = 0; j < CERT_BATCH; j++) ok &= cert_entry_ok(n[j], d, qd, kd1);
    }
    return ok;
}
// True: the ray may use the block cull -- block_cull_ray() accepts it and the plane test's den, evaluated here in the kernel's
// own operation order for every listed normal, is nonzero with margin; with the table's guarantee for the unlisted ones every
// triangle of the scene then has a nonzero den and a finite t for this ray.  *ncand <- length of the cell's list (host only).
__host__ __device__ __forceinline__ bool ray_sign_certified(const uint32_t* __restrict__ cert, float4 o, float4 d, uint32_t* ncand = nullptr,
                                                   float kappa = CERT_KAPPA) {
    if (ncand) *ncand = 0u;
    if (!block_cull_ray(o, d)) return false;
    const uint32_t cell = ray_cert_cell(cert[0], d);
    const uint32_t beg = cert[4u + cell], end = cert[5u + cell];
    if (ncand) *ncand = end - beg;
    if (end - beg > CERT_CAP) return false;
    const float kd1 = kappa * ((fabsf(d.x) + fabsf(d.y)) + fabsf(d.z));
    const float qd = 0.f * d.w;
    return cert[3] != 0u ? cert_walk<true>(cert, beg, end, d, qd, kd1) : cert_walk<false>(cert, beg, end, d, qd, kd1);
}
// The list walk as it was before the batches, an entry at a time: the referee of the walk above (rtmi_debug_ray_cert_ref,
// tests/test_ray_cert_walk_cpu.py).  Host only.
inline bool ray_sign_certified_ref(const uint32_t* cert, float4 o, float4 d, uint32_t* ncand = nullptr, float kappa = CERT_KAPPA) {
    if (ncand) *ncand = 0u;
    if (!block_cull_ray(o, d)) return false;
    const uint32_t cell = ray_cert_cell(cert[0], d);
    const uint32_t beg = cert[4u + cell], end = cert[5u + cell];
    if (ncand) *ncand = end - beg;
    if (end - beg > CERT_CAP) return false;
    const uint16_t* const i16 = reinterpret_cast<const uint16_t*>(cert + cert[1]);
    const uint32_t* const i32 = cert + cert[1];
    const float4* const nrm = reinterpret_cast<const float4*>(cert + cert[2]);
    const bool wide = cert[3] != 0u;
    const float kd1 = kappa * ((fabsf(d.x) + fabsf(d.y)) + fabsf(d.z));
    const float qd = 0.f * d.w;
    bool ok = true;
    for (uint32_t k = beg; k < end; k++) {
        const float4 n = nrm[wide ? i32[k] : (uint32_t)i16[k]];
        const float den = (((0.f + n.x * d.x) + n.y * d.y) + n.z * d.z) + qd;
        ok &= fabsf(den) > n.w * kd1;
    }
    return ok;
}

// (One read of the list per pixel packet -- the lanes of a wave that share a cell load an entry each and hand the normals
// round with v_readlane -- was built and measured: no gain, DESIGN.md 4.1.  Every lane walks its list.)
__device__ __attribute__((noinline)) bool primary_ray_certified(const uint32_t* cert, float4 o, float4 d) {
    return ray_sign_certified(cert, o, d, nullptr, CERT_KAPPA_PRIMARY);
}

// S: the batch's sampling mode (W_PRIMARY / W_SLOW; Samp::LIST takes the batch's pixels from `list`, path_pixel, shade.hpp;
// Samp::VIEWS each pixel's camera and seed from `vt`, pixel_key)
// PNCULL (W_PRIMARY): the node cull of the primary kernels (k_path_primary*_cull); false: the walk without it, instruction for
// instruction
// VIA (W_TRACE): the launch drains the fallback list of the hybrid pass `a.pass` (hybrid.hpp) instead of the pass's queue: `list`
// holds the queue indices of its rays, count and cursors are DCtrl::fbcount / fbhead, the result goes to the ray's own index, and
// the rays -- which the queue's launch counted -- are not added to "Rays".  false: the walk without it, instruction for instruction
template <bool COUNT, bool FAST, int MODE, Samp S = Samp::FRAME, bool PNCULL = false, bool VIA = false>
__device__ __forceinline__ void oct_walk(const DScene& sc, const OctArgs& a, DCtrl* __restrict__ ctrl, uint32_t* __restrict__ lds,
                                         int refill_min, int xcd_aware, const RecArgs& rec = RecArgs{},
                                         const uint32_t* __restrict__ list = nullptr, const ViewTab& vt = ViewTab{},
                                         const OcclArgs& oc = OcclArgs{}) {
    const int lane = threadIdx.x;  // one wave per block
    // rays from the queue of pass `a.pass`, closest hit to hit_tf / hit_t (W_RECORD is W_TRACE with a record per ray)
    // (W_OCCL is W_TRACE with a limit per ray and one byte out)
    constexpr bool QUEUE = MODE == W_TRACE || MODE == W_RECORD || MODE == W_OCCL;
    constexpr int NT = 64;
    // which queue of the control block this launch drains: W_TRACE pass `pass`, W_PRIMARY the implicit queue of all paths
    // of the batch (slot 0); W_SLOW does not use it (its launch drains a range of the slow-path queue)
    const int pass = QUEUE ? a.pass : 0;
    const uint32_t count = MODE == W_PRIMARY ? a.npaths : (MODE == W_SLOW ? ctrl->shi[a.slow_k] : (VIA ? ctrl->fbcount[pass] : ctrl->count[pass]));
    // "Rays": every queued ray of this launch (the slow path counts its rays one by one, below)
    if (MODE != W_SLOW && !VIA && blockIdx.x == 0 && lane == 0) atomicAdd(&ctrl->rays, (unsigned long long)count);
    const float4* __restrict__ qo = MODE == W_SLOW ? a.slow.o : a.qo;
    const float4* __restrict__ qd = MODE == W_SLOW ? a.slow.d : a.qd;
    if (MODE == W_SLOW) refill_min = 1;
    // W_PRIMARY / W_SLOW: the path this lane works for (slot of its sample colour); W_PRIMARY keeps the bounce (0, or 1 for
    // a mirror reflection traced in place) in bit 31 and, with the node cull, the ray's certificate in bit 30 -- a batch has
    // < 2^30 paths -- instead of in more loop-carried registers
    uint32_t path = 0;
    uint32_t bounce = 0;  // W_SLOW: bounces the path has behind it = the reference's maxdepth - depth of the ray being traced
    uint32_t ncont = 0;   // W_SLOW: rays this lane cast that no queue counted (the "Rays" statistic)
    unsigned long long cnt[5] = {0, 0, 0, 0, 0};
    // COUNT only: S steps, S lanes, L steps, L lanes, refills, refill lanes, edge steps, edge lanes, then shader-clock
    // cycles (s_memtime) this wave spent in SELECT steps, LEAF steps, refills, and in total
    // dbg[12..15]: leaf visits, leaf-memo hits, plane tests and edge tests the memo hits skipped
    // dbg[16..20] (W_PRIMARY): LEAF steps of the packet cull, all LEAF steps, references of those steps, references the
    // predicate culls, violations (a culled reference whose exact test passed: must stay 0)
    // dbg[21..23] (W_PRIMARY): primary rays whose path goes on through a Reflective hit (and not to the slow path), those
    // of them traced in place, exchange steps with >= 32 such lanes (low 32 bits) | with 64 such lanes (high 32 bits)
    // dbg[26..30] (W_TRACE, block cull): blocks seen by lanes with a qualifying ray, blocks whose box the half-line misses,
    // blocks culled, culled blocks that end their list, violations (a culled block with a reference whose exact test
    // passed: must stay 0); dbg[31..32]: rays k_trace_oct took with the cull on, those of them the certificate refused
    // dbg[24..25] (W_PRIMARY): leaf visits whose first LEAF step is a packet step (the whole-list cull starts at the list's
    // first block), whole-list culls (= the LEAF steps that the fast build spends on packet steps)
    // dbg[33..37] (W_TRACE, node cull): inner boxes a certified lane visits for the first time outside a missed subtree, those
    // whose node record the half-line misses, then what the fast build saves -- SELECT lane-steps and leaf visits inside a
    // missed subtree (the step that finds the miss not included) -- and violations (a hit taken inside a missed subtree:
    // must stay 0)
    // dbg[38..44] (W_PRIMARY, node cull, primary rays) and dbg[45..51] (the mirror reflections it traces in place): lanes
    // certified, lanes refused, then the five of dbg[33..37]
    unsigned long long dbg[RTMI_NDBG] = {};
    // COUNT, W_TRACE / W_PRIMARY: depth of the box at which the missed subtree this lane walks began (-1: it is in none)
    int mlvl = -1;
    // The node cull of W_PRIMARY (PNC_BIT of `path`: this lane's ray holds the certificate; a batch has < 2^30 paths)
    constexpr bool PNC = MODE == W_PRIMARY && PNCULL;
    constexpr uint32_t PNC_BIT = 0x40000000u;
    // (wave-uniform; read from the LDS header where it is used, not kept in a register since the kernel's start.  It is
    // never 0 in these kernels; the branches on it are kept because hipcc's register allocation is at its edge here: without
    // them the running best `gt` is spilled and reloaded inside the SELECT and LEAF steps)
    const uint32_t* const lds_hdr = lds;
    auto pnc_off = [&]() {
        return (uint32_t)__builtin_amdgcn_readfirstlane((int)reinterpret_cast<const volatile PrimHdr*>(lds_hdr)->foff);
    };
    auto pnc_count = [&](int k) { if (path >> 31) dbg[45 + k]++; else dbg[38 + k]++; };
    const unsigned long long t_begin = COUNT ? __builtin_amdgcn_s_memtime() : 0ull;
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    const float root_half = sc.root_half;
    const uint32_t inf_bits = 0x7F800000u;

    uint32_t mode = M_IDLE;
    bool exhausted = false;  // wave-uniform
    // HW_REG_XCC_ID (id 20, bits 3:0): which XCD this wave runs on; only a locality hint
    const uint32_t nranges = xcd_aware ? 8u : 1u;
    const uint32_t home = xcd_aware == 1 ? (__builtin_amdgcn_s_getreg((3 << 11) | 20) & 7u) : (blockIdx.x & 7u);
    uint32_t tries = 0;      // ranges this wave has seen exhausted (wave-uniform)
    RayK r = make_rayk(make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 1.f, 0.f));
    uint32_t ridx = 0;
    uint32_t fnode = 0, fw = 0;  // current frame
    float ft = 0.f;
    int lvl = 0;                 // depth of the current frame's box
    bool ghave = false;          // running best over the ray's leaf results
    float gt = 0.f;
    uint32_t gtf = 0;
    // W_RECORD: the lane's counters when it took its ray, and where its next leaf id goes
    uint32_t rc0[5] = {0, 0, 0, 0, 0};
    unsigned long long lcur = 0;
    uint32_t lblock = 0;
    bool lhave = false;
    float lt = 0.f;
    uint32_t ltf = 0;
    // W_OCCL: the ray's limit.  The exit test is on the ACCUMULATORS, never on the t of the triangle just tested: a NaN
    // accumulator sticks (`t < NaN` is false for every later hit, and a NaN running best blocks every later merge), so a
    // real hit found behind it must not answer 1.  `ghave && gt < tmx` is the running best; inside a leaf `lhave && lt <
    // tmx` answers early only when the merge at the leaf's end would take lt (no best yet, or lt < gt): lt only falls
    // from there on, so the merged best is < tmx too.  Boxes are NOT pruned by tmx (a triangle's hit point need not lie in
    // the leaf being scanned): the exit is the only thing this mode does less than the closest-hit walk.
    // A ray answered 1 is retired where the test passes: its byte is stored and its lane goes idle, to refill like one whose
    // walk ended.
    float tmx = 0.f;
    // One-entry leaf memo per lane, in LDS behind the frame stack ([word][lane], like the stack): the first block of the
    // last leaf list this lane's ray scanned (its identity: rtmi_scene_create stores each distinct list once), that list's
    // result (t, tri | face << 30, 0 = no hit: triangle 0 is never in a tree) and, COUNT only, its plane and edge tests.
    // A leaf whose first block equals the key takes the stored result instead of being scanned again: the leaf fold
    // (raytrace.rs:1012-1050) is a pure function of the ray and the list.  The key is invalidated whenever a lane takes a
    // new ray.  Not in the slow path (its wide LEAF step keeps the ray's state in lane 0).
    constexpr bool MEMO = MODE != W_SLOW;
    // W_PRIMARY: the packet of the last whole-wave refill (below) is wave-uniform and kept out of registers: it sits in the
    // LDS header (PrimHdr, a constant address), the frame stack and the memo behind it
    PrimHdr* const hdr = reinterpret_cast<PrimHdr*>(lds);
    Packet* const pkl = &hdr->pk;
    if (MODE == W_PRIMARY) {
        if (lane == 0) {
            hdr->q2[0] = (unsigned long long)a.b2qo; hdr->q2[1] = (unsigned long long)a.b2qd; hdr->q2[2] = (unsigned long long)a.b2qpath;
            hdr->minpl = a.minpl ? (uint32_t)a.minpl : 65u;
            if (PNC) {  // (launched only for scenes with node cull records, rtmi_device.hip launch_path)
                hdr->cert = (unsigned long long)sc.cert;
                hdr->foff = (uint32_t)(reinterpret_cast<const char*>(sc.fcull) - reinterpret_cast<const char*>(sc.fnodes));
            }
            if (COUNT) { hdr->llo = 0u; hdr->lhi = 0u; }
        }
        lds += sizeof(PrimHdr) / 4;
    }
    uint32_t* const memo = lds + sc.levels * 2 * NT + lane;
    // wave-uniform: PK_NEW = the lanes took new rays, the next LEAF step records their packet; PK_ON = LEAF steps may cull
    // against *pkl
    enum : uint32_t { PK_OFF = 0, PK_NEW = 1, PK_ON = 2 };
    uint32_t pk = PK_OFF;
    // W_TRACE (wave-uniform, a scalar pair): the lanes whose ray ray_sign_certified() accepts, updated where lanes take rays
    unsigned long long bcm = 0ull;
    auto take_leaf = [&](float t, uint32_t tf) {  // a finished leaf's hit into the frame and the running best
        if (COUNT && MODE == W_TRACE && mlvl >= 0) dbg[37]++;  // the node predicate was wrong: must never happen
        if (COUNT && PNC && mlvl >= 0) pnc_count(6);
        if (!(fw & O_HAS) || t < ft) ft = t;
        fw |= O_HAS;
        if (!ghave || t < gt) { gt = t; gtf = tf; }
        ghave = true;
    };

    for (;;) {
        const unsigned long long m_idle = __ballot(mode == M_IDLE);
        // lanes whose ray is finished and waits to be shaded (path kernels only)
        const unsigned long long m_shade = QUEUE ? 0ull : __ballot(mode == M_SHADE);
        // lanes the exchange step would serve (the slow path keeps one path per wave: only lane 0 ever takes a ray)
        const unsigned long long m_x = m_shade | (exhausted ? 0ull : (MODE == W_SLOW ? (m_idle & 1ull) : m_idle));
        if (QUEUE ? (m_idle == ~0ull && exhausted) : ((m_idle | m_shade) == ~0ull && m_x == 0ull)) break;
        if (m_x != 0ull && (__popcll(m_x) >= refill_min || (m_idle | m_shade) == ~0ull)) {
            // ---- exchange step: finished rays are shaded, lanes without a ray take consecutive queued rays
            const unsigned long long t_r0 = COUNT ? __builtin_amdgcn_s_memtime() : 0ull;
            bool start = false;     // this lane begins a new ray below
            bool inplace = false;   // W_PRIMARY (wave-uniform): this wave continues its mirror paths, no refill
            float4 no = make_float4(0.f, 0.f, 0.f, 0.f), nd = make_float4(0.f, 0.f, 1.f, 0.f);
            const uint32_t pth = MODE == W_PRIMARY ? path & (PNC ? PNC_BIT - 1u : 0x7FFFFFFFu) : path, bnc = MODE == W_PRIMARY ? path >> 31 : bounce;
            uint32_t npath = pth, nbounce = bnc;
            if (!QUEUE) {
                bool push = false;  // W_PRIMARY: the path goes on -> its bounce ray is queued for pass bounce + 1
                bool mirror = false;  // ... through a Reflective surface
                RayV nr;
                if (mode == M_SHADE) {
                    uint32_t prow, pcol, sample;
                    path_pixel<S>(a.v, a.pix0, pth, prow, pcol, sample, list);
                    const PixKey key = pixel_key<S>(a.v, prow, vt);  // (VIEWS: the view's row and seed; the other modes: prow, a.seed)
                    const bool cont = shade_hit(sc, a.v.maxdepth, key_seed<S>(key, vt, a.seed), a.npaths, pth, key.row * a.v.width + pcol, sample, bnc,
                                                ghave ? gtf : 0u, gt, V4{r.ox, r.oy, r.oz, r.ow}, V4{r.dx, r.dy, r.dz, r.dw},
                                                a.mstack, a.scol, nr, &mirror);
                    mode = M_IDLE;
                    if (cont) {
                        if (MODE == W_SLOW) {
                            no = make_float4(nr.orig.x, nr.orig.y, nr.orig.z, nr.orig.w);
                            nd = make_float4(nr.dir.x, nr.dir.y, nr.dir.z, nr.dir.w);
                            nbounce = bounce + 1u;
                            ncont++;
                            start = true;
                            mode = M_SELECT;  // (not idle: it keeps its lane)
                        } else push = true;
                    }
                }
                if (MODE == W_PRIMARY) {
                    if (push && a.slow.cap && has_zero_component(nr.dir.x, nr.dir.y, nr.dir.z) &&
                        slow_push(a.slow, ctrl, make_float4(nr.orig.x, nr.orig.y, nr.orig.z, nr.orig.w),
                                  make_float4(nr.dir.x, nr.dir.y, nr.dir.z, nr.dir.w), pth, bnc + 1u))
                        push = false;  // its path goes on in k_path_slow
                    // Mirror paths in place: the reflections of a pixel's primary rays off a mirror are as coherent as the
                    // primary rays themselves.  When at least a.minpl lanes have one, this wave traces them as bounce 1 (the
                    // packet of the next LEAF step is theirs) and takes no new primary rays until they are done; the other
                    // bounce rays go to queue 1 as always.  A reflection traced here is never continued here again: what
                    // follows it goes to queue 2, which nothing reads before pass 2 (queue 3 shares the buffer of queue 1,
                    // which pass 1 has still to read).
                    const volatile PrimHdr* const vh = hdr;  // (volatile: read here, not kept in registers since the kernel's start)
                    auto hword = [](uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); };
                    auto hptr = [&](int k) {
                        const unsigned long long v = vh->q2[k];
                        return (unsigned long long)hword((uint32_t)v) | ((unsigned long long)hword((uint32_t)(v >> 32)) << 32);
                    };
                    const unsigned long long mm = __ballot(push && mirror && bnc == 0u);
                    const uint32_t nm = (uint32_t)__popcll(mm);
                    inplace = nm != 0u && nm >= hword(vh->minpl);
                    if (COUNT && lane == 0) {
                        dbg[21] += nm;
                        dbg[22] += inplace ? nm : 0u;
                        dbg[23] += (nm >= 32u ? 1ull : 0ull) | (nm == 64u ? 1ull << 32 : 0ull);
                    }
                    if (inplace) {
                        if (lane == 0) atomicAdd(&ctrl->rays, (unsigned long long)nm);  // "Rays": no queue counts them
                        if ((mm >> lane) & 1ull) {
                            no = make_float4(nr.orig.x, nr.orig.y, nr.orig.z, nr.orig.w);
                            nd = make_float4(nr.dir.x, nr.dir.y, nr.dir.z, nr.dir.w);
                            nbounce = 1u;
                            start = true;
                            push = false;
                        }
                    }
                    // compaction into the queue of pass bounce + 1: ballot + prefix sum, one atomic per wave and queue
                    auto enqueue = [&](bool p, uint32_t* qcount, float4* bo, float4* bd, uint32_t* bp) {
                        const unsigned long long mask = __ballot(p);
                        if (mask) {
                            uint32_t qb = 0;
                            if (lane == 0) qb = atomicAdd(qcount, (uint32_t)__popcll(mask));
                            qb = __builtin_amdgcn_readfirstlane(qb);
                            if (p) {
                                const uint32_t slot = qb + (uint32_t)__popcll(mask & lt_mask);
                                store_stream(&bo[slot], make_float4(nr.orig.x, nr.orig.y, nr.orig.z, nr.orig.w));
                                store_stream(&bd[slot], make_float4(nr.dir.x, nr.dir.y, nr.dir.z, nr.dir.w));
                                store_stream(&bp[slot], pth);
                            }
                        }
                    };
                    enqueue(push && bnc == 0u, &ctrl->count[1], a.bqo, a.bqd, a.bqpath);
                    if (__ballot(push && bnc != 0u))
                        enqueue(push && bnc != 0u, &ctrl->count[2], reinterpret_cast<float4*>(hptr(0)), reinterpret_cast<float4*>(hptr(1)),
                                reinterpret_cast<uint32_t*>(hptr(2)));
                }
            }
            const unsigned long long m_want = QUEUE ? m_idle : (MODE == W_SLOW ? (__ballot(mode == M_IDLE) & 1ull) : __ballot(mode == M_IDLE));
            if (MODE == W_SLOW) {
                if (!exhausted && m_want != 0ull) {  // lane 0 takes the next entry of this launch's range
                    uint32_t i = 0;
                    if (lane == 0) i = ctrl->slo[a.slow_k] + atomicAdd(&ctrl->shead[a.slow_k], 1u);
                    i = __builtin_amdgcn_readfirstlane(i);
                    if (i >= count) exhausted = true;
                    else if (lane == 0) {
                        no = qo[i]; nd = qd[i];
                        npath = a.slow.path[i]; nbounce = a.slow.bounce[i];
                        ncont += nbounce != 0u ? 1u : 0u;  // a diverted bounce ray was not counted by any queue; a primary ray was
                        start = true;
                    }
                }
            } else
            if (!exhausted && m_want != 0ull && !inplace) {
                const uint32_t n = (uint32_t)__popcll(m_want);
                if (COUNT && lane == 0) { dbg[4]++; dbg[5] += n; }
                // XCD-aware work fetch: the queue is cut into 8 contiguous ranges, one per XCD (each XCD has its own
                // L2, so the waves of an XCD walk one image region and share its boxes/triangles there).  A wave pulls
                // from the range of the XCD it runs on and moves to the next range when that one is exhausted, so the
                // ranges only steer locality, never correctness or balance.
                uint32_t base = 0, hi = 0;
                for (;;) {
                    const uint32_t x = (home + tries) % nranges;
                    hi = (uint32_t)(((unsigned long long)count * (x + 1)) / nranges);
                    const uint32_t lo = (uint32_t)(((unsigned long long)count * x) / nranges);
                    if (lane == 0) base = lo + atomicAdd(VIA ? &ctrl->fbhead[pass][x] : &ctrl->xhead[pass][x], n);
                    base = __builtin_amdgcn_readfirstlane(base);
                    if (base < hi) break;
                    if (++tries == nranges) { exhausted = true; break; }
                }
                bool took = false;  // W_TRACE: this lane takes a queued ray here
                if (!exhausted && mode == M_IDLE) {
                    const uint32_t i = base + (uint32_t)__popcll(m_want & lt_mask);
                    if (i < hi) {
                        if (MODE == W_PRIMARY) {
                            uint32_t prow, pcol, sample;
                            path_pixel<S>(a.v, a.pix0, i, prow, pcol, sample, list);
                            const PixKey key = pixel_key<S>(a.v, prow, vt);
                            const RayV pr = pixel_ray<S>(a.v, key.row, pcol, key_seed<S>(key, vt, a.seed), key.row * a.v.width + pcol, sample,
                                                         S == Samp::VIEWS ? &vt.cams[key.view] : nullptr);
                            no = make_float4(pr.orig.x, pr.orig.y, pr.orig.z, pr.orig.w);
                            nd = make_float4(pr.dir.x, pr.dir.y, pr.dir.z, pr.dir.w);
                            npath = i; nbounce = 0u;
                            start = true;
                            // an exactly-zero direction component: ~150 x the work of an ordinary ray and the other 63
                            // samples of the pixel would wait for it -> its path is traced by k_path_slow
                            if (a.slow.cap && has_zero_component(nd.x, nd.y, nd.z) && slow_push(a.slow, ctrl, no, nd, i, 0u)) start = false;
                        } else {
                            ridx = VIA ? list[i] : i;
                            r = make_rayk(qo[ridx], qd[ridx]);
                            // the root box itself is never slab-tested (raytrace.rs:1272 calls
                            // get_object_intersection_for_ray on it directly): start with its frame
                            fnode = 0; fw = 0; ft = 0.f; lvl = 0;
                            ghave = false; gt = 0.f; gtf = 0;
                            if (MEMO) memo[0] = 0xFFFFFFFFu;  // no block index (< 2^28)
                            mode = M_SELECT;
                            took = true;
                            if (COUNT && MODE == W_TRACE) mlvl = -1;
                            if constexpr (MODE == W_OCCL) tmx = oc.tmax ? oc.tmax[i] : __uint_as_float(inf_bits);
                            if constexpr (MODE == W_RECORD) {  // this ray's counters start here; its leaf list at lfirst[i]
#pragma unroll
                                for (int k = 0; k < 5; k++) rc0[k] = (uint32_t)cnt[k];
                                lcur = rec.lids ? rec.lfirst[i] : 0ull;
                            }
                        }
                    }
                }
                if constexpr (MODE == W_TRACE) {
                    if (sc.ocull) {
                        const float4 co = make_float4(r.ox, r.oy, r.oz, r.ow), cd = make_float4(r.dx, r.dy, r.dz, r.dw);
                        const bool cb = took && (sc.cert ? ray_sign_certified(sc.cert, co, cd) : block_cull_ray(co, cd));
                        bcm = (bcm & ~__ballot(took)) | __ballot(cb);
                        if (COUNT) { dbg[31] += took ? 1u : 0u; dbg[32] += (took && !cb) ? 1u : 0u; }
                    }
                }
            }
            if (MODE == W_SLOW && __ballot(start) != 0ull) {
                // the slow path's one ray per wave (lane 0's) is held by EVERY lane: its leaves are scanned one reference
                // per lane (the wide LEAF step below)
                auto bc = [](float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); };
                const float4 bo = make_float4(bc(no.x), bc(no.y), bc(no.z), bc(no.w)), bd = make_float4(bc(nd.x), bc(nd.y), bc(nd.z), bc(nd.w));
                r = make_rayk(bo, bd);
            }
            if (MODE == W_PRIMARY) pk = a.pcull ? PK_NEW : PK_OFF;  // every refill of k_path_primary is whole-wave
            if (!QUEUE && start) {  // one place where a path kernel's lane takes a ray: bounce in place, or refill
                if (MODE != W_SLOW) r = make_rayk(no, nd);
                path = MODE == W_PRIMARY ? npath | (nbounce << 31) : npath; bounce = nbounce;
                if constexpr (PNC) {
                    // the certificate of this lane's ray (a primary ray, or a mirror reflection started in place), kept in a
                    // spare bit of `path`: no register of its own across the steps
                    if (pnc_off() != 0u) {
                        const uint32_t* const ct = reinterpret_cast<const uint32_t*>(reinterpret_cast<const volatile PrimHdr*>(lds_hdr)->cert);
                        const bool cb = primary_ray_certified(ct, make_float4(r.ox, r.oy, r.oz, r.ow), make_float4(r.dx, r.dy, r.dz, r.dw));
                        path |= cb ? PNC_BIT : 0u;
                        if (COUNT) { pnc_count(cb ? 0 : 1); mlvl = -1; }
                    }
                }
                fnode = 0; fw = 0; ft = 0.f; lvl = 0;
                ghave = false; gt = 0.f; gtf = 0;
                if (MEMO) memo[0] = 0xFFFFFFFFu;
                mode = M_SELECT;
            }
            if (COUNT && lane == 0) dbg[10] += __builtin_amdgcn_s_memtime() - t_r0;
            // no `continue`: the step below runs in the same iteration (one back edge, fewer copies of the loop-carried state)
        }
        // 32-bit counts: hipcc compares two popcountll results as 64-bit values, on the VALU
        const unsigned long long mS = __ballot(mode == M_SELECT), mL = __ballot(mode == M_LEAF);
        const int nS = __builtin_popcount((uint32_t)mS) + __builtin_popcount((uint32_t)(mS >> 32));
        const int nL = __builtin_popcount((uint32_t)mL) + __builtin_popcount((uint32_t)(mL >> 32));

        const unsigned long long t_s0 = COUNT ? __builtin_amdgcn_s_memtime() : 0ull;
        // Majority vote, weighted 3 : 2 towards SELECT: a LEAF step costs 1.7 x the instructions of a SELECT step, so it pays
        // to let a few more lanes gather for it (1:1 918, 3:2 925, 2:1 920, 2:3 905 Mrays/s);
        const bool stepS = nS * a.vote_s >= nL * a.vote_l;
        if (COUNT && lane == 0) { if (stepS) { dbg[0]++; dbg[1] += nS; } else { dbg[2]++; dbg[3] += nL; } }
        if (stepS) {  // hysteresis (stay in a phase until its lanes fall below 1/2..1/8 of the other's) measured 1-7 % slower
            // ================================================= SELECT step
            if (mode == M_SELECT) {
                // pop finished frames; the frames of depth 0 .. lvl-1 are in LDS levels 0 .. lvl-1
                while ((fw & O_DONE) && lvl != 0) {
                    const bool have = (fw & O_HAS) != 0;
                    const float ct = ft;
                    lvl--;
                    const uint32_t* fr = lds + lvl * 2 * NT + lane;
                    fnode = fr[0] & 0x3FFFFFu;
                    fw = fr[0] >> 22;
                    ft = __uint_as_float(fr[NT]);
                    if (have) {  // fold step of raytrace.rs:949-1007: first hit is taken, later ones replace iff strictly closer
                        if (!(fw & O_HAS) || ct < ft) ft = ct;
                        fw |= O_HAS;
                    }
                }
                if (COUNT && (MODE == W_TRACE || PNC) && lvl < mlvl) mlvl = -1;  // back above the box where the missed subtree began
                if (fw & O_DONE) {  // the root frame is finished: the ray is
                    if (QUEUE) {
                        if constexpr (MODE == W_RECORD) {
#pragma unroll
                            for (int k = 0; k < 5; k++) rec.rcnt[(size_t)ridx * 5u + k] = (uint32_t)cnt[k] - rc0[k];
                        }
                        if constexpr (MODE == W_OCCL) {
                            // the whole walk is behind the ray: the closest hit's t against the limit (a ray whose best
                            // went below it has retired before, so this is 0 but for what the definition says itself)
                            oc.occ[ridx] = (ghave && gt < tmx) ? (uint8_t)1 : (uint8_t)0;
                        } else {
                            a.hit_tf[ridx] = ghave ? gtf : 0u;
                            a.hit_t[ridx] = ghave ? gt : 0.f;
                        }
                        mode = M_IDLE;
                    } else mode = M_SHADE;  // shaded in the next exchange step, together with the other finished lanes
                } else {
                    const uint4 q0 = ld_off32(sc.fnodes, fnode << 5), q1 = ld_off32(sc.fnodes, (fnode << 5) + 16u);
                    // ---- node cull ("Node cull" above): the box's node record comes in the same round trip; a certified
                    // lane that visits the box for the first time and whose half-line misses the record's box ends the box
                    // here.  The counting build evaluates the same predicate, counts, and walks the subtree all the same.
                    bool ncut = false;
                    if constexpr (MODE == W_TRACE) {
                        if (sc.fcull) {
                            const uint4 nc = ld_off32(sc.fcull, fnode << 4);
                            const bool first = (((bcm >> lane) & 1ull) != 0ull) & ((fw & 0xFFu) == 0u);
                            const bool miss = first & packed_block_miss(nc, r.ox, r.oy, r.oz, r.ix, r.iy, r.iz);
                            if (COUNT) {
                                if (mlvl >= 0) dbg[35]++;
                                else if (first) {
                                    dbg[33]++;
                                    if (miss) { dbg[34]++; mlvl = lvl; }
                                }
                            } else ncut = miss;
                        }
                    }
                    // ... and the same for a certified lane of W_PRIMARY (the bit of `path`; CERT_KAPPA_PRIMARY).  The result is
                    // not carried to `ok` in a register of its own (k_path_primary has none to give): a missed box gets every
                    // octant marked visited, so the step finds no candidate, `ok` is false and the frame is done -- the visited
                    // bits of a finished frame are never read again.
                    if constexpr (PNC) {
                        const uint32_t foff = pnc_off();
                        if (foff != 0u) {
                            const uint4 nc = ld_off32(sc.fnodes, foff + (fnode << 4));
                            const bool first = ((path & PNC_BIT) != 0u) & ((fw & 0xFFu) == 0u);
                            const bool miss = first & packed_block_miss(nc, r.ox, r.oy, r.oz, r.ix, r.iy, r.iz);
                            if (COUNT) {
                                if (mlvl >= 0) pnc_count(4);
                                else if (first) {
                                    pnc_count(2);
                                    if (miss) { pnc_count(3); mlvl = lvl; }
                                }
                            } else fw |= miss ? 0xFFu : 0u;
                        }
                    }
                    const float cx = __uint_as_float(q0.x), cy = __uint_as_float(q0.y), cz = __uint_as_float(q0.z);
                    const float hc = ldexpf(root_half, -(lvl + 1));  // half edge of the children (depth lvl + 1)
                    if (COUNT && (fw & 0xFFu) == 0u) { cnt[0] += __popc(q0.w & 0xFFu); cnt[3]++; }  // first visit: collides() on every child
                    // candidate planes per axis (child centres: builder's orig.add(off_vec))
                    const float xl = cx + (-hc), xh = cx + hc, yl = cy + (-hc), yh = cy + hc, zl = cz + (-hc), zh = cz + hc;
                    // t1s = tmp1 - tmp2, t2s = tmp1 + tmp2 with tmp2 = inv_dir * len2 (raytrace.rs:866-870); near/far swap
                    // when inv_dir <= 0.  With b = |inv_dir| * len2 the pair is (a - b, a + b) in both cases, bit for
                    // bit: negation is exact and x + y == x - (-y).
                    const float bx = fabsf(r.ix) * hc, by = fabsf(r.iy) * hc, bz = fabsf(r.iz) * hc;
                    const float axl = (xl - r.ox) * r.ix, axh = (xh - r.ox) * r.ix;
                    const float ayl = (yl - r.oy) * r.iy, ayh = (yh - r.oy) * r.iy;
                    const float azl = (zl - r.oz) * r.iz, azh = (zh - r.oz) * r.iz;
                    float nx[2] = {axl - bx, axh - bx}, fx[2] = {axl + bx, axh + bx};
                    float ny[2] = {ayl - by, ayh - by}, fy[2] = {ayl + by, ayh + by};
                    float nz[2] = {azl - bz, azh - bz}, fz[2] = {azl + bz, azh + bz};
                    // a zero direction component skips its slab (raytrace.rs:872, :882, :892): axis 0 then leaves the
                    // initial (-MAX, MAX); for axes 1, 2 a NaN operand makes max3/min3 return the running value.
                    // Rare: whole waves skip this block.  (inv_dir = -inf with dir = -0 keeps the `inv > 0` choice
                    // of the reference because only |inv_dir| is used above.)
                    if (!(r.dx != 0.f) | !(r.dy != 0.f) | !(r.dz != 0.f)) {
                        if (!(r.dx != 0.f)) { nx[0] = nx[1] = -FLT_MAX; fx[0] = fx[1] = FLT_MAX; }
                        if (!(r.dy != 0.f)) { ny[0] = ny[1] = fy[0] = fy[1] = __uint_as_float(0x7FC00000u); }
                        if (!(r.dz != 0.f)) { nz[0] = nz[1] = fz[0] = fz[1] = __uint_as_float(0x7FC00000u); }
                    }
                    float tmv[8];
                    uint32_t hits = 0;
#pragma unroll
                    for (int o = 0; o < 8; o++) {
                        tmv[o] = max3f(nx[o & 1], ny[(o >> 1) & 1], nz[o >> 2]);
                        const float tmax = min3f(fx[o & 1], fy[(o >> 1) & 1], fz[o >> 2]);
                        // RTMI_OPT_FAST (off by default, NOT the reference's traversal): ignore boxes that lie entirely
                        // behind the ray origin.  The reference visits them (collides() has no `tmax > 0` test,
                        // raytrace.rs:902).
                        const bool c = FAST ? ((tmv[o] < tmax) & !(tmax < 0.f)) : (tmv[o] < tmax);
                        hits |= c ? (1u << o) : 0u;
                    }
                    // candidates: colliding, present, not visited yet
                    const uint32_t cand = hits & q0.w & ~fw & 0xFFu;
                    const uint32_t nh = (uint32_t)__popc(cand);
                    float tm[8];
#pragma unroll
                    for (int o = 0; o < 8; o++) {
                        const uint32_t ex = (uint32_t)__builtin_amdgcn_sbfe((int)cand, o, 1);
                        tm[o] = __uint_as_float((__float_as_uint(tmv[o]) & ex) | (inf_bits & ~ex));  // a colliding tmin is never NaN and never +inf
                    }
                    const float m1 = min3f(min3f(tm[0], tm[1], tm[2]), min3f(tm[3], tm[4], tm[5]), min3f(tm[6], tm[7], tm[7]));
                    // Next child of the sorted order = smallest tmin among the remaining ones, lowest index on ties
                    // (the insertion sort is stable).  Skip rule raytrace.rs:965: with a hit in this box only a child
                    // with tmin < best t is entered, and since the order is ascending and the best t never grows the
                    // first child that fails ends the box.  Without a hit yet a child whose tmin == f32::MAX is not
                    // entered (raytrace.rs:986; it looks like an empty boxmap slot) -- and then neither is any later
                    // one, because every remaining tmin is >= this one.
                    // One compare does all of that: without a candidate m1 is +inf, with one it is in [-MAX, MAX] (a
                    // colliding tmin is never NaN or +inf), where `!= MAX` is `< MAX`; and `inf < ft` is false for every ft.
                    const bool ok = (m1 < ((fw & O_HAS) ? ft : FLT_MAX)) & !ncut;  // (a culled box: nothing is selected, its frame is done)
                    uint32_t bit = 0u;
#pragma unroll
                    for (int o = 7; o >= 0; o--) bit = (tm[o] == m1) ? (1u << o) : bit;
                    if (!ok) {
                        fw |= O_DONE;
                    } else {
                        fw |= bit | (nh == 1u ? O_DONE : 0u);  // nothing remains after the last candidate
                        const uint32_t leafmask = (q0.w >> 8) & 0xFFu;
                        if (leafmask & bit) {
                            // first block of this leaf child: base + byte `octant` of the offsets
                            const uint32_t oct = (uint32_t)__ffs((int)bit) - 1u;
                            if constexpr (MODE == W_RECORD) {  // every leaf entered, a leaf-memo hit included (its list counts again)
                                if (rec.lids && lcur < rec.lcap) rec.lids[lcur] = (fnode << 3) | oct;
                                lcur++;
                            }
                            if (q0.w & FN_WIDE) lblock = sc.wlinks[(size_t)q1.y * 8u + oct];  // rare: explicit indices
                            else lblock = q1.y + __builtin_amdgcn_ubfe(oct < 4u ? q1.z : q1.w, (oct & 3u) * 8u, 8u);
                            if (COUNT) cnt[4]++;
                            if (COUNT && MEMO) dbg[12]++;
                            if (COUNT && MODE == W_TRACE && mlvl >= 0) dbg[36]++;
                            if (COUNT && PNC && mlvl >= 0) pnc_count(5);
                            if (MEMO && memo[0] == lblock) {  // the list this ray scanned last: its result, no LEAF steps
                                const uint32_t mtf = memo[2 * NT];
                                if (mtf != 0u) take_leaf(__uint_as_float(memo[NT]), mtf);
                                // (the exit test after the merge, as everywhere; a reused result cannot pass it, since the
                                // scan that stored it would have)
                                if constexpr (MODE == W_OCCL) {
                                    if (ghave && gt < tmx) { oc.occ[ridx] = (uint8_t)1; mode = M_IDLE; }
                                }
                                if (COUNT) {
                                    const uint32_t np = memo[3 * NT], ne = memo[4 * NT];
                                    cnt[1] += np; cnt[2] += ne;
                                    dbg[13]++; dbg[14] += np; dbg[15] += ne;
                                }
                            } else {
                                if (MEMO) {
                                    memo[0] = lblock;
                                    if (COUNT) { memo[3 * NT] = (uint32_t)cnt[1]; memo[4 * NT] = (uint32_t)cnt[2]; }
                                }
                                lhave = false;  // lt, ltf are dead until the first hit of the leaf sets them
                                mode = M_LEAF;
                            }
                        } else {
                            uint32_t* fr = lds + lvl * 2 * NT + lane;
                            fr[0] = fnode | (fw << 22);  // record index (< 2^22, checked at scene creation) | visited bits, DONE, HAS
                            fr[NT] = __float_as_uint(ft);
                            lvl++;
                            // record of this inner child: the inner children before it in octant order
                            fnode = q1.x + (uint32_t)__popc((q0.w & ~leafmask & 0xFFu) & (bit - 1u));
                            fw = 0u; ft = 0.f;
                        }
                    }
                }
            }
        }
        // (a second `if`, not an `else`: hipcc's CFG structurizer then has two plain if-regions to handle instead of an
        // if/else whose join needs copies of every loop-carried register written on either side -- 25 fewer v_mov per iteration,
        // what round 2 got from an LLVM-internal switch that later miscompiled this loop, csrc/Makefile)
        if (!stepS) {
            // ================================================= LEAF step: one block of <= 4 references
            if (MODE == W_SLOW) {
                // ---- wide LEAF step of the slow path: the wave holds ONE ray (lane 0 owns its state, every lane has a copy
                // of the ray), so the leaf is scanned one REFERENCE per lane, 16 blocks per step, and the reference's
                // sequential fold (get_box_min_time_intersection, raytrace.rs:1012-1050: the first hit is taken, a later
                // one replaces it iff strictly closer) is replayed over the hits in list order on the scalar unit.
                const uint32_t lb0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)lblock);
                const uint32_t myb = lb0 + ((uint32_t)lane >> 2);
                const bool inb = myb < sc.noblocks;
                const uint4 blk = inb ? ld_off32(sc.oblocks, myb << 4) : make_uint4(0u, 0u, 0u, 0u);
                const uint32_t cpos = (uint32_t)lane & 3u;
                const uint32_t id = (cpos == 0u ? blk.x : cpos == 1u ? blk.y : cpos == 2u ? blk.z : blk.w) & 0x7FFFFFFFu;
                const bool term = blk.w == 0u || (blk.w >> 31);            // this block ends the list (a block past the array does too)
                const unsigned long long tm = __ballot(term);
                const uint32_t endb = tm ? ((uint32_t)(__ffsll((long long)tm) - 1) >> 2) : 16u;  // first terminating block of the 16
                const bool valid = (((uint32_t)lane >> 2) <= endb) & (id != 0u);              // a 0 is padding behind the list's end
                float t = 0.f;
                uint32_t face = 0u;
                bool hit = false;
                if (valid) hit = tri_test<COUNT>(sc, id, r, t, face, cnt);
                bool have = __builtin_amdgcn_readfirstlane((int)lhave) != 0;
                float best = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(lt)));
                uint32_t btf = (uint32_t)__builtin_amdgcn_readfirstlane((int)ltf);
                const uint32_t mytf = id | (face << 30);
                for (unsigned long long hm = __ballot(hit); hm; hm &= hm - 1ull) {
                    const int l = __ffsll((long long)hm) - 1;
                    const float tl = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(t), l));
                    if (!have || tl < best) { best = tl; btf = (uint32_t)__builtin_amdgcn_readlane((int)mytf, l); }
                    have = true;
                }
                if (lane == 0) {
                    lhave = have; lt = best; ltf = btf;
                    if (tm == 0ull) lblock = lb0 + 16u;  // no end among these 16 blocks: the list goes on
                    else {
                        if (lhave) take_leaf(lt, ltf);
                        mode = M_SELECT;
                    }
                }
            } else {
            // ---- packet cull (W_PRIMARY, DESIGN.md 4.1 "Packet cull"): when every LEAF lane stands at the same block lb0, ONE
            // step culls the list from lb0 on against the packet.  Lane i takes reference i & 3 of block lb0 + (i >> 2) (the
            // addressing and end rule of the slow path's wide step below) and tests it with packet_culls; one ballot gives the
            // references that survive, and they get the exact test one at a time, in list order, in the same step.  A list of
            // <= 16 blocks thus costs one LEAF step, culled whole or not; a longer one goes on at block lb0 + 16 with the next
            // step.  The full LEAF step runs when the lanes stand at different blocks.  The counting build evaluates the same
            // mask, keeps it in the LDS header and tests every reference block by block, checking each one the mask culls.
            uint32_t cullm = 0u;  // COUNT (wave-uniform): the references of this block that the list mask culls
            if (MODE == W_PRIMARY && __builtin_amdgcn_readfirstlane((int)pk) == (int)PK_NEW) {
                // the packet of the last refill: the rays of every lane that has one (in W_PRIMARY a lane's ray only changes
                // at a refill, so r still holds it; lanes whose ray went to the slow path are idle and do not count)
                pk = PK_OFF;
                const unsigned long long mr = __ballot(mode != M_IDLE);
                const int l0 = __ffsll((long long)mr) - 1;
                auto rl = [&](float v) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l0)); };
                Packet p;
                p.ox = rl(r.ox); p.oy = rl(r.oy); p.oz = rl(r.oz);
                p.dx = rl(r.dx); p.dy = rl(r.dy); p.dz = rl(r.dz);
                float so = 0.f, sd = 0.f;
                bool ok = true;
                if (mode != M_IDLE) ok = packet_spread(p, make_float4(r.ox, r.oy, r.oz, r.ow), make_float4(r.dx, r.dy, r.dz, r.dw), so, sd);
                if (__ballot(!ok) == 0ull) {
                    // wave maxima (non-negative finite floats order like their bit patterns)
                    uint32_t mo = __float_as_uint(so), md = __float_as_uint(sd);
#pragma unroll
                    for (int k = 1; k < NT; k <<= 1) {
                        mo = max(mo, (uint32_t)__shfl_xor((int)mo, k));
                        md = max(md, (uint32_t)__shfl_xor((int)md, k));
                    }
                    if (packet_finish(p, __uint_as_float(__builtin_amdgcn_readfirstlane(mo)), __uint_as_float(__builtin_amdgcn_readfirstlane(md)))) {
                        pk = PK_ON;
                        if (lane == 0) {
                            *pkl = p;
                            if (COUNT) { hdr->llo = 0u; hdr->lhi = 0u; }  // a list mask of the previous packet covers nothing
                        }
                    }
                }
            }
            auto finish_leaf = [&]() {  // the list ended with this block
                if (lhave) take_leaf(lt, ltf);
                if (MEMO) {  // the key was written at leaf entry
                    memo[NT] = __float_as_uint(lt);
                    memo[2 * NT] = MODE == W_OCCL ? (lhave ? 1u : 0u) : (lhave ? ltf : 0u);  // (W_OCCL keeps no hit index)
                    if (COUNT) { memo[3 * NT] = (uint32_t)cnt[1] - memo[3 * NT]; memo[4 * NT] = (uint32_t)cnt[2] - memo[4 * NT]; }
                }
                mode = M_SELECT;
            };
            // Triangle::intersects (raytrace.rs:400-439), plane part for the 4 references, branch-free (a
            // padding index 0 reads the sentinel's record and is masked out); see tri_test() for the lane-3
            // terms.  A reference that passes `t >= 0` and the bounding-radius test becomes the lane's pending
            // candidate; its edge part runs below, once per step.
            struct Cand { uint32_t tri; float t, ix, iy, iz, den; };  // a lane's pending candidate (tri 0: none)
            auto resolve = [&](const Cand& q) {
                // all four edge records are requested together and every comparison is evaluated (no
                // short-circuit): one memory round trip instead of three
                if (COUNT) { cnt[2]++; const unsigned long long em = __ballot(true); if (lane == __ffsll((long long)em) - 1) { dbg[6]++; dbg[7] += __popcll(em); } }
                const uint32_t eo = q.tri << 6;
                const float4 e0 = ld_off32(sc.tedge, eo), e1 = ld_off32(sc.tedge, eo + 16u), e2 = ld_off32(sc.tedge, eo + 32u), e3 = ld_off32(sc.tedge, eo + 48u);
                const float pz = (r.dw * q.t + r.ow) * 0.f;  // lane-3 product ip.w * side.w (side.w is +-0); ip.w as the plane part computed it
                const float d0 = ((q.ix * e0.x + q.iy * e0.y) + q.iz * e0.z) + pz;
                const float d1 = ((q.ix * e1.x + q.iy * e1.y) + q.iz * e1.z) + pz;
                const float d2 = ((q.ix * e2.x + q.iy * e2.y) + q.iz * e2.z) + pz;
                const bool inside = !(d0 > e0.w) & !(d1 > e1.w) & !(d2 > e2.w);
                const bool edge = (d0 > e3.x) | (d1 > e3.y) | (d2 > e3.z);
                const uint32_t face = (q.den > 0.f ? 1u : 0u) | (edge ? 2u : 0u);  // back face: norm . dir > 0
                const bool take = inside & (!lhave | (q.t < lt));  // raytrace.rs:1028-1038
                lt = take ? q.t : lt;
                ltf = take ? (q.tri | (face << 30)) : ltf;
                lhave = lhave | inside;
            };
            auto plane = [&](Cand& q, uint32_t id, const float4& a0, const float4& a1, bool culled) {
                const float ax = a0.x - r.ox, ay = a0.y - r.oy, az = a0.z - r.oz;
                const float num = (((0.f + a1.x * ax) + a1.y * ay) + a1.z * az) + r.qn;
                const float den = (((0.f + a1.x * r.dx) + a1.y * r.dy) + a1.z * r.dz) + r.qd;
                const float t = num / den;
                const float px = r.dx * t + r.ox, py = r.dy * t + r.oy, pz_ = r.dz * t + r.oz, pw = r.dw * t + r.ow;
                const float ix = px - a0.x, iy = py - a0.y, iz = pz_ - a0.z;
                const float l2 = ((ix * ix + iy * iy) + iz * iz) + pw * pw;
                const bool real = id != 0u;
                if (COUNT) cnt[1] += real ? 1u : 0u;
                const bool c = real & !(t < 0.f) & !(l2 > a0.w);
                if (COUNT && c && culled) dbg[MODE == W_TRACE ? 30 : 20]++;  // the packet (block) predicate was wrong: must never happen
                if (c & (q.tri != 0u)) resolve(q);  // second candidate of this lane in one block: rare
                q.tri = c ? id : q.tri;
                q.t = c ? t : q.t;
                q.ix = c ? ix : q.ix; q.iy = c ? iy : q.iy; q.iz = c ? iz : q.iz;
                q.den = c ? den : q.den;
            };
            // ---- block cull (W_TRACE, DESIGN.md 4.1 "Block cull"): a lane whose ray qualifies reads the cull record of its
            // block first and skips the block when the half-line misses its box (packed_block_miss; the ray is certified, so
            // the miss rejects the block's references), up to a.bcn blocks per step (the sweep of the count is in DESIGN.md).
            // A culled block that ends its list finishes the leaf like the full step does
            // (lhave of earlier blocks is kept, the memo entry is written).  The counting build evaluates the predicate for
            // the block of the full step and still tests every reference.
            bool bcut = false;  // COUNT: the predicate culls this lane's block
            if constexpr (MODE == W_TRACE) {
                if (sc.ocull) {
                    const bool cl = (mode == M_LEAF) & (((bcm >> lane) & 1ull) != 0ull);
                    if (COUNT) {
                        if (cl && sc.cert) {
                            const uint4 c = ld_off32(sc.ocull, lblock << 4);
                            bcut = packed_block_miss(c, r.ox, r.oy, r.oz, r.ix, r.iy, r.iz);
                            // (a never-cull block has an infinite box: "box missed" and "culled" are one count here)
                            dbg[26]++; dbg[27] += bcut ? 1u : 0u; dbg[28] += bcut ? 1u : 0u;
                            dbg[29] += (bcut && (c.w & BC_END)) ? 1u : 0u;
                        } else if (cl) {
                            const uint4 c0 = ld_off32(sc.ocull, lblock << 5), c1 = ld_off32(sc.ocull, (lblock << 5) + 16u);
                            const uint32_t parts = block_cull_parts(c0, c1, r.ox, r.oy, r.oz, r.dx, r.dy, r.dz, r.ix, r.iy, r.iz);
                            bcut = block_culls(c0, c1, r.ox, r.oy, r.oz, r.dx, r.dy, r.dz, r.ix, r.iy, r.iz);
                            dbg[26]++; dbg[27] += parts & 1u; dbg[28] += bcut ? 1u : 0u;
                            dbg[29] += (bcut && ((c1.w >> 16) & BC_END)) ? 1u : 0u;
                        }
                    } else if (sc.cert) {
                        // this block's record and the next ones' in one round trip, a.bcn of them (2..4, wave-uniform): the
                        // lane skips blocks while they are culled and the list goes on (a later record only counts when
                        // every block before it is culled and none of them ends the list; behind the array's last record
                        // lie three zero ones)
                        bool bfin = false;
                        if (cl) {
                            const uint32_t off = lblock << 4;
                            const uint4 z = make_uint4(0u, 0u, 0u, 0u);
                            const uint4 c0 = ld_off32(sc.ocull, off), c1 = ld_off32(sc.ocull, off + 16u);
                            const uint4 c2 = a.bcn > 2 ? ld_off32(sc.ocull, off + 32u) : z, c3 = a.bcn > 3 ? ld_off32(sc.ocull, off + 48u) : z;
                            const uint4 cs[4] = {c0, c1, c2, c3};
                            bool go = true;
                            uint32_t adv = 0u;
#pragma unroll
                            for (int k = 0; k < 4; k++) {
                                const bool cut = (k < a.bcn) & packed_block_miss(cs[k], r.ox, r.oy, r.oz, r.ix, r.iy, r.iz);
                                const bool end = (cs[k].w & BC_END) != 0u;
                                bfin = bfin | (go & cut & end);
                                go = go & cut & !end;
                                adv += go ? 1u : 0u;
                            }
                            lblock += adv;
                        }
                        if (bfin) finish_leaf();
                    } else {
                        // a scene without a direction table (too many distinct normals, rtmi_scene_create): the 32-B records
                        // with their normal box, this block's and the next one's in one round trip
                        bool bfin = false;
                        if (cl) {
                            const uint4 c0 = ld_off32(sc.ocull, lblock << 5), c1 = ld_off32(sc.ocull, (lblock << 5) + 16u);
                            const uint4 e0 = ld_off32(sc.ocull, (lblock << 5) + 32u), e1 = ld_off32(sc.ocull, (lblock << 5) + 48u);
                            const bool cutA = block_culls(c0, c1, r.ox, r.oy, r.oz, r.dx, r.dy, r.dz, r.ix, r.iy, r.iz);
                            const bool cutB = block_culls(e0, e1, r.ox, r.oy, r.oz, r.dx, r.dy, r.dz, r.ix, r.iy, r.iz);
                            const bool endA = ((c1.w >> 16) & BC_END) != 0u, endB = ((e1.w >> 16) & BC_END) != 0u;
                            const bool goA = cutA & !endA, goB = goA & cutB & !endB;
                            bfin = (cutA & endA) | (goA & cutB & endB);
                            lblock += (goA ? 1u : 0u) + (goB ? 1u : 0u);
                        }
                        if (bfin) finish_leaf();
                    }
                }
            }
            bool lm = mode == M_LEAF;  // this lane runs the full LEAF step below
            const uint32_t* const oref = reinterpret_cast<const uint32_t*>(sc.oblocks);  // the references one word at a time
            bool fin = false;          // W_PRIMARY: this lane's list ended in this step
            bool wl = false;           // (wave-uniform) the whole-list step runs: its survivors and blocks are in the LDS header
            if (MODE == W_PRIMARY && __builtin_amdgcn_readfirstlane((int)pk) == (int)PK_ON) {
                const int l0 = __ffsll((long long)mL) - 1;
                const uint32_t lb0 = (uint32_t)__builtin_amdgcn_readlane((int)lblock, l0);
                if (__ballot((mode == M_LEAF) & (lblock != lb0)) == 0ull) {
                    auto rf = [](uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); };
                    const volatile PrimHdr* const vh = hdr;
                    // counting build: a block that the last list mask covers (past the block it started at) is not culled again
                    if (!COUNT || !(lb0 > rf(vh->llo) && lb0 < rf(vh->lhi))) {
                        // the lane's number, computed here: hipcc would otherwise keep lane >> 2, lane & 3 live over the whole loop
                        // (and counted, not copied from `lane`: a register the walk gives up elsewhere must not come back
                        // from scratch in this step)
                        uint32_t ln;
                        if constexpr (PNC) asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(ln));
                        else asm volatile("v_mov_b32 %0, %1" : "=v"(ln) : "v"(lane));
                        // one word per lane (the array has 15 zero blocks behind its last one: no bounds test)
                        const uint32_t w = ld_off32(oref, ((lb0 + (ln >> 2)) << 4) + ((ln & 3u) << 2));
                        const uint32_t id = w & 0x7FFFFFFFu;
                        // blocks that end the list: their 4th word (lane 4 j + 3) is 0 or has bit 31 set
                        const unsigned long long tm = __ballot(((ln & 3u) == 3u) & ((w == 0u) | ((w >> 31) != 0u)));
                        const uint32_t nb = tm ? ((uint32_t)(__ffsll((long long)tm) - 1) >> 2) + 1u : 16u;  // blocks of the list from lb0, <= 16
                        const bool inl = ((ln >> 2) < nb) & (id != 0u);  // a 0 is padding behind the list's end
                        const uint32_t pid = inl ? id : 0u;               // (the others read the sentinel's record: one line)
                        const float4 q0 = ld_off32(sc.tplane, pid << 5), q1 = ld_off32(sc.tplane, (pid << 5) + 16u);
                        const bool cut = packet_culls(*pkl, q0, q1);
                        if (!COUNT) {
                            wl = true;
                            const unsigned long long sm = __ballot(inl & !cut);  // the survivors, in list order
                            if (lane == 0) { hdr->lmask = sm; hdr->llo = lb0; hdr->lhi = (lb0 + nb) | (tm != 0ull ? 0x80000000u : 0u); }
                        } else {
                            const unsigned long long cm = __ballot(inl & cut);
                            const uint32_t key = (uint32_t)__builtin_amdgcn_readlane((int)memo[0], l0);  // the list's first block
                            if (lane == 0) {
                                hdr->lmask = cm; hdr->llo = lb0; hdr->lhi = lb0 + nb;
                                dbg[25]++;
                                if (lb0 == key) dbg[24]++;
                            }
                        }
                    }
                    if (COUNT) {  // this block's part of the mask; the full step below tests all 4 references
                        const uint32_t lo = rf(vh->llo);
                        const unsigned long long cm = vh->lmask;
                        cullm = (uint32_t)(((unsigned long long)rf((uint32_t)cm) | ((unsigned long long)rf((uint32_t)(cm >> 32)) << 32)) >> ((lb0 - lo) * 4u)) & 0xFu;
                        const uint4 b = ld_off32(sc.oblocks, lb0 << 4);
                        if (lane == 0) {
                            const uint32_t real = (b.x != 0u ? 1u : 0u) | (b.y != 0u ? 2u : 0u) | (b.z != 0u ? 4u : 0u) | ((b.w & 0x7FFFFFFFu) != 0u ? 8u : 0u);
                            dbg[16]++; dbg[18] += __popc(real); dbg[19] += __popc(real & cullm);
                        }
                    }
                }
                if (COUNT && lane == 0) dbg[17]++;
            }
            if (!COUNT && wl) {
                // the whole-list step's survivors: a region of its own, apart from the full step (uniform
                // branches around the full step's plane tests make hipcc spill)
                if (lm) {
                    auto rf = [](uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); };
                    const volatile PrimHdr* const vh = hdr;
                    const unsigned long long sm = vh->lmask;
                    const uint32_t lo = rf(vh->llo), hi = rf(vh->lhi);
                    Cand q{0u, 0.f, 0.f, 0.f, 0.f, 0.f};
                    // one reference at a time, in list order (a wave-uniform loop): reference l & 3 of block lo + (l >> 2)
                    for (unsigned long long m = (unsigned long long)rf((uint32_t)sm) | ((unsigned long long)rf((uint32_t)(sm >> 32)) << 32); m != 0ull; m &= m - 1ull) {
                        const uint32_t l = (uint32_t)(__ffsll((long long)m) - 1);
                        const uint32_t sid = rf(ld_off32(oref, ((lo + (l >> 2)) << 4) + ((l & 3u) << 2)) & 0x7FFFFFFFu);
                        plane(q, sid, ld_off32(sc.tplane, sid << 5), ld_off32(sc.tplane, (sid << 5) + 16u), false);
                    }
                    if (q.tri != 0u) resolve(q);
                    if (hi >> 31) fin = true;
                    else lblock = hi;  // no end among these 16 blocks: the list goes on
                }
                lm = false;
            }
            if (lm) {
                const uint4 blk = ld_off32(sc.oblocks, lblock << 4);
                const uint32_t ids[4] = {blk.x, blk.y, blk.z, blk.w & 0x7FFFFFFFu};
                float4 p0[4], p1[4];
#pragma unroll
                for (int k = 0; k < 4; k++) { p0[k] = ld_off32(sc.tplane, ids[k] << 5); p1[k] = ld_off32(sc.tplane, (ids[k] << 5) + 16u); }
                const bool more = blk.w != 0u && !(blk.w >> 31);  // bit 31 of the 4th index: this full block is the last
                if (more) lblock++;
                Cand q{0u, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int k = 0; k < 4; k++) plane(q, ids[k], p0[k], p1[k], MODE == W_TRACE ? bcut : (bool)((cullm >> k) & 1u));
                if (q.tri != 0u) resolve(q);
                // (W_PRIMARY: one call of finish_leaf after both steps; the other modes keep it here, their code unchanged)
                if constexpr (MODE == W_OCCL) {  // the any-hit exit, mid-list or at its end
                    if (lhave && lt < tmx && (!ghave || lt < gt)) { oc.occ[ridx] = (uint8_t)1; mode = M_IDLE; }
                    else if (!more) finish_leaf();
                } else {
                if (MODE == W_PRIMARY) fin = !more;
                else if (!more) finish_leaf();
                }
            }
            if (MODE == W_PRIMARY && fin) finish_leaf();
            }
        }
        if (COUNT && lane == 0) {  // the step is over for the wave when its slowest lane is (s_memtime is a scalar read)
            const unsigned long long dt = __builtin_amdgcn_s_memtime() - t_s0;
            if (stepS) dbg[8] += dt; else dbg[9] += dt;
        }
    }
    if (MODE == W_SLOW) {  // "Rays": the rays this launch cast that no queue counted
        unsigned long long wsum = 0;
        for (unsigned long long m = __ballot(ncont != 0u); m; m &= m - 1ull)
            wsum += (uint32_t)__builtin_amdgcn_readlane((int)ncont, __ffsll((long long)m) - 1);
        if (lane == 0 && wsum) atomicAdd(&ctrl->rays, wsum);
    }
    if (COUNT) {
        if (lane == 0) dbg[11] = __builtin_amdgcn_s_memtime() - t_begin;
#pragma unroll
        for (int k = 0; k < 5; k++)
            if (cnt[k]) atomicAdd(&ctrl->counters[k], cnt[k]);
#pragma unroll
        for (int k = 0; k < RTMI_NDBG; k++)
            if (dbg[k]) atomicAdd(&ctrl->dbg[k], dbg[k]);
    }
}

#ifndef RTMI_TRACE_WAVES
#define RTMI_TRACE_WAVES 4
#endif
template <bool COUNT, bool FAST>
__global__ void __launch_bounds__(64, RTMI_TRACE_WAVES) k_trace_oct(DScene sc, OctArgs a, DCtrl* __restrict__ ctrl, int refill_min, int xcd_aware) {
    extern __shared__ uint32_t lds[];
    oct_walk<COUNT, FAST, W_TRACE>(sc, a, ctrl, lds, refill_min, xcd_aware);
}
// The exact walk over the fallback list of a hybrid pass (hybrid.hpp): k_trace_oct's walk, its rays taken through `list`
__global__ void __launch_bounds__(64, RTMI_TRACE_WAVES) k_trace_oct_list(DScene sc, OctArgs a, DCtrl* __restrict__ ctrl, int refill_min, int xcd_aware,
                                                                         const uint32_t* __restrict__ list) {
    extern __shared__ uint32_t lds[];
    oct_walk<false, false, W_TRACE, Samp::FRAME, false, true>(sc, a, ctrl, lds, refill_min, xcd_aware, RecArgs{}, list);
}
// 6 waves per SIMD = at most 80 VGPRs, the occupancy k_trace_oct has (24 waves per CU is where this walk peaks, DESIGN.md
// 4.1).  The exchange step (Philox + shading with the whole traversal state live) needs ~95; with the cap hipcc keeps the
// SELECT / LEAF steps spill-free and parks launch constants in scratch that only the (rare) exchange step reloads.
#ifndef RTMI_PATH_WAVES
#define RTMI_PATH_WAVES 6
#endif
// Any-hit occlusion (rtmi_occluded*): k_trace_oct's launch with a limit per ray and one byte out
template <bool COUNT, bool FAST>
__global__ void __launch_bounds__(64, RTMI_TRACE_WAVES) k_occluded_oct(DScene sc, OctArgs a, DCtrl* __restrict__ ctrl, int refill_min, int xcd_aware,
                                                                       OcclArgs oc) {
    extern __shared__ uint32_t lds[];
    oct_walk<COUNT, FAST, W_OCCL>(sc, a, ctrl, lds, refill_min, xcd_aware, RecArgs{}, nullptr, ViewTab{}, oc);
}
// Per-ray records of the exact walk (rtmi_trace_records / rtmi_primary_records): k_trace_oct<true, false> plus RecArgs
__global__ void __launch_bounds__(64, RTMI_TRACE_WAVES) k_trace_record(DScene sc, OctArgs a, DCtrl* __restrict__ ctrl, int refill_min, int xcd_aware,
                                                                       RecArgs rec) {
    extern __shared__ uint32_t lds[];
    oct_walk<true, false, W_RECORD>(sc, a, ctrl, lds, refill_min, xcd_aware, rec);
}
template <bool COUNT, bool FAST>
__global__ void __launch_bounds__(64, RTMI_PATH_WAVES) k_path_primary(DScene sc, OctArgs a, DCtrl* __restrict__ ctrl, int refill_min, int xcd_aware) {
    extern __shared__ uint32_t lds[];
    oct_walk<COUNT, FAST, W_PRIMARY>(sc, a, ctrl, lds, refill_min, xcd_aware);
}
// k_path_primary with the node cull (scenes with node cull records, RTMI_PRIMARY_NODE_CULL != 0); a kernel of its own, so
// that every other scene runs k_path_primary as it was
template <bool COUNT, bool FAST>
__global__ void __launch_bounds__(64, RTMI_PATH_WAVES) k_path_primary_cull(DScene sc, OctArgs a, DCtrl* __restrict__ ctrl, int refill_min, int xcd_aware) {
    extern __shared__ uint32_t lds[];
    oct_walk<COUNT, FAST, W_PRIMARY, Samp::FRAME, true>(sc, a, ctrl, lds, refill_min, xcd_aware);
}
template <bool COUNT, bool FAST>
__global__ void __launch_bounds__(64, RTMI_PATH_WAVES) k_path_slow(DScene sc, OctArgs a, DCtrl* __restrict__ ctrl, int refill_min, int xcd_aware) {
    extern __shared__ uint32_t lds[];
    oct_walk<COUNT, FAST, W_SLOW>(sc, a, ctrl, lds, refill_min, xcd_aware);
}
// The same two kernels for progressive passes (rtmi_render_samples*): sample numbers start at DView::sample_key's sample0
template <bool COUNT, bool FAST>
__global__ void __launch_bounds__(64, RTMI_PATH_WAVES) k_path_primary_samples(DScene sc, OctArgs a, DCtrl* __restrict__ ctrl, int refill_min, int xcd_aware) {
    extern __shared__ uint32_t lds[];
    oct_walk<COUNT, FAST, W_PRIMARY, Samp::PASS>(sc, a, ctrl, lds, refill_min, xcd_aware);
}
template <bool COUNT, bool FAST>
__global__ void __launch_bounds__(64, RTMI_PATH_WAVES) k_path_primary_samples_cull(DScene sc, OctArgs a, DCtrl* __restrict__ ctrl, int refill_min,
                                                                                   int xcd_aware) {
    extern __shared__ uint32_t lds[];
    oct_walk<COUNT, FAST, W_PRIMARY, Samp::PASS, true>(sc, a, ctrl, lds, refill_min, xcd_aware);
}
template <bool COUNT, bool FAST>
__global__ void __launch_bounds__(64, RTMI_PATH_WAVES) k_path_slow_samples(DScene sc, OctArgs a, DCtrl* __restrict__ ctrl, int refill_min, int xcd_aware) {
    extern __shared__ uint32_t lds[];
    oct_walk<COUNT, FAST, W_SLOW, Samp::PASS>(sc, a, ctrl, lds, refill_min, xcd_aware);
}
// ... and for adaptive passes (rtmi_render_adaptive*): local pixel q of the batch is list[pix0 + q], a tile-local pixel index.
// The list pointer is a kernel argument of these two only (OctArgs, shared with every other walk kernel, stays as it is).
template <bool COUNT, bool FAST>
__global__ void __launch_bounds__(64, RTMI_PATH_WAVES) k_path_primary_list(DScene sc, OctArgs a, DCtrl* __restrict__ ctrl, int refill_min, int xcd_aware,
                                                                           const uint32_t* __restrict__ list) {
    extern __shared__ uint32_t lds[];
    oct_walk<COUNT, FAST, W_PRIMARY, Samp::LIST>(sc, a, ctrl, lds, refill_min, xcd_aware, RecArgs{}, list);
}
template <bool COUNT, bool FAST>
__global__ void __launch_bounds__(64, RTMI_PATH_WAVES) k_path_primary_list_cull(DScene sc, OctArgs a, DCtrl* __restrict__ ctrl, int refill_min,
                                                                                int xcd_aware, const uint32_t* __restrict__ list) {
    extern __shared__ uint32_t lds[];
    oct_walk<COUNT, FAST, W_PRIMARY, Samp::LIST, true>(sc, a, ctrl, lds, refill_min, xcd_aware, RecArgs{}, list);
}
template <bool COUNT, bool FAST>
__global__ void __launch_bounds__(64, RTMI_PATH_WAVES) k_path_slow_list(DScene sc, OctArgs a, DCtrl* __restrict__ ctrl, int refill_min, int xcd_aware,
                                                                        const uint32_t* __restrict__ list) {
    extern __shared__ uint32_t lds[];
    oct_walk<COUNT, FAST, W_SLOW, Samp::LIST>(sc, a, ctrl, lds, refill_min, xcd_aware, RecArgs{}, list);
}
// ... and for batches of views (rtmi_render_views*): each view's camera and seed from the view table, an argument of these
// two only, like the list above
template <bool COUNT, bool FAST>
__global__ void __launch_bounds__(64, RTMI_PATH_WAVES) k_path_primary_views(DScene sc, OctArgs a, DCtrl* __restrict__ ctrl, int refill_min,
                                                                            int xcd_aware, ViewTab vt) {
    extern __shared__ uint32_t lds[];
    oct_walk<COUNT, FAST, W_PRIMARY, Samp::VIEWS>(sc, a, ctrl, lds, refill_min, xcd_aware, RecArgs{}, nullptr, vt);
}
template <bool COUNT, bool FAST>
__global__ void __launch_bounds__(64, RTMI_PATH_WAVES) k_path_primary_views_cull(DScene sc, OctArgs a, DCtrl* __restrict__ ctrl, int refill_min,
                                                                                 int xcd_aware, ViewTab vt) {
    extern __shared__ uint32_t lds[];
    oct_walk<COUNT, FAST, W_PRIMARY, Samp::VIEWS, true>(sc, a, ctrl, lds, refill_min, xcd_aware, RecArgs{}, nullptr, vt);
}
template <bool COUNT, bool FAST>
__global__ void __launch_bounds__(64, RTMI_PATH_WAVES) k_path_slow_views(DScene sc, OctArgs a, DCtrl* __restrict__ ctrl, int refill_min,
                                                                         int xcd_aware, ViewTab vt) {
    extern __shared__ uint32_t lds[];
    oct_walk<COUNT, FAST, W_SLOW, Samp::VIEWS>(sc, a, ctrl, lds, refill_min, xcd_aware, RecArgs{}, nullptr, vt);
}

}  // namespace rtmi
