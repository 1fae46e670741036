// rt_trace.h -- the geometry every ray-tracing kernel rests on (device header; gfx950 / CDNA4, wave64): V3 algebra, Hit, Counters,
// the sphere / plane / box / triangle tests, the scalar-cache loads (cld*), the BVH traversal stack, mesh_hit and trace<ANY, MODEL, TEX>
// (closest hit or any hit through the scene's object list).  Behind them what a unit below the shading layer also needs: the
// texture lookups (k_resolve samples the background map), attenuation (the photon bounce) and pixel_of (the tile walk of k_resolve).
// Included by rt_shade.h (and through it rt_kernels.hip), by rt_trace.hip and by rt_resolve.hip.
// May include rt_launch.h and rt_kernel_util.h, nothing of the shading layer.
//
// The arithmetic of every device function follows the reference operation by operation (same
// expression order, thresholds and quirks; file:line cited per function, FIN = the reference's
// RayTracingFinal/RayTracingFinal) and every unit is compiled with -ffp-contract=off, so hit
// records agree with the CPU oracle bit for bit and colours to the last ulp of powf/expf.
// What differs is control: the recursion of TraceNode/TraceBVHNode/Shade becomes loops, ray
// queues and a per-lane LDS stack; zero-weight subtrees are not traced; the shadow ray is an
// any-hit query; BVH boxes are culled against the closest hit so far.
#ifndef RT_TRACE_H
#define RT_TRACE_H

#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include "rt_launch.h"
#include "rt_kernel_util.h"

#define BIGFLOAT 1.0e30f
#define LEAF_BIT 0x80000000u

// ------------------------------------------------------------------------------------------------
// float3 algebra in the reference's evaluation order (cyPoint.h:259-350, cyMatrix.h:542-546)
// ------------------------------------------------------------------------------------------------
struct V3 { float x, y, z; };
__device__ __forceinline__ V3 mk(float x, float y, float z) { V3 r; r.x = x; r.y = y; r.z = z; return r; }
__device__ __forceinline__ V3 ld3(const float *p) { return mk(p[0], p[1], p[2]); }
__device__ __forceinline__ V3 operator+(V3 a, V3 b) { return mk(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ __forceinline__ V3 operator-(V3 a, V3 b) { return mk(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ V3 operator*(V3 a, V3 b) { return mk(a.x * b.x, a.y * b.y, a.z * b.z); }
__device__ __forceinline__ V3 operator*(V3 a, float s) { return mk(a.x * s, a.y * s, a.z * s); }
__device__ __forceinline__ V3 operator/(V3 a, float s) { return mk(a.x / s, a.y / s, a.z / s); }
__device__ __forceinline__ V3 operator-(V3 a) { return mk(-a.x, -a.y, -a.z); }
__device__ __forceinline__ float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ V3 cross(V3 a, V3 p) { return mk(a.y * p.z - a.z * p.y, a.z * p.x - a.x * p.z, a.x * p.y - a.y * p.x); }
__device__ __forceinline__ float len2(V3 a) { return dot(a, a); }
__device__ __forceinline__ V3 normalize(V3 a) { return a / sqrtf(len2(a)); }
__device__ __forceinline__ V3 mmul(const float *d, V3 p)
{
    return mk(p.x * d[0] + p.y * d[3] + p.z * d[6], p.x * d[1] + p.y * d[4] + p.z * d[7], p.x * d[2] + p.y * d[5] + p.z * d[8]);
}
__device__ __forceinline__ V3 mtmul(const float *d, V3 v)      // TransposeMult, scene.h:254-261
{
    return mk(dot(mk(d[0], d[1], d[2]), v), dot(mk(d[3], d[4], d[5]), v), dot(mk(d[6], d[7], d[8]), v));
}
__device__ __forceinline__ float gray(V3 c) { return (c.x + c.y + c.z) / 3.0f; }      // Color::Gray, cyColor.h
#define RMAX(a, b) ((a) > (b) ? (a) : (b))     // the reference's macros, scene.h:48-54
#define RMIN(a, b) ((a) < (b) ? (a) : (b))

struct Counters { uint32_t inst, nodes, tris, shadow; uint32_t occ; };     // occ: 1 + the object that occluded this lane's last shadow ray (0: none)

// Halton, FIN/include/scene.h:131-140
__device__ __forceinline__ float halton(int index, int base)
{
    float r = 0;
    float f = 1.0f / (float)base;
    for (int i = index; i > 0; i /= base) { r += f * (i % base); f /= (float)base; }
    return r;
}


struct Hit { float z; V3 p, N; int node; int front; V3 uvw; };

// ------------------------------------------------------------------------------------------------
// primitives (object space)
// ------------------------------------------------------------------------------------------------
// Sphere::IntersectRay, FIN/include/objects.h:24-70
__device__ __forceinline__ bool sphere_hit(V3 rp, V3 rd, float &z, V3 &hp, V3 &hN, int &front)
{
    const float a = dot(rd, rd);
    const float c = dot(rp, rp) - 1;
    const float b = 2 * dot(rp, rd);
    const float insqrt = b * b - (4 * a * c);
    const float zero = 0.001f;
    if (insqrt >= zero) {
        const float sq = sqrtf(insqrt);
        const float t1 = (-b + sq) / (a * 2);
        const float t2 = (-b - sq) / (a * 2);
        const float prez = z;
        if (t2 >= prez) return false;
        if (t1 > zero && t2 < zero && t1 < prez) {
            z = t1; front = 0;
            hp = rd * z + rp; hN = normalize(hp);
            return true;
        } else if (t1 > zero && t2 > zero && t2 < prez) {
            z = t2; front = 1;
            hp = rd * z + rp; hN = normalize(hp);
            return true;
        }
    }
    return false;
}

// Sphere::IntersectRay of RayTracingProj3 (main.cpp:192-221): no bias, z = min(t1,t2), rejected when negative
// or not closer; N = p un-normalised; front untouched
__device__ __forceinline__ bool sphere_hit_p3(V3 rp, V3 rd, float &z, V3 &hp, V3 &hN)
{
    const float a = dot(rd, rd);
    const float c = dot(rp, rp) - 1;
    const float b = 2 * dot(rp, rd);
    const float insqrt = b * b - (4 * a * c);
    if (insqrt >= 0) {
        const float sq = sqrtf(insqrt);
        const float t1 = (-b + sq) / (a * 2);
        const float t2 = (-b - sq) / (a * 2);
        const float zz = RMIN(t1, t2);
        if (zz < 0 || zz >= z) return false;
        z = zz;
        hp = rd * z + rp; hN = hp;
        return true;
    }
    return false;
}

// Plane::IntersectRay, FIN/include/objects.h:84-111 (P13 flips `front`, P13/include/objects.h:98-101)
__device__ __forceinline__ bool plane_hit(int model, V3 P, V3 d, float &z, V3 &hp, V3 &hN, int &front)
{
    const float zero = 0.001f;
    const float t = -(P.z / d.z);
    if (t >= zero && t < BIGFLOAT && t < z) {
        const V3 Hitp = P + d * t;
        if (Hitp.x >= -1 && Hitp.x <= 1 && Hitp.y >= -1 && Hitp.y <= 1) {
            z = t; hp = Hitp; hN = mk(0, 0, 1);
            const float nd = dot(mk(0, 0, 1), d);
            front = (model != RT_SHADE_FIN) ? ((nd < 0.0f) ? 0 : 1) : ((nd <= 0.0f) ? 1 : 0);
            return true;
        }
    }
    return false;
}

// Slab test against a node box.  Box::IntersectRay (FIN/scene.cpp:11-65) is only conservative
// (accepts boxes behind the ray, never culls by distance); this one culls against the closest
// hit so far and is padded by 2e-6 relative so that reciprocal rounding never rejects a box
// whose triangle the exact test would accept.  Returns the entry distance, or BIGFLOAT*2.
// `inv` comes from slab_inv: NaN where the direction component is zero.  Both products of that axis are then NaN and the fmaxf /
// fminf below drop them (they return the other operand): a slab the ray runs parallel to does not constrain it, as in
// Box::IntersectRay, which skips an axis with dir == 0.  (With inv = 1/0 = inf and the origin ON a plane of the slab one
// product is 0 * inf = NaN and the other +-inf, which min / max keep on BOTH sides: tenter = +inf or texit = -inf, and a box
// the reference enters was rejected.)  An unused child's bounds are NaN on every axis: tenter and texit NaN, never a hit.
__device__ __forceinline__ float slab_inv(float d, float rcp) { return d == 0.0f ? __builtin_nanf("") : rcp; }
__device__ __forceinline__ float box_entry(const float *lo, const float *hi, V3 o, V3 inv, float zbest)
{
    const float t0x = (lo[0] - o.x) * inv.x, t1x = (hi[0] - o.x) * inv.x;
    const float t0y = (lo[1] - o.y) * inv.y, t1y = (hi[1] - o.y) * inv.y;
    const float t0z = (lo[2] - o.z) * inv.z, t1z = (hi[2] - o.z) * inv.z;
    const float tenter = fmaxf(fmaxf(fminf(t0x, t1x), fminf(t0y, t1y)), fminf(t0z, t1z));
    const float texit = fminf(fminf(fmaxf(t0x, t1x), fmaxf(t0y, t1y)), fmaxf(t0z, t1z));
    const bool hit = (texit >= 0.0f) && (tenter <= texit * 1.000002f) && (tenter * 0.999998f <= zbest);
    return hit ? tenter : 3.0e30f;
}

// TriObj::TriangleArea, FIN/include/objects.h:146-157
__device__ __forceinline__ float tri_area(int i, V3 A, V3 B, V3 C)
{
    if (i == 0) return (B.y - A.y) * (C.z - A.z) - (C.y - A.y) * (B.z - A.z);
    if (i == 1) return (B.x - A.x) * (C.z - A.z) - (C.x - A.x) * (B.z - A.z);
    return (B.x - A.x) * (C.y - A.y) - (C.x - A.x) * (B.y - A.y);
}

// TriObj::IntersectTriangle, FIN/include/objects.h:226-267.  N (unit face normal) is precomputed
// with the same expression on the host.  Returns barycentrics; normal interpolation is deferred.
__device__ __forceinline__ bool tri_hit_fin(const DevTri &T, V3 rp, V3 rd, float &z, V3 &hp, V3 &bc, int &front)
{
    const V3 A = ld3(T.A), B = ld3(T.B), C = ld3(T.C), N = ld3(T.N);
    const float dz = dot(rd, N);
    if (fabsf(dz) < 1e-7f) return false;
    const float pz = dot(rp - A, N);
    const float t = -pz / dz;
    if (t <= 0.001f) return false;
    if (t < z) {
        const V3 p = rp + rd * t;
        int ign;
        const float ax = fabsf(N.x), ay = fabsf(N.y), az = fabsf(N.z);
        if (ax > ay && ax > az) ign = 0; else if (ay > az) ign = 1; else ign = 2;
        const float s = 1.f / tri_area(ign, A, B, C);
        const float a = tri_area(ign, p, B, C) * s;
        const float b = tri_area(ign, p, C, A) * s;
        const float c = 1.f - a - b;
        if (a < 0 || b < 0 || c < 0) return false;
        z = t; hp = p; bc = mk(a, b, c); front = (dz <= 0) ? 1 : 0;
        return true;
    }
    return false;
}

// TriObj::IntersectTriangle, P13/include/objects.h:148-206 (back-face culled, bias 1e-7)
__device__ __forceinline__ bool tri_hit_p13(const DevTri &T, V3 rp, V3 rd, float &z, V3 &hp, V3 &bc, int &front)
{
    const float bias = 1e-7f;
    const V3 A = ld3(T.A), B = ld3(T.B), C = ld3(T.C), tN = ld3(T.N);
    if (dot(tN, rp - A) < bias) return false;
    const float den = dot(tN, rd);
    if (den == 0) return false;
    const float t = dot(tN, C - rp) / den;
    if (t < bias || t >= z || t >= BIGFLOAT) return false;
    const float fx = fabsf(tN.x), fy = fabsf(tN.y), fz = fabsf(tN.z);
    const float maxN = fmaxf(fz, fmaxf(fx, fy));
    const V3 P = rp + rd * t;
    float pax, pay, pbx, pby, pcx, pcy, ppx, ppy;
    if (maxN == fx)      { pax = A.y; pay = A.z; pbx = B.y; pby = B.z; pcx = C.y; pcy = C.z; ppx = P.y; ppy = P.z; }
    else if (maxN == fy) { pax = A.x; pay = A.z; pbx = B.x; pby = B.z; pcx = C.x; pcy = C.z; ppx = P.x; ppy = P.z; }
    else                 { pax = A.x; pay = A.y; pbx = B.x; pby = B.y; pcx = C.x; pcy = C.y; ppx = P.x; ppy = P.y; }
    const float area_tri = (pax - pcx) * (pby - pcy) - (pay - pcy) * (pbx - pcx);
    const float area_bcp = (ppx - pcx) * (pby - pcy) - (ppy - pcy) * (pbx - pcx);
    const float area_acp = (pax - pcx) * (ppy - pcy) - (pay - pcy) * (ppx - pcx);
    const float alpha = area_bcp / area_tri;
    const float beta = area_acp / area_tri;
    const float gam = (float)(1.0 - (double)alpha - (double)beta);
    if (alpha < -bias || beta < -bias || gam < -bias || alpha > 1.0f || beta > 1.0f || gam > 1.0f) return false;
    z = t; bc = mk(alpha, beta, gam); front = 1;
    hp = A * alpha + B * beta + C * gam;
    return true;
}

// Scene tables (objects, node transforms, lights) are written before a launch and only read by it, and the loops over
// them are wave-uniform: read through the constant address space such a table entry comes over the scalar data cache
// into SGPRs (s_load, merged to x4/x8/x16) -- one short-latency read per wave instead of a 64-lane vector load of one
// address, and no vector registers held for data every lane shares.  (With a lane-varying index the same code falls
// back to a vector load.)
template <class T> __device__ __forceinline__ T cld(const T *p) { return *(const __attribute__((address_space(4))) T *)(uintptr_t)p; }
__device__ __forceinline__ V3 cld3(const float *p) { return mk(cld(p), cld(p + 1), cld(p + 2)); }
struct M9 { float m[9]; };
__device__ __forceinline__ rt_light cld_light(const rt_light *p)
{
    rt_light l;
    l.type = cld(&p->type); l.size = cld(&p->size);
    for (int i = 0; i < 3; i++) { l.intensity[i] = cld(p->intensity + i); l.position[i] = cld(p->position + i); l.direction[i] = cld(p->direction + i); }
    return l;
}
__device__ __forceinline__ M9 cld9(const float *p) { M9 r; for (int i = 0; i < 9; i++) r.m[i] = cld(p + i); return r; }

// A thread's BVH traversal stack: `cap` entries in LDS (entry i of this thread at lds[i * RT_BLOCK]) and RT_BVH_SPILL more in
// HBM behind them (spill, this thread's own 64 bytes; NULL when the scene's trees cannot outgrow the LDS part -- the host
// checks DevScene::max_bvh_depth against cap + RT_BVH_SPILL).  The spill part is touched only by a traversal that is
// deeper than the LDS part: a four-wide node leaves up to three entries behind.
typedef __attribute__((address_space(3))) uint32_t lds_u32;      // the LDS part is addressed as LDS (ds_read / ds_write), never through flat instructions
struct BvhStack { lds_u32 *lds; uint32_t *spill; uint32_t cap; };
__device__ __forceinline__ BvhStack bvh_stack(uint32_t *lds_base, uint32_t cap, uint32_t *spill_base)
{
    BvhStack st;
    st.lds = (lds_u32 *)lds_base + threadIdx.x; st.cap = cap;
    st.spill = spill_base ? spill_base + ((size_t)blockIdx.x * RT_BLOCK + threadIdx.x) * RT_BVH_SPILL : nullptr;
    return st;
}
__device__ __forceinline__ void bvh_push(const BvhStack &st, uint32_t &sp, uint32_t v)
{
    if (sp < st.cap) st.lds[sp * RT_BLOCK] = v;
    else if (st.spill && sp < st.cap + RT_BVH_SPILL) st.spill[sp - st.cap] = v;
    sp++;
}
__device__ __forceinline__ uint32_t bvh_pop(const BvhStack &st, uint32_t &sp)
{
    --sp;
    if (sp < st.cap) return st.lds[sp * RT_BLOCK];
    return st.spill[sp - st.cap];
}

// TriObj::IntersectRay -> TraceBVHNode (FIN/include/objects.h:127-133, 271-302) as an iterative,
// near-first traversal with a per-lane stack in LDS.  ANY: stop at the first accepted triangle.
template <bool ANY, int MODEL>
__device__ bool mesh_hit(const DevMesh *Mp, V3 o, V3 d, float &z, V3 &hp, V3 &hN, int &front,
                         const BvhStack &stack, Counters &cnt, V3 *uvw = nullptr)
{
    // the mesh record is the same for every lane: over the scalar cache (see cld), so that the array bases live in SGPRs
    DevMesh M;
    M.nodes = cld(&Mp->nodes); M.tris = cld(&Mp->tris); M.nrm = cld(&Mp->nrm); M.tex = cld(&Mp->tex);
    for (int i = 0; i < 6; i++) M.root_box[i] = cld(Mp->root_box + i);
    M.root_ref = cld(&Mp->root_ref);
    const V3 inv = mk(slab_inv(d.x, 1.0f / d.x), slab_inv(d.y, 1.0f / d.y), slab_inv(d.z, 1.0f / d.z));
    if (box_entry(M.root_box, M.root_box + 3, o, inv, z) > 2.0e30f) return false;
    uint32_t cur = M.root_ref;
    uint32_t sp = 0;
    bool any = false;
    uint32_t best_slot = 0;
    V3 bc = mk(0, 0, 0);
    // "while-while" traversal: every lane first walks down to its next leaf (inner loop), then all lanes
    // that hold a leaf test its triangles together.  With one loop that does either step per iteration a
    // single lane at a leaf makes the whole wave sit through the triangle code; for the reflected rays of
    // the 100 k-triangle scene that costs about half the bounce kernel's time.  Each lane still visits
    // the same nodes and triangles in the same order (near child first, far child on the stack).
    const uint32_t DONE = 0xFFFFFFFFu;                  // has LEAF_BIT set: ends the inner loop
    while (cur != DONE) {
        while (!(cur & LEAF_BIT)) {
            // one 128-byte record = the boxes of four children (two levels of the reference's tree): six 16-byte loads of
            // bounds, one of refs, issued together -- ONE dependent round trip where the binary tree takes two
            const float4 *np = (const float4 *)(M.nodes + cur);
            const float4 lx = np[0], ly = np[1], lz = np[2], hx = np[3], hy = np[4], hz = np[5];
            const uint4 cr = *(const uint4 *)(np + 6);
            cnt.nodes++;
            const float l0[3] = {lx.x, ly.x, lz.x}, h0[3] = {hx.x, hy.x, hz.x}, l1[3] = {lx.y, ly.y, lz.y}, h1[3] = {hx.y, hy.y, hz.y};
            const float l2[3] = {lx.z, ly.z, lz.z}, h2[3] = {hx.z, hy.z, hz.z}, l3[3] = {lx.w, ly.w, lz.w}, h3[3] = {hx.w, hy.w, hz.w};
            float e0 = box_entry(l0, h0, o, inv, z), e1 = box_entry(l1, h1, o, inv, z);
            float e2 = box_entry(l2, h2, o, inv, z), e3 = box_entry(l3, h3, o, inv, z);      // an unused child's bounds are NaN: never entered
            uint32_t c0 = cr.x, c1 = cr.y, c2 = cr.z, c3 = cr.w;
            // nearest first: sort the four (entry distance, ref) pairs (misses carry 3e30 and end up last); equal distances keep
            // the reference's child order
#define RT_CSWAP(ea, ca, eb, cb) do { const bool s_ = (eb) < (ea); const float te_ = s_ ? (eb) : (ea); const uint32_t tc_ = s_ ? (cb) : (ca); \
                                      (eb) = s_ ? (ea) : (eb); (cb) = s_ ? (ca) : (cb); (ea) = te_; (ca) = tc_; } while (0)
            RT_CSWAP(e0, c0, e1, c1); RT_CSWAP(e2, c2, e3, c3); RT_CSWAP(e0, c0, e2, c2); RT_CSWAP(e1, c1, e3, c3); RT_CSWAP(e1, c1, e2, c2);
#undef RT_CSWAP
            if (e3 < 2.0e30f) bvh_push(stack, sp, c3);
            if (e2 < 2.0e30f) bvh_push(stack, sp, c2);
            if (e1 < 2.0e30f) bvh_push(stack, sp, c1);
            cur = (e0 < 2.0e30f) ? c0 : (sp ? bvh_pop(stack, sp) : DONE);
        }
        if (cur == DONE) break;
        const uint32_t count = ((cur >> 28) & 7u) + 1;
        const uint32_t first = cur & 0x0FFFFFFFu;
        // the next triangle of the leaf is fetched while this one is tested (one exposed round trip per leaf, not per triangle)
        DevTri T = M.tris[first];
        for (uint32_t i = 0; i < count; i++) {
            DevTri Tn = T;
            if (i + 1 < count) Tn = M.tris[first + i + 1];
            cnt.tris++;
            const bool h = (MODEL != RT_SHADE_FIN) ? tri_hit_p13(T, o, d, z, hp, bc, front)
                                                   : tri_hit_fin(T, o, d, z, hp, bc, front);
            if (h) { any = true; best_slot = first + i; }
            T = Tn;
        }
        if (ANY && any) return true;
        cur = sp ? bvh_pop(stack, sp) : DONE;
    }
    if (!any) return false;
    // cyTriMesh::GetNormal = vn[fn0]*bc.x + vn[fn1]*bc.y + vn[fn2]*bc.z (cyTriMesh.h:167,191)
    const float *n9 = M.nrm + 9 * (size_t)best_slot;
    const V3 Ni = ld3(n9) * bc.x + ld3(n9 + 3) * bc.y + ld3(n9 + 6) * bc.z;
    hN = (MODEL != RT_SHADE_FIN) ? normalize(Ni) : Ni;     // FIN leaves it un-normalised (:262)
    // the PROJ13 triangle also sets uvw = GetTexCoord(face, bc) (P13/include/objects.h:203)
    if (MODEL != RT_SHADE_FIN && uvw && M.tex) {
        const float *t9 = M.tex + 9 * (size_t)best_slot;
        *uvw = ld3(t9) * bc.x + ld3(t9 + 3) * bc.y + ld3(t9 + 6) * bc.z;
    }
    return true;
}

// ------------------------------------------------------------------------------------------------
// TraceNode(rootNode, ray, hit), FIN/main.cpp:108-130, flattened: for every node that carries an
// Object (in the recursion's visiting order) the ray is taken through ToNodeCoords of each
// ancestor in turn (scene.h:502-508; direction NOT renormalised, so t is shared by all spaces),
// and the closest hit is brought back through FromNodeCoords of each ancestor (scene.h:509-513).
// ------------------------------------------------------------------------------------------------
template <bool ANY, int MODEL, bool TEX = false>
__device__ bool trace(const DevScene &S, V3 o, V3 d, float zinit, Hit &h, const BvhStack &stack, Counters &cnt)
{
    float z = zinit;
    int best = -1, bfront = 1;
    V3 bp = mk(0, 0, 0), bN = mk(0, 0, 0);
    // HitInfo::uvw starts at (0.5,0.5,0.5) (scene.h:163); spheres and planes overwrite it whenever they
    // accept a hit (objects.h:49-51,103), FIN's triangles never do (:226-267) -- so a mesh hit keeps the
    // coordinate of whatever sphere/plane hit the ray had accepted before it.  Reproduced as is.
    // (The PROJ13 triangle does write it, from the mesh's texture vertices.)
    V3 uvw = mk(0.5f, 0.5f, 0.5f);
    // Node::ToNodeCoords (scene.h:502-508) of one level; the direction is the image of p+d minus the image of p
    auto to_node = [&](int node, V3 &lp, V3 &ldir) {
        const DevNodeXf *X = S.nodes + node;
        const V3 pos = cld3(X->pos);
        const M9 itm = cld9(X->itm);
        const V3 rp = mmul(itm.m, lp - pos);
        ldir = mmul(itm.m, (lp + ldir) - pos) - rp;
        lp = rp;
    };
    // Every chain starts at the root (node 0) and siblings share their parent: the ray in the root's and
    // in the last visited level-1 group's coordinates is kept instead of being recomputed per object
    // (same operations on the same inputs, so the results do not change).  The object loop is
    // wave-uniform, so the bookkeeping is scalar.
    V3 p0 = o, d0 = d;
    to_node(0, p0, d0);
    V3 p1 = p0, d1 = d0;
    int cached1 = -1;
    // reciprocal direction (in the root's coordinates) for the bounds cull only: approximate is fine, the
    // bounds are inflated
    const V3 winv = mk(slab_inv(d0.x, __builtin_amdgcn_rcpf(d0.x)), slab_inv(d0.y, __builtin_amdgcn_rcpf(d0.y)), slab_inv(d0.z, __builtin_amdgcn_rcpf(d0.z)));
    // any-hit queries: the object that occluded the last shadow ray of this wave is tried first (its neighbours' rays mostly end on
    // the same occluder, and the first accepted hit ends a lane's query: the order of the objects does not change the answer)
    int hint = -1;
    if (ANY) { hint = __builtin_amdgcn_readfirstlane((int)cnt.occ) - 1; if (hint >= S.n_objects) hint = -1; }
    for (int it = (hint >= 0 ? -1 : 0); it < S.n_objects; it++) {
        const int oi = it < 0 ? hint : it;
        if (it >= 0 && oi == hint) continue;
        const DevObject *obp = S.objects + oi;
        // Everything this iteration needs of the object comes from its one 128-byte record, fetched by two 64-byte scalar loads
        // issued back to back and waited for ONCE.  Written as inline assembly because the compiler, short of scalar registers
        // in these kernels, otherwise sinks every field's load to its first use: five dependent scalar-cache round trips per
        // object (bounds -> chain length -> group id -> chain entry -> node transform) in a loop three waves per SIMD cannot hide.
        typedef uint32_t u32x16 __attribute__((ext_vector_type(16)));
        u32x16 r0, r1;
        asm volatile("s_load_dwordx16 %0, %2, 0x0\n\ts_load_dwordx16 %1, %2, 0x40\n\ts_waitcnt lgkmcnt(0)" : "=&s"(r0), "=&s"(r1) : "s"(obp) : "memory");
        static_assert(offsetof(DevObject, type) == 24 && offsetof(DevObject, chain_len) == 32 && offsetof(DevObject, chain) == 48 && offsetof(DevObject, own_itm) == 80, "record layout the loads assume");
        const float wlo[3] = {__uint_as_float(r0[0]), __uint_as_float(r0[1]), __uint_as_float(r0[2])}, whi[3] = {__uint_as_float(r0[3]), __uint_as_float(r0[4]), __uint_as_float(r0[5])};
        const int ob_type = (int)r0[6], ob_mesh = (int)r0[7], ob_chain_len = (int)r0[8], n1 = (int)r0[13];
        M9 own_itm;
        own_itm.m[0] = __uint_as_float(r1[4]); own_itm.m[1] = __uint_as_float(r1[5]); own_itm.m[2] = __uint_as_float(r1[6]);
        own_itm.m[3] = __uint_as_float(r1[7]); own_itm.m[4] = __uint_as_float(r1[8]); own_itm.m[5] = __uint_as_float(r1[9]);
        own_itm.m[6] = __uint_as_float(r1[10]); own_itm.m[7] = __uint_as_float(r1[11]); own_itm.m[8] = __uint_as_float(r1[12]);
        const V3 own_pos = mk(__uint_as_float(r1[13]), __uint_as_float(r1[14]), __uint_as_float(r1[15]));
        // skip the object when no lane's ray can reach its bounds before that lane's closest hit so far
        if (!__any(box_entry(wlo, whi, p0, winv, z) < 2.0e30f)) continue;
        V3 lp = p0, ldir = d0;
        int c = 1;
        if (ob_chain_len > 2) {
            if (n1 != cached1) { p1 = p0; d1 = d0; to_node(n1, p1, d1); cached1 = n1; }
            lp = p1; ldir = d1; c = 2;
        }
        for (; c < ob_chain_len - 1; c++) to_node(cld(&obp->chain[c]), lp, ldir);     // levels between the group and the object: deeper scene graphs only
        if (ob_chain_len > 1) {
            // the object's own level, Node::ToNodeCoords with the copy of its transform in the record (same arithmetic as to_node)
            const V3 rp = mmul(own_itm.m, lp - own_pos);
            ldir = mmul(own_itm.m, (lp + ldir) - own_pos) - rp;
            lp = rp;
        }
        cnt.inst++;
        V3 hp, hN;
        int fr = 1;
        bool hit = false;
        if (ob_type == RT_OBJ_SPHERE) hit = (MODEL == RT_SHADE_P3) ? sphere_hit_p3(lp, ldir, z, hp, hN) : sphere_hit(lp, ldir, z, hp, hN, fr);
        else if (ob_type == RT_OBJ_PLANE) hit = plane_hit(MODEL, lp, ldir, z, hp, hN, fr);
        else if (ob_type == RT_OBJ_MESH) hit = mesh_hit<ANY, MODEL>(S.meshes + ob_mesh, lp, ldir, z, hp, hN, fr, stack, cnt, (TEX && S.use_uvw) ? &uvw : nullptr);
        if (hit) {
            if (ANY) { cnt.occ = (uint32_t)oi + 1u; return true; }
            best = oi; bp = hp; bN = hN; bfront = fr;
            if (TEX && S.use_uvw) {
                if (ob_type == RT_OBJ_SPHERE)               // objects.h:49-51, atan2/asin in double; hp is not normalised and rounding
                                                            // lifts |hp.z| above 1 next to a pole: asin's argument is clamped (rt_mi355x.h)
                    uvw = mk((float)(0.5 - atan2((double)hp.x, (double)hp.y) / (2 * M_PI)), (float)(0.5 + asin(fmin(1.0, fmax(-1.0, (double)hp.z))) / M_PI), 0);
                else if (ob_type == RT_OBJ_PLANE) uvw = mk((hp.x + 1) / 2, (hp.y + 1) / 2, 0);    // objects.h:103
            }
        }
    }
    if (best < 0) return false;
    h.uvw = uvw;
    // Node::FromNodeCoords (scene.h:509-513) level by level, the object's own node first.  The levels below the root come inline
    // with the object's DevObjectBack record (addresses depend on `best` alone: one round trip); the root's over the scalar cache.
    const DevObjectBack *ob = S.objects_back + best;
    const int len = ob->chain_len;
    auto from_node = [&](const DevNodeXf &X) {
        bp = mmul(X.tm, bp) + ld3(X.pos);
        bN = normalize(mtmul(X.itm, bN));
    };
    const int inl = min(len - 1, RT_BACK_LEVELS);            // levels held inline (all but the root, up to RT_BACK_LEVELS)
#pragma unroll
    for (int k = 0; k < RT_BACK_LEVELS; k++) if (k < inl) from_node(ob->lvl[k]);
    if (len - 1 > RT_BACK_LEVELS) {                          // a deeper chain: the levels between, through the object's chain
        const DevObject &o2 = S.objects[best];
        for (int c = len - 1 - RT_BACK_LEVELS; c >= 1; c--) from_node(S.nodes[o2.chain[c]]);
    }
    {
        const DevNodeXf *R = S.nodes;                        // chain[0] is the root for every object
        const M9 tm = cld9(R->tm), itm = cld9(R->itm);
        const V3 pos = cld3(R->pos);
        bp = mmul(tm.m, bp) + pos;
        bN = normalize(mtmul(itm.m, bN));
    }
    h.z = z; h.p = bp; h.N = bN; h.node = ob->node; h.front = bfront;
    return true;
}

// ------------------------------------------------------------------------------------------------
// textures: TextureFile::Sample (FIN/texture.cpp:95-121: tiling + bilinear), TextureChecker::Sample
// (:125-133), TextureMap (scene.h:376-398: uvw -> itm*(uvw-pos)) and TexturedColor::Sample (:422-423);
// SampleEnvironment and the material colours, which only shading uses, are in rt_shade.h.  duvw is always
// zero on this path, so the 32-tap filtered Texture::Sample (:331-349) reduces to one lookup.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ V3 tile_clamp(V3 uvw)
{
    V3 u = mk(uvw.x - (int)uvw.x, uvw.y - (int)uvw.y, uvw.z - (int)uvw.z);
    if (u.x < 0) u.x += 1;
    if (u.y < 0) u.y += 1;
    if (u.z < 0) u.z += 1;
    return u;
}
__device__ V3 texture_sample(const rt_texture &t, const uint8_t *texels, V3 uvw)
{
    // a coordinate that is not finite (a singular map transform can make one) samples black, like RT_MAP_EMPTY: rt_mi355x.h
    if (!(isfinite(uvw.x) && isfinite(uvw.y) && isfinite(uvw.z))) return mk(0, 0, 0);
    const V3 u = tile_clamp(uvw);
    if (t.type == RT_TEX_CHECKER) {
        const float *c = (u.x <= 0.5f) ? (u.y <= 0.5f ? t.color1 : t.color2) : (u.y <= 0.5f ? t.color2 : t.color1);
        return ld3(c);
    }
    const int width = t.width, height = t.height;
    if (width + height == 0) return mk(0, 0, 0);
    const uint8_t *data = texels + t.texel_offset;
    const float x = width * u.x, y = height * u.y;
    int ix = (int)x, iy = (int)y;
    const float fx = x - ix, fy = y - iy;
    if (ix < 0) ix -= (ix / width - 1) * width;
    if (ix >= width) ix -= (ix / width) * width;
    int ixp = ix + 1;
    if (ixp >= width) ixp -= width;
    if (iy < 0) iy -= (iy / height - 1) * height;
    if (iy >= height) iy -= (iy / height) * height;
    int iyp = iy + 1;
    if (iyp >= height) iyp -= height;
    auto texel = [&](int X, int Y) { const uint8_t *q = data + 3 * ((size_t)Y * width + X); return mk(q[0] / 255.0f, q[1] / 255.0f, q[2] / 255.0f); };
    return texel(ix, iy) * ((1 - fx) * (1 - fy)) + texel(ixp, iy) * (fx * (1 - fy)) + texel(ix, iyp) * ((1 - fx) * fy) + texel(ixp, iyp) * (fx * fy);
}
__device__ V3 textured_color(const DevScene &S, V3 color, const rt_texmap &m, V3 uvw)
{
    if (m.texture == RT_MAP_NONE) return color;
    V3 t = mk(0, 0, 0);
    if (m.texture >= 0 && m.texture < S.n_textures) t = texture_sample(S.textures[m.texture], S.texels, mmul(m.itm, uvw - ld3(m.pos)));
    return color * t;
}

// Attenuation, FIN/include/materials.h:60-66 (exp on floats resolves to the float overload)
__device__ __forceinline__ V3 attenuation(V3 a, float l) { return mk(expf(-a.x * l), expf(-a.y * l), expf(-a.z * l)); }

// chunk-local pixel q -> image pixel, walking this call's tiles (tile-major, row-major inside)
__device__ __forceinline__ bool pixel_of(const DevTiles &T, const DevCamera &cam, uint32_t q, int &x, int &y)
{
    const uint32_t per = (uint32_t)(T.tile_w * T.tile_h);
    const uint32_t k = fastdiv(q, T.div_per), w = q - k * per;
    if (k >= (uint32_t)T.n_tiles) return false;
    const uint32_t t = (uint32_t)T.first + k * (uint32_t)T.stride;
    const uint32_t ty = fastdiv(t, T.div_tiles_x), tx = t - ty * (uint32_t)T.tiles_x;
    const uint32_t wy = fastdiv(w, T.div_tile_w), wx = w - wy * (uint32_t)T.tile_w;
    x = (int)(tx * (uint32_t)T.tile_w + wx);
    y = (int)(ty * (uint32_t)T.tile_h + wy);
    return x < cam.width && y < cam.height;
}

#endif
