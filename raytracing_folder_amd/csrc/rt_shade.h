// rt_shade.h -- what the shading kernels share (device header; gfx950 / CDNA4, wave64): the counter-based random numbers (philox4x32,
// RngCtx, rng2), the wave-aggregated queue append, PathIn / SlotMap / ShadeCtx, environment_color, material_colors, illuminate, add_sample, push_ray,
// push_photon_query, the four shading models (shade_fin / p13 / p3 / p6) and shade_path, flush_counters, PrimaryArgs
// and primary_setup; RT_WF_PERWAVE, the one k_wavefront tuning define that shade_path reads.  Included by rt_kernels.hip alone;
// the trace-only kernels (rt_trace.hip) and the image kernels (rt_resolve.hip) do not see it.  May include rt_trace.h (and
// through it rt_launch.h and rt_kernel_util.h).
#ifndef RT_SHADE_H
#define RT_SHADE_H

#include "rt_trace.h"

#ifndef RT_WF_PERWAVE
#define RT_WF_PERWAVE 1        // 1: for the P12 model every wave of k_wavefront runs its own rounds on its own part of the LDS ray stack (no workgroup barriers); 0: the four waves always share stack and rounds
#endif

// ------------------------------------------------------------------------------------------------
// Counter-based random numbers for the stochastic effects.  The reference calls
// libc rand() from all its threads at once, so its sequences are not even reproducible; here every
// draw is Philox-4x32-10 keyed by the seed and counted by WHAT it is for:
//   (sample id = (y*W+x)*max_sample+j, ray-tree node, purpose, index)
// so a pixel's value does not depend on tiling, chunking, scheduling or the number of GPUs, and the
// CPU oracle draws the very same numbers.
// ------------------------------------------------------------------------------------------------
__host__ __device__ inline void philox4x32(uint32_t k0, uint32_t k1, uint32_t x0, uint32_t x1, uint32_t x2, uint32_t x3, uint32_t out[4])
{
    for (int r = 0; r < 10; r++) {
        const unsigned long long p0 = (unsigned long long)0xD2511F53u * x0, p1 = (unsigned long long)0xCD9E8D57u * x2;
        const uint32_t y0 = (uint32_t)(p1 >> 32) ^ x1 ^ k0, y1 = (uint32_t)p1, y2 = (uint32_t)(p0 >> 32) ^ x3 ^ k1, y3 = (uint32_t)p0;
        x0 = y0; x1 = y1; x2 = y2; x3 = y3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = x0; out[1] = x1; out[2] = x2; out[3] = x3;
}
#define RNG_LENS   1u     // DoF lens table entry (sample id = pixel id)
#define RNG_PICK   2u     // which lens entry a sample uses
#define RNG_SHADOW 3u     // area-light sample (index = light*64 + i, refinement batch at +32)
#define RNG_GLOSSR 4u     // glossy reflection jitter
#define RNG_GLOSST 5u     // glossy refraction jitter
#define RNG_GI     6u     // hemisphere sample
struct RngCtx { uint32_t seed, sample, node; };
// two uniforms in [0,1): each stands in for one rand() / (float) RAND_MAX
__device__ __forceinline__ void rng2(const RngCtx &c, uint32_t purpose, uint32_t index, float &u0, float &u1)
{
    uint32_t o[4];
    philox4x32(c.seed, 0x52544D49u, c.sample, c.node, (purpose << 24) | (index & 0xFFFFFFu), 0x5eed5eedu, o);
    u0 = (float)(o[0] >> 8) * (1.0f / 16777216.0f);
    u1 = (float)(o[1] >> 8) * (1.0f / 16777216.0f);
}
// id of a child node in the ray tree (1 = primary ray): only has to be reproducible
__host__ __device__ inline uint32_t child_node(uint32_t node, uint32_t kind) { return node * 0x9E3779B1u + kind * 0x85EBCA6Bu + 0x27D4EB2Fu; }

// ------------------------------------------------------------------------------------------------
// queues: wave-aggregated append (one atomic per wave, __ballot + popcount for the lane offset)
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t wave_push(bool pred, uint32_t *counter)
{
    const unsigned long long mask = ballot64(pred);
    if (mask == 0) return 0xFFFFFFFFu;
    const int lane = __lane_id();
    const int leader = __ffsll((long long)mask) - 1;
    uint32_t base = 0;
    if (lane == leader) base = atomicAdd(counter, (uint32_t)__popcll(mask));
    base = __shfl(base, leader);
    const uint32_t off = (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
    return pred ? base + off : 0xFFFFFFFFu;
}

#define KIND_REFLECT 0u
#define KIND_REFRACT 1u
#define KIND_GI      2u

// wave-wide maximum of a small non-negative int (loop bound for wave-collective pushes)
__device__ __forceinline__ int __reduce_max_sync_compat(int v)
{
    for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off));
    return v;
}

struct PathIn { V3 o, d, thr, absorb; uint32_t slot; int bounce; uint32_t kind; bool primary; uint32_t node, sample; V3 side_dir, side_K;
                uint32_t spec; };      // Shade's `specount` argument (P13/main.cpp:485): lights seen on the way, for the caustic lookup

// How a sample slot of the chunk maps back to its global sample id (pixel * max_sample + j, the key of the counter RNG): the
// LDS ray records of k_wavefront do not carry the id, it is recomputed for the rays of a scene that draws random numbers
struct SlotMap { DevTiles tiles; int32_t width, height; uint32_t q0; int32_t max_sample, mode; FastDiv div_ms; };

struct ShadeCtx {
    DevScene S; DevWork W; rt_params P;
    DevRayQueue qout; uint32_t *qout_count;
    // k_wavefront only: the workgroup's ray stack in LDS, THREE 16-byte words per ray (48 B):
    //   a = (o.xyz, d.x)   b = (d.yz, thr.r, thr.g)   c = (thr.b, slot, bounce | kind << 4 | spec << 8 | material << 16, node)
    // -- the absorption the child needs on arrival travels as the index of the material that spawned it, the sample id is
    // recomputed from the slot (SlotMap).  Children go there first and to qout (the 64-byte global form) only when it is
    // full.  NULL in the per-level kernels.
    float4 *lds_a, *lds_b, *lds_c; uint32_t *lds_count; uint32_t lds_cap;
    SlotMap sm;
    // reproducible instantiations only (FX = true): the secondary plane, three int64 fixed-point values per sample (fx_encode);
    // last member, so that the default instantiations' argument layout does not move
    unsigned long long *fx;
};

// the environment and the material colours on top of rt_trace.h's textured_color: SampleEnvironment (FIN scene.h:426-432) and
// the two TexturedColor::Sample calls of the shading models
template <bool TEX>
__device__ V3 environment_color(const DevScene &S, V3 dir)
{
    if (!TEX || S.env_map.texture == RT_MAP_NONE) return ld3(S.env);
    // the library's two departures from the reference's undefined results (rt_mi355x.h): asinf's argument is clamped, and a ray
    // straight along +-z (0/0 below) takes x = y = 0
    const float z = asinf(fminf(1.0f, fmaxf(-1.0f, -dir.z))) / (float)M_PI + 0.5f;
    const float l1 = fabsf(dir.x) + fabsf(dir.y);
    const float x = l1 == 0 ? 0.0f : dir.x / l1;
    const float y = l1 == 0 ? 0.0f : dir.y / l1;
    const V3 uvw = mk(0.5f, 0.5f, 0.0f) + (mk(0.5f, 0.5f, 0) * x + mk(-0.5f, 0.5f, 0) * y) * z;
    return textured_color(S, ld3(S.env), S.env_map, uvw);
}
template <bool TEX>
__device__ __forceinline__ void material_colors(const DevScene &S, const Hit &h, const rt_blinn &m, V3 &kd, V3 &ks)
{
    kd = ld3(m.diffuse); ks = ld3(m.specular);
    if (TEX && S.material_maps) {
        const int mi = S.node_material[h.node];
        kd = textured_color(S, kd, S.material_maps[2 * mi], h.uvw);       // diffuse.Sample(uvw, duvw), FIN/main.cpp:531
        ks = textured_color(S, ks, S.material_maps[2 * mi + 1], h.uvw);   // specular.Sample(uvw, duvw), :532
    }
}

// Light::Direction (FIN/include/lights.h:35,51,159)
__device__ __forceinline__ V3 light_direction(const rt_light &l, V3 p)
{
    if (l.type == RT_LIGHT_POINT) return normalize(p - ld3(l.position));
    if (l.type == RT_LIGHT_DIRECT) return ld3(l.direction);
    return mk(0, 0, 0);
}

// Light::Illuminate.  Ambient: intensity (lights.h:34).  Direct: Shadow(Ray(p,-direction))*intensity
// (:50).  Point, FIN (FIN/include/lights.h:67-131): MIN_SHADOW_SAMPLES rays towards position + s*(1,1,1)
// with s = |xv|+|yv| (the reference adds the two LENGTHS to every coordinate, :103), xv,yv a random
// point of the disc of radius `size`; if their mean is neither 0 nor 1, MAX_SHADOW_SAMPLES (16) more
// replace them; result intensity*shadow/dist^2.  Point, P13 (P13/include/lights.h:65-91): 4 rays
// towards position + (dx,dy,dz), radius sqrt(Halton(i,2))*size, two random angles; P12 the same without
// the division by dist^2 (RayTracingProj12/include/lights.h:66-89).
// Each shadow ray is an any-hit query (GenLight::Shadow, FIN/main.cpp:499-513: occluded iff
// 1e-14 < z < t_max).  With size == 0 all samples coincide and ONE query decides them.
template <int MODEL>
__device__ V3 illuminate(const DevScene &S, const rt_params &P, const rt_light &l, int li, V3 p, const RngCtx &rc,
                         const BvhStack &stack, Counters &cnt)
{
    const V3 I = ld3(l.intensity);
    if (l.type == RT_LIGHT_AMBIENT) return I;
    Hit dummy;
    if (l.type == RT_LIGHT_DIRECT) {
        cnt.shadow++;
        bool occ;
        if (MODEL == RT_SHADE_P3) { Hit sh; occ = trace<false, MODEL>(S, p, -ld3(l.direction), BIGFLOAT, sh, stack, cnt) && sh.z > 1e-14f; }
        else occ = trace<true, MODEL>(S, p, -ld3(l.direction), BIGFLOAT, dummy, stack, cnt);
        return I * (occ ? 0.0f : 1.0f);
    }
    const V3 position = ld3(l.position);
    if (MODEL == RT_SHADE_P6 || MODEL == RT_SHADE_P3) {
        // PointLight::Illuminate of P6/P3 (include/lights.h:61): Shadow(Ray(p,position-p),1) * intensity.
        // P3's spheres have no bias: the CLOSEST hit decides (z in (1e-14, 1)), an any-hit would not do
        cnt.shadow++;
        bool occ;
        if (MODEL == RT_SHADE_P3) { Hit sh; occ = trace<false, MODEL>(S, p, position - p, BIGFLOAT, sh, stack, cnt) && sh.z > 1e-14f && sh.z < 1.0f; }
        else occ = trace<true, MODEL>(S, p, position - p, 1.0f, dummy, stack, cnt);
        return I * (occ ? 0.0f : 1.0f);
    }
    const int ns = P.shadow_samples > 0 ? P.shadow_samples : 4;
    if (l.size == 0) {
        cnt.shadow++;
        const bool occ = trace<true, MODEL>(S, p, position - p, 1.0f, dummy, stack, cnt);
        float coefsum = 0.0f;
        for (int i = 0; i < ns; i++) coefsum += occ ? 0.0f : 1.0f;     // the ns identical samples
        if (MODEL == RT_SHADE_P12) return (I * coefsum) / (float)ns;    // no fall-off yet in RayTracingProj12 (include/lights.h:86-88)
        if (MODEL != RT_SHADE_FIN) return ((I * coefsum) / (float)ns) / len2(p - position);
        const float shadow = coefsum / (float)ns;
        return (I * shadow) / len2(p - position);                       // lights.h:130
    }
    if (MODEL != RT_SHADE_FIN) {
        float coef = 0.0f;
        for (int i = 0; i < ns; i++) {
            float u0, u1;
            rng2(rc, RNG_SHADOW, (uint32_t)(li * 64 + i), u0, u1);
            float r = halton(i, 2);
            r = sqrtf(r) * l.size;
            const float theta = (float)(M_PI * 2.0 * (double)u0);
            const float gam = (float)(M_PI * (double)u1);
            const float dx = r * sinf(gam) * cosf(theta), dy = r * sinf(gam) * sinf(theta), dz = r * cosf(gam);
            const V3 lp = mk(dx, dy, dz) + position;
            cnt.shadow++;
            coef += trace<true, MODEL>(S, p, lp - p, 1.0f, dummy, stack, cnt) ? 0.0f : 1.0f;
        }
        if (MODEL == RT_SHADE_P12) return (I * coef) / (float)ns;       // RayTracingProj12/include/lights.h:86-88: avg_shadow, undivided
        return ((I * coef) / (float)ns) / len2(p - position);          // P13/include/lights.h:86-90: inverse square fall-off
    }
    const V3 dir = position - p;
    V3 v1 = dot(dir, mk(1, 0, 0)) > 0.8f ? cross(mk(0, 1, 0), dir) : cross(mk(1, 0, 0), dir);
    V3 v2 = cross(v1, dir);
    v2 = normalize(v2);
    v1 = normalize(v1);
    float shadow = 0.0f;
    for (int i = 0; i < ns; i++) {
        float u0, u1;
        rng2(rc, RNG_SHADOW, (uint32_t)(li * 64 + i), u0, u1);
        const float rRadius = sqrtf(u0) * l.size;
        const float rAngle = (float)((double)u1 * (2.0 * M_PI));
        const float xv = rRadius * cosf(rAngle), yv = rRadius * sinf(rAngle);
        const float lx = sqrtf(len2(v1 * xv)), ly = sqrtf(len2(v2 * yv));
        const V3 tgt = mk(position.x + lx + ly, position.y + lx + ly, position.z + lx + ly);
        cnt.shadow++;
        shadow += trace<true, MODEL>(S, p, tgt - p, 1.0f, dummy, stack, cnt) ? 0.0f : 1.0f;
    }
    shadow /= (float)ns;
    if (shadow != 0.0f && shadow != 1.0f) {
        shadow = 0.0f;
        for (int i = 0; i < 16; i++) {                                  // MAX_SHADOW_SAMPLES
            float u0, u1;
            rng2(rc, RNG_SHADOW, (uint32_t)(li * 64 + 32 + i), u0, u1);
            const float rRadius = sqrtf(u0) * l.size;
            const float rAngle = (float)((double)u1 * (2.0 * M_PI));
            const float xv = rRadius * cosf(rAngle), yv = rRadius * sinf(rAngle);
            const float lx = sqrtf(len2(v1 * (-xv))), ly = sqrtf(len2(v2 * (-yv)));
            const V3 tgt = mk(position.x + lx + ly, position.y + lx + ly, position.z + lx + ly);
            cnt.shadow++;
            shadow += trace<true, MODEL>(S, p, tgt - p, 1.0f, dummy, stack, cnt) ? 0.0f : 1.0f;
        }
        shadow /= 16.0f;
    }
    return (I * shadow) / len2(p - position);
}

template <bool FX = false>
__device__ __forceinline__ void add_sample(const ShadeCtx &C, uint32_t slot, V3 c, bool primary)
{
    float *dst = C.W.sample_rgb + 3 * (size_t)slot;
    if (primary) { dst[0] = c.x; dst[1] = c.y; dst[2] = c.z; }
    else if constexpr (FX) fx_add(C.fx + 3 * (size_t)slot, c.x, c.y, c.z);
    else { atomicAdd(dst, c.x); atomicAdd(dst + 1, c.y); atomicAdd(dst + 2, c.z); }
}

template <bool SIDE = false, bool TWO_ENDED = false>
__device__ __forceinline__ void push_ray(const ShadeCtx &C, bool pred, V3 o, V3 d, V3 thr, V3 absorb,
                                         uint32_t slot, int bounce, uint32_t kind, uint32_t node, uint32_t sample,
                                         V3 side_dir = V3{0, 0, 0}, V3 side_K = V3{0, 0, 0}, uint32_t spec = 0, uint32_t mat = 0)
{
    if (!SIDE && C.lds_count) {
        if constexpr (TWO_ENDED) {
            // two stacks in one array, keyed by the kind of ray (side 0: reflection rays grow up from 0, side 1: refraction and hemisphere
            // rays grow down from the top); ONE packed counter (low half: side 0, high half: side 1) so that an add sees both fills
            const uint32_t side = kind == KIND_REFLECT ? 0u : 1u;
            bool stored = false;
            for (uint32_t sd = 0; sd < 2; sd++) {
                const bool mine = pred && side == sd;
                const unsigned long long mask = ballot64(mine);
                if (!mask) continue;
                const int lane = __lane_id();
                const int leader = __ffsll((long long)mask) - 1;
                const uint32_t n = (uint32_t)__popcll(mask), sh = 16u * sd;
                uint32_t base = 0, room = 0;
                if (lane == leader) {
                    const uint32_t old = atomicAdd(C.lds_count, n << sh);
                    base = (old >> sh) & 0xFFFFu;
                    const uint32_t fill = (old & 0xFFFFu) + (old >> 16);
                    room = fill >= C.lds_cap ? 0u : C.lds_cap - fill;
                    if (room < n) atomicSub(C.lds_count, (n - room) << sh);      // only what was stored counts
                }
                base = __shfl(base, leader); room = __shfl(room, leader);
                const uint32_t off = lanes_below(mask);
                if (mine && off < room) {
                    const uint32_t at = sd ? C.lds_cap - 1u - (base + off) : base + off;
                    C.lds_a[at] = make_float4(o.x, o.y, o.z, d.x);
                    C.lds_b[at] = make_float4(d.y, d.z, thr.x, thr.y);
                    C.lds_c[at] = make_float4(thr.z, __uint_as_float(slot), __uint_as_float((uint32_t)bounce | (kind << 4) | (spec << 8) | (mat << 16)), __uint_as_float(node));
                    stored = true;
                }
            }
            pred = pred && !stored;
            if (!__any(pred)) return;
        } else {
            // the wave's own stack first (LDS atomic, one per wave); what does not fit goes to the global queue
            const uint32_t at = wave_push(pred, C.lds_count);
            if (pred && at < C.lds_cap) {
                C.lds_a[at] = make_float4(o.x, o.y, o.z, d.x);
                C.lds_b[at] = make_float4(d.y, d.z, thr.x, thr.y);
                C.lds_c[at] = make_float4(thr.z, __uint_as_float(slot), __uint_as_float((uint32_t)bounce | (kind << 4) | (spec << 8) | (mat << 16)), __uint_as_float(node));
            }
            pred = pred && at >= C.lds_cap;
            if (!__any(pred)) return;
        }
    }
    const uint32_t idx = wave_push(pred, C.qout_count);
    if (pred) {
        if (idx < C.qout.cap) {
            C.qout.a[idx] = make_float4(o.x, o.y, o.z, d.x);
            C.qout.b[idx] = make_float4(d.y, d.z, thr.x, thr.y);
            if (SIDE) {
                C.qout.c[idx] = make_float4(thr.z, absorb.x, side_K.y, side_K.z);
                C.qout.e[idx] = make_float4(side_dir.x, side_dir.y, side_dir.z, side_K.x);
            } else C.qout.c[idx] = make_float4(thr.z, absorb.x, absorb.y, absorb.z);
            C.qout.d[idx] = make_uint4(slot, (uint32_t)bounce | (kind << 8) | (spec << 16), node, sample);
        } else atomicAdd(&C.W.stats[ST_AT(ST_QUEUE_OVERFLOW)], 1ull);
    }
}

__device__ __forceinline__ void push_photon_query(const ShadeCtx &C, bool pred, V3 p, V3 N, V3 w, uint32_t slot, bool caustic = false)
{
    const DevPhotonQueue &Q = caustic ? C.W.cq : C.W.pq;
    const uint32_t idx = wave_push(pred, C.W.counts + (caustic ? CNT_CAUSTICQ : CNT_PHOTONQ));
    if (pred) {
        if (idx < Q.cap) {
            Q.qa[idx] = make_float4(p.x, p.y, p.z, N.x);
            Q.qb[idx] = make_float4(N.y, N.z, w.x, w.y);
            Q.qc[idx] = make_float4(w.z, __uint_as_float(slot), 0.f, 0.f);
        } else atomicAdd(&C.W.stats[ST_AT(ST_QUEUE_OVERFLOW)], 1ull);
    }
}

// What one Shade() call produces besides its local colour: up to two child rays with their weights
// and (FIN only) a photon-map query.
struct ShadeOut {
    V3 color;                        // local colour (emission + direct light), before the ray weight
    bool want_refl, want_refr, want_photon;
    V3 rdir, tdir;                   // child directions (reflection is normalised by the caller side)
    V3 rK, tK;                       // child weights relative to this ray
    V3 child_absorb;                 // what the children need to finish their own weight on arrival
    V3 kd, N;                        // photon query: diffuse colour and shading normal
    bool want_side;                  // P6: a reflection ray that exists only if the refraction ray hits
    V3 side_dir, side_K;
    int n_caustic;                   // P13: caustic-map lookups this hit makes (one per light past specount > 2, all identical)
    uint32_t spec_out;               // P13: specount handed to the children
    int n_gi;                        // P12: hemisphere rays to spawn (weights/dirs are drawn at push time)
    V3 gi_x, gi_y, gi_z;             // P12: frame of the hemisphere
    uint32_t mat;                    // index of the hit's material (what child_absorb was read from)
};

// MtlBlinn::Shade, FIN/main.cpp:516-708
template <bool TEX>
__device__ void shade_fin(const DevScene &S, const rt_params &P, const Hit &h, V3 ray_d, int bounce, const RngCtx &rc,
                          ShadeOut &o, const BvhStack &stack, Counters &cnt)
{
    const int mi = S.node_material[h.node];
    const rt_blinn &m = S.materials[mi];
    // what the lowering found out about this material (RT_MAT_*, rt_dev.h; the argument is at material_class_of in rt_lower.cpp):
    // terms that are exactly +0 for every hit on it are left out below.  A per-lane branch on a per-material value -- the 64
    // samples of a pixel nearly always agree on it
    const uint32_t cls = S.material_class[mi];
    V3 color = ld3(m.emission);                                         // :517
    const V3 p = h.p;
    const V3 N = normalize(h.N);                                        // :521-522
    const V3 direction = normalize(-ray_d);                             // :523-524
    V3 kd, ks;
    material_colors<TEX>(S, h, m, kd, ks);
    const float gloss = m.glossiness;
    const V3 reflection = ld3(m.reflection), refraction = ld3(m.refraction);
    const float ior = m.ior;
    const float coef = S.n_lights == 0 ? 1.0f : 1.0f / S.n_lights;      // :545
    for (int li = 0; li < S.n_lights; li++) {
        const rt_light light = cld_light(S.lights + li);
        // the reference still calls Illuminate (its shadow rays) for a back-face hit but uses the
        // result only for front hits (:551-553): nothing to add, nothing traced
        if (!h.front) continue;
        const V3 Il = illuminate<RT_SHADE_FIN>(S, P, light, li, p, rc, stack, cnt);
        if (light.type != RT_LIGHT_AMBIENT) {
            const V3 intensity = Il * coef;                             // :551
            V3 L = light_direction(light, p) * (float)(-1);             // :556
            L = normalize(L);
            const V3 LpD = L + direction;
            const float cosNL = RMAX(0.f, dot(N, L));
            const V3 diffuse = (kd * intensity) * cosNL;                // :563
            V3 specular = ks * intensity;
            // RT_MAT_NO_SPECULAR: ks is +0, the lobe finite and >= 0, so (ks * intensity) * lobe has the bits of ks * intensity (a
            // zero of either sign, or the NaN of an infinite intensity): H, cosNH and powf are left out, the multiplications
            // around them and the additions below stay, so every sum rounds -- and signs its zeros -- as before.  L == -direction
            // (the light straight behind the hit) is the one case whose lobe is a NaN: it keeps the general path
            if (!(cls & RT_MAT_NO_SPECULAR) || (LpD.x == 0.f && LpD.y == 0.f && LpD.z == 0.f)) {
                const V3 H = normalize(LpD);
                const float cosNH = RMAX(0.f, dot(N, H));
                specular = specular * powf(cosNH, gloss);               // :564 (std::pow(float,float))
            }
            specular = specular * cosNL;
            color = color + (diffuse + specular);                       // :566
        } else {
            color = color + kd * Il;                                    // :568-569
        }
    }
    // :642-693: at bounceCount == BOUNCE the hemisphere loop's result is assigned to a shadowing
    // variable and contributes exactly 0 -- not traced.  :695-705: every other hit adds
    // kd * irradiance * max(0, N.(-dir)); queued for k_gather.
    o.want_photon = (bounce != P.bounce) && S.pm.n_leaves != 0;
    o.color = color; o.kd = kd; o.N = N;
    o.child_absorb = ld3(m.absorption);      // children: K *= Attenuation(absorption, z) on a back-face hit (:620,:632)
    o.mat = (uint32_t)mi;
    // RT_MAT_NO_SPEC_TREE: rK and tK below would be zeros (reflection and refraction are +0, rC is finite), no child ray passes the
    // threshold and nobody reads the directions: rK, tK, rdir, tdir and the two flags keep what shade_path initialised them to
    if (cls & RT_MAT_NO_SPEC_TREE) return;
    // reflection / refraction set-up, :577-610
    float ein = 1, eout = ior;
    if (!h.front) { ein = ior; eout = 1; }
    const float eta = ein / eout;
    const float cosI = dot(N, direction);
    const V3 Y = cosI > 0.f ? N : -N;
    const V3 Z = cross(direction, Y);
    const V3 X = normalize(cross(Y, Z));
    // sqrtf(1 - cosI*cosI) is NaN in the reference when |cosI| exceeds 1 by rounding (:592);
    // clamped at 0 here (documented deviation)
    const float sinI = sqrtf(fmaxf(0.0f, 1 - cosI * cosI));
    const float sinO = RMAX(0.f, RMIN(1.f, sinI * eta));
    const float cosO = sqrtf(1.f - sinO * sinO);
    o.tdir = normalize((-X) * sinO - Y * cosO);                         // :596, tRay.Normalize() :627
    o.rdir = normalize((N * 2.f) * cosI - direction);                   // :597, r.Normalize() :615
    const float C0 = (eta - 1.f) * (eta - 1.f) / ((eta + 1.f) * (eta + 1.f));
    const float rC = C0 + (1.f - C0) * powf(1.f - fabsf(cosI), 5.f);    // :601
    const float tC = 1.f - rC;
    const bool totReflection = (eta * sinI) > 1.001f;                   // materials.h:20
    o.tK = totReflection ? mk(0.f, 0.f, 0.f) : refraction * tC;
    o.rK = totReflection ? (reflection + refraction) : (reflection + refraction * rC);
    const float th = 0.001f;                                            // materials.h:21-22
    o.want_refl = bounce > 0 && (o.rK.x > th || o.rK.y > th || o.rK.z > th);   // :613
    o.want_refr = bounce > 0 && (o.tK.x > th || o.tK.y > th || o.tK.z > th);   // :625
}

// MtlBlinn::Shade, P13/main.cpp:485-756 (reflectionGlossiness == refractionGlossiness == 0).
// all = ambient + direct; all += re_color*reflection; all += refraction*(ra_ratio*absorb*ra_color +
// re_ratio*re_color): the reflection child weighs reflection + refraction*re_ratio, the refraction
// child refraction*ra_ratio*exp(-absorption.r * z_child) (z_child = BIGFLOAT on a miss).
template <int MODEL, bool TEX>
__device__ void shade_p13(const DevScene &S, const rt_params &P, const Hit &h, V3 ray_d, int bounce, const RngCtx &rc,
                          ShadeOut &o, const BvhStack &stack, Counters &cnt, uint32_t spec_in)
{
    constexpr bool p12 = MODEL == RT_SHADE_P12;
    const rt_blinn &m = S.materials[S.node_material[h.node]];
    V3 N = h.N;
    const V3 Pp = h.p;
    V3 Kd, Ks;
    material_colors<TEX>(S, h, m, Kd, Ks);
    const float alpha = m.glossiness;
    V3 ambient = mk(0, 0, 0), diffuse = mk(0, 0, 0);
    uint32_t spec = spec_in;
    int n_caustic = 0;
    for (int i = 0; i < S.n_lights; i++) {
        const rt_light l = cld_light(S.lights + i);
        const V3 Il = illuminate<MODEL>(S, P, l, i, Pp, rc, stack, cnt);
        if (l.type == RT_LIGHT_AMBIENT) ambient = ambient + Il * Kd;                     // :510
        else {
            // the caustic lookup the reference sketches in a comment (:518-533): per non-ambient light, on a photon
            // surface (diffuse.Gray() > 0), once specount has passed 2; specount++ after every such light
            if (gray(ld3(m.diffuse)) > 0 && spec > 2u) n_caustic++;
            spec++;
            V3 L = light_direction(l, Pp) * (float)-1;
            if (!p12) L = normalize(L);                                                   // P13 adds L.Normalize() (:540)
            const V3 V = normalize(-ray_d);
            const V3 H = normalize(L + V);
            const V3 kse = Ks * powf(dot(N, H), alpha) + Kd;                              // :547
            const float theta = dot(N, L);
            diffuse = diffuse + (Il * (theta > 0.0f ? theta : 0.0f)) * kse;               // :551
        }
    }
    o.color = ambient + diffuse;                                                          // :622
    o.spec_out = spec > 255u ? 255u : spec;
    o.n_caustic = (P.caustic_k > 0 && S.cm.n_leaves != 0) ? n_caustic : 0;
    o.n_gi = 0;
    if (p12) {
        // RayTracingProj12 main.cpp:393-448: all = ambient + ((diffuse/pi) + idr)*Kd, idr = mean over the
        // hemisphere rays of childColour * (dir.N): local part here, rays spawned by the caller
        o.color = ambient + (diffuse / (float)M_PI) * Kd;
        if (bounce > 0) {
            o.n_gi = (bounce == P.bounce) ? P.hemisphere_sample : 1;
            o.gi_z = h.N;
            V3 nx = dot(o.gi_z, mk(1, 0, 0)) < 0.4f ? cross(o.gi_z, mk(1, 0, 0)) : cross(o.gi_z, mk(0, 0, 1));
            o.gi_x = normalize(nx);
            o.gi_y = cross(o.gi_z, o.gi_x);
        }
    }
    V3 V = -normalize(ray_d);                                                             // :632
    // glossy reflection: the normal is jittered inside a disc of radius reflectionGlossiness (:635-647)
    V3 Nr = N;
    if (m.reflection_glossiness != 0) {
        const V3 newx = cross(Nr, mk(1, 0, 0));
        const V3 newy = cross(Nr, newx);
        float u0, u1;
        rng2(rc, RNG_GLOSSR, 0u, u0, u1);
        const float r = sqrtf(u0) * m.reflection_glossiness;
        const float theta = (float)(M_PI * 2.0 * (double)u1);
        Nr = normalize(Nr + (newx * (r * cosf(theta)) + newy * (r * sinf(theta))));
    }
    const float costheta = fminf(fmaxf(dot(Nr, V), -1.0f), 1.0f);                         // clamp :648
    o.rdir = normalize(Nr * (2 * costheta) - V);                                          // :649, :652
    // refraction block :671-751 (starts again from the unjittered normal, :672)
    N = h.N;
    if (m.refraction_glossiness != 0) {                                                   // :673-686
        const V3 newx = cross(N, mk(1, 0, 0));
        const V3 newy = cross(N, newx);
        float u0, u1;
        rng2(rc, RNG_GLOSST, 0u, u0, u1);
        const float r = sqrtf(u0) * m.refraction_glossiness;
        const float theta = (float)(M_PI * 2.0 * (double)u1);
        N = normalize(N + (newx * (r * cosf(theta)) + newy * (r * sinf(theta))));
    }
    V = normalize(V);
    const float costheta1 = fabsf(dot(V, N));
    const float sintheta1 = sqrtf(RMAX(0.0f, 1 - (costheta1 * costheta1)));
    float n1 = 1.0f, n2 = 1.0f;
    if (h.front) n2 = m.ior; else { n1 = m.ior; N = -N; }
    const float ratio_n = n1 / n2;
    const float sintheta2 = ratio_n * sintheta1;
    float re_ratio = 0.0f, ra_ratio = 0.0f;
    o.tdir = mk(0, 0, 1);
    bool refr_ok = false;
    if (sintheta2 <= 1.0f) {
        const float costheta2 = sqrtf(RMAX(0.0f, 1 - (sintheta2 * sintheta2)));
        V3 Sv = cross(N, cross(N, V));
        N = normalize(N);
        Sv = normalize(Sv);
        o.tdir = (-N) * costheta2 + Sv * sintheta2;                                       // not normalised (:718-720)
        float R0 = (n1 - n2) / (n1 + n2);
        R0 = R0 * R0;
        const double tmp = 1.0 - costheta1;
        re_ratio = (float)(R0 + (1.0 - R0) * pow(tmp, 5.0));                              // :733 (double)
        ra_ratio = (float)(1.0 - re_ratio);
        refr_ok = true;
    } else re_ratio = 1.0f;
    const V3 reflection = ld3(m.reflection), refraction = ld3(m.refraction);
    o.rK = reflection + refraction * re_ratio;
    o.tK = refraction * ra_ratio;
    o.want_refl = bounce > 0;
    o.want_refr = bounce > 0 && refr_ok;
    o.want_photon = false;
    o.kd = Kd; o.N = h.N;
    o.child_absorb = mk(m.absorption[0], 0, 0);          // refraction child: *= exp(-absorption.r * z) (:728)
    o.mat = (uint32_t)S.node_material[h.node];
}

// MtlBlinn::Shade of RayTracingProj3, main.cpp:152-190: ambient + Blinn with V = camera.pos - p (all P3
// rays start at the camera, so camera.pos is the ray origin); no children
template <bool TEX>
__device__ void shade_p3(const DevScene &S, const rt_params &P, const Hit &h, V3 ray_o, const RngCtx &rc, ShadeOut &o,
                         const BvhStack &stack, Counters &cnt)
{
    const rt_blinn &m = S.materials[S.node_material[h.node]];
    const V3 N = h.N, Pp = h.p;
    V3 Kd, Ks;
    material_colors<TEX>(S, h, m, Kd, Ks);
    V3 ambient = mk(0, 0, 0), diffuse = mk(0, 0, 0);
    for (int i = 0; i < S.n_lights; i++) {
        const rt_light l = cld_light(S.lights + i);
        const V3 Il = illuminate<RT_SHADE_P3>(S, P, l, i, Pp, rc, stack, cnt);
        if (l.type == RT_LIGHT_AMBIENT) ambient = ambient + Il * Kd;
        else {
            const V3 L = light_direction(l, Pp) * (float)-1;
            const V3 V = normalize(ray_o - Pp);
            const V3 LpV = L + V;
            const V3 H = normalize(LpV / sqrtf(len2(LpV)));
            const V3 kse = Ks * powf(dot(N, H), m.glossiness) + Kd;
            const float theta = dot(N, L);
            diffuse = diffuse + (Il * (theta > 0 ? theta : 0.0f)) * kse;
        }
    }
    o.color = ambient + diffuse;
    o.kd = Kd; o.N = N;
}

// MtlBlinn::Shade of RayTracingProj6, main.cpp:175-340.  Children: a reflection ray only when
// reflection.Gray() > 0 (weight reflection); a refraction ray only when refraction.Gray() > 0 (weight
// refraction*ra_ratio*exp(-absorption.r*z)); and refraction*re_ratio times a reflection colour that the
// reference adds ONLY IF THE REFRACTION RAY HIT something (re_ratio is set inside that branch, :296-303) --
// or under total internal reflection.  That conditional ray travels with the refraction ray as a
// "side" ray and is spawned when the refraction ray reports a hit.  Misses add nothing (no environment).
template <bool TEX>
__device__ void shade_p6(const DevScene &S, const rt_params &P, const Hit &h, V3 ray_d, int bounce, const RngCtx &rc,
                         ShadeOut &o, const BvhStack &stack, Counters &cnt)
{
    const rt_blinn &m = S.materials[S.node_material[h.node]];
    V3 N = h.N;
    const V3 Pp = h.p;
    V3 Kd, Ks;
    material_colors<TEX>(S, h, m, Kd, Ks);
    const V3 reflection = ld3(m.reflection), refraction = ld3(m.refraction);
    V3 ambient = mk(0, 0, 0), diffuse = mk(0, 0, 0);
    for (int i = 0; i < S.n_lights; i++) {
        const rt_light l = cld_light(S.lights + i);
        const V3 Il = illuminate<RT_SHADE_P6>(S, P, l, i, Pp, rc, stack, cnt);
        if (l.type == RT_LIGHT_AMBIENT) ambient = ambient + Il * Kd;                          // :199
        else {
            const V3 L = light_direction(l, Pp) * (float)-1;
            const V3 V = normalize(-ray_d);
            const V3 H = normalize(L + V);
            const V3 kse = Ks * powf(dot(N, H), m.glossiness) + Kd;                           // :210
            const float theta = dot(N, L);
            diffuse = diffuse + (Il * (theta > 0.0f ? theta : 0.0f)) * kse;                   // :214
        }
    }
    o.color = ambient + diffuse;
    o.kd = Kd; o.N = h.N;
    V3 V = -normalize(ray_d);                                                                 // :223
    const bool has_re = gray(reflection) > 0;
    const float ct0 = fminf(fmaxf(dot(N, V), -1.0f), 1.0f);
    const V3 R1 = normalize(N * (2 * ct0) - V);                                               // :227-229
    o.rdir = R1;
    o.rK = reflection;
    o.want_refl = has_re && bounce > 0;
    o.want_refr = false; o.want_side = false;
    o.tK = mk(0, 0, 0); o.tdir = mk(0, 0, 1); o.side_dir = mk(0, 0, 1); o.side_K = mk(0, 0, 0);
    o.child_absorb = mk(m.absorption[0], 0, 0);
    if (gray(refraction) > 0 && bounce > 0) {                                                 // :246
        V = normalize(V);
        const float costheta1 = fabsf(dot(V, N));
        const float sintheta1 = sqrtf(RMAX(0.0f, 1 - (costheta1 * costheta1)));
        float n1 = 1.0f, n2 = 1.0f;
        if (h.front) n2 = m.ior; else { n1 = m.ior; N = -h.N; }
        const float ratio_n = n1 / n2;
        const float sintheta2 = ratio_n * sintheta1;
        float re_ratio, ra_ratio = 0.0f;
        const bool transmit = sintheta2 <= 1.0f;
        if (transmit) {
            const float costheta2 = sqrtf(RMAX(0.0f, 1 - (sintheta2 * sintheta2)));
            V3 Sv = cross(N, cross(N, V));
            N = normalize(N);
            Sv = normalize(Sv);
            o.tdir = (-N) * costheta2 + Sv * sintheta2;
            float R0 = (n1 - n2) / (n1 + n2);
            R0 = R0 * R0;
            const double tmp = 1.0 - costheta1;
            re_ratio = (float)(R0 + (1.0 - R0) * pow(tmp, 5.0));                              // if the refraction ray hits
            ra_ratio = (float)(1.0 - re_ratio);
            o.tK = refraction * ra_ratio;
            o.want_refr = true;
        } else re_ratio = 1.0f;                                                               // total internal reflection
        // the reflection colour that refraction*re_ratio multiplies: the first reflection ray again when the
        // material is reflective (:310), else a second ray about the (flipped, normalised) normal, direction
        // NOT normalised (:314-319)
        V3 sdir = R1;
        if (!has_re) { const float ct = fminf(fmaxf(dot(N, V), -1.0f), 1.0f); sdir = N * (2 * ct) - V; }
        const V3 sK = refraction * re_ratio;
        if (re_ratio > 0.0f || has_re) {
            if (transmit) { o.want_side = true; o.side_dir = sdir; o.side_K = sK; }          // only if the refraction ray hits
            else if (has_re) o.rK = reflection + sK;                                          // same ray as the first reflection
            else { o.want_refl = true; o.rdir = sdir; o.rK = sK; }
        }
    }
}

// One node of the ray tree: Trace + MtlBlinn::Shade with the recursion unrolled into queue pushes.
// Shade is linear in its children (color += K*child), so a ray carries the product `thr` of the K
// factors above it and adds thr*local colour to its sample; the part of a child's K that depends on
// the child's own hit (FIN: Attenuation(parent absorption, z) on a back-face hit, FIN/main.cpp:620,
// 632; P13: exp(-absorption.r*z) on the refraction child, P13/main.cpp:728) is applied on arrival.
template <int MODEL, bool TEX, bool FX = false>
__device__ void shade_path(const ShadeCtx &C, const PathIn &in, bool active, const BvhStack &stack, Counters &cnt)
{
    const DevScene &S = C.S;
    const rt_params &P = C.P;
    constexpr bool p13 = MODEL == RT_SHADE_P13 || MODEL == RT_SHADE_P12;     // they share lights and the ray tree
    Hit h;
    bool hit = false;
    if (active) hit = trace<false, MODEL, TEX>(S, in.o, in.d, BIGFLOAT, h, stack, cnt);
    V3 thr = in.thr;
    ShadeOut o;
    o.want_refl = o.want_refr = o.want_photon = false;
    o.rdir = o.tdir = mk(0, 0, 1); o.rK = o.tK = o.child_absorb = o.kd = o.N = mk(0, 0, 0);
    o.n_gi = 0; o.gi_x = o.gi_y = o.gi_z = mk(0, 0, 1);
    o.want_side = false; o.side_dir = mk(0, 0, 1); o.side_K = mk(0, 0, 0);
    o.n_caustic = 0; o.spec_out = in.spec; o.mat = 0;
    constexpr bool p6 = MODEL == RT_SHADE_P6, p3 = MODEL == RT_SHADE_P3;
    // the workgroup-shared ray stack of k_wavefront is two-ended (push_ray); a wave's own stack in the P12 rounds is plain
    constexpr bool TWO = !(RT_WF_PERWAVE && MODEL == RT_SHADE_P12);
    bool spawn_side = false;
    if (active && !in.primary) {
        if (p6) {
            // refraction ray of P6: weight *= exp(-absorption.r*z) when it hits (main.cpp:296); its side ray
            // (the reflection that refraction*re_ratio multiplies) exists only in that case
            if (in.kind == KIND_REFRACT && hit) { thr = thr * expf(-in.absorb.x * h.z); spawn_side = (in.side_K.x != 0.f || in.side_K.y != 0.f || in.side_K.z != 0.f); }
        } else if (p13) { if (in.kind == KIND_REFRACT) thr = thr * expf(-in.absorb.x * (hit ? h.z : BIGFLOAT)); }   // not for GI rays
        else if (hit && !h.front) thr = thr * attenuation(in.absorb, h.z);
    }
    if (active && !hit) {
        if (in.primary) C.W.sample_hit[in.slot] = 0;
        // a refraction ray that leaves the scene sees the environment (FIN/main.cpp:635); in P13 so
        // does a reflection ray (P13/main.cpp:660-662)
        else if (!p6 && !p3 && (in.kind != KIND_REFLECT || p13)) add_sample<FX>(C, in.slot, thr * environment_color<TEX>(S, in.d), false);
    }
    if (active && hit) {
        if (in.primary) { C.W.sample_hit[in.slot] = 1; C.W.sample_z[in.slot] = h.z; }
        RngCtx rc; rc.seed = P.seed; rc.sample = in.sample; rc.node = in.node;
        if (p3) shade_p3<TEX>(S, P, h, in.o, rc, o, stack, cnt);
        else if (p6) shade_p6<TEX>(S, P, h, in.d, in.bounce, rc, o, stack, cnt);
        else if (p13) shade_p13<MODEL, TEX>(S, P, h, in.d, in.bounce, rc, o, stack, cnt, in.spec);
        else shade_fin<TEX>(S, P, h, in.d, in.bounce, rc, o, stack, cnt);
        add_sample<FX>(C, in.slot, thr * o.color, in.primary);
        // a child (or query) whose accumulated weight is exactly zero cannot change the pixel
        const V3 wr = thr * o.rK, wt = thr * o.tK, wp = thr * o.kd;
        o.want_refl = o.want_refl && (wr.x != 0.f || wr.y != 0.f || wr.z != 0.f);
        o.want_refr = o.want_refr && (wt.x != 0.f || wt.y != 0.f || wt.z != 0.f);
        o.want_photon = o.want_photon && (wp.x != 0.f || wp.y != 0.f || wp.z != 0.f);
    }
    // pushes are wave-collective: every lane of the wave reaches them
    push_ray<false, TWO>(C, o.want_refl, h.p, o.rdir, thr * o.rK, o.child_absorb, in.slot, in.bounce - 1, KIND_REFLECT,
             child_node(in.node, 1u), in.sample, mk(0, 0, 0), mk(0, 0, 0), o.spec_out, o.mat);
    if (p6) {
        const V3 sK = thr * o.side_K;
        push_ray<true>(C, o.want_refr, h.p, o.tdir, thr * o.tK, o.child_absorb, in.slot, in.bounce - 1, KIND_REFRACT,
                       child_node(in.node, 2u), in.sample, o.side_dir, o.want_side ? sK : mk(0, 0, 0));
        // the side ray of an arriving refraction ray: same origin and level as that ray
        push_ray<false, TWO>(C, spawn_side, in.o, in.side_dir, in.side_K, mk(0, 0, 0), in.slot, in.bounce, KIND_REFLECT, child_node(in.node, 4u), in.sample);
    } else
    push_ray<false, TWO>(C, o.want_refr, h.p, o.tdir, thr * o.tK, o.child_absorb, in.slot, in.bounce - 1, KIND_REFRACT,
             child_node(in.node, 2u), in.sample, mk(0, 0, 0), mk(0, 0, 0), o.spec_out, o.mat);
    push_photon_query(C, o.want_photon, h.p, o.N, thr * o.kd, in.slot);
    if (p13) {
        // cau_Color += Kd * causticrad * theta, once per counted light (P13/main.cpp:518-531): one query, weight x count
        const V3 wc = (thr * o.kd) * (float)o.n_caustic;
        push_photon_query(C, active && hit && o.n_caustic > 0 && (wc.x != 0.f || wc.y != 0.f || wc.z != 0.f), h.p, o.N, wc, in.slot, true);
    }
    if (MODEL == RT_SHADE_P12) {
        // hemisphere rays: idr += childColour * (dir.N) / Nofsample, times Kd (main.cpp:420-446)
        const int n_max = __reduce_max_sync_compat(o.n_gi);
        for (int i = 0; i < n_max; i++) {
            bool want = i < o.n_gi;
            V3 hd = mk(0, 0, 1), w = mk(0, 0, 0);
            if (want) {
                RngCtx rc; rc.seed = P.seed; rc.sample = in.sample; rc.node = in.node;
                float u0, u1;
                rng2(rc, RNG_GI, (uint32_t)i, u0, u1);
                const float phi = (float)(2 * M_PI * (double)u0);
                const float cosphi = cosf(phi);
                const float sintheta = sqrtf(u1), costheta = sqrtf(1 - u1);
                hd = normalize(o.gi_x * (sintheta * cosphi) + o.gi_y * (sintheta * sinf(phi)) + o.gi_z * costheta);
                const float dotN_wi = dot(hd, o.gi_z);
                w = thr * (o.kd * (dotN_wi / (float)o.n_gi));
                hd = normalize(hd);                        // Ray_idr.dir.Normalize() (:433)
                want = (w.x != 0.f || w.y != 0.f || w.z != 0.f);
            }
            push_ray<false, TWO>(C, want, h.p, hd, w, mk(0, 0, 0), in.slot, in.bounce - 1, KIND_GI, child_node(in.node, 3u + (uint32_t)i), in.sample, mk(0, 0, 0), mk(0, 0, 0), o.spec_out);
        }
    }
}

// The whole workgroup calls this once, at the end of its kernel.  The waves' counts meet in LDS and ONE thread per counter adds them
// to the statistics block: a wave-level flush was 7 device-scope atomics per wave on one 128-byte line, all of them when the launch
// drains -- 21 000 per k_wavefront launch queueing at the memory side while the kernel waits to retire (r4: 0.4 ms of the Cornell
// frame's tracer, 0.3 of its gather).  The block's counters sit RT_STAT_STRIDE apart for the same reason (rt_dev.h).
__device__ __forceinline__ void flush_counters(unsigned long long *stats, const Counters &c, uint32_t nprim, uint32_t nrefl, uint32_t nrefr)
{
    __shared__ unsigned long long s_acc[7];
    if (threadIdx.x < 7) s_acc[threadIdx.x] = 0;
    __syncthreads();
    uint32_t v[7] = {c.inst, c.nodes, c.tris, c.shadow, nprim, nrefl, nrefr};
#pragma unroll
    for (int i = 0; i < 7; i++) {
        uint32_t x = v[i];
        for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
        v[i] = x;
    }
    if (__lane_id() == 0) {
#pragma unroll
        for (int i = 0; i < 7; i++) if (v[i]) atomicAdd(&s_acc[i], (unsigned long long)v[i]);
    }
    __syncthreads();
    if (threadIdx.x < 7) {
        const int slot = threadIdx.x == 0 ? ST_INSTANCE_VISITS : threadIdx.x == 1 ? ST_BVH_NODES : threadIdx.x == 2 ? ST_TRIS : threadIdx.x == 3 ? ST_RAYS_SHADOW
                       : threadIdx.x == 4 ? ST_RAYS_PRIMARY : threadIdx.x == 5 ? ST_RAYS_REFLECT : ST_RAYS_REFRACT;
        const unsigned long long x = s_acc[threadIdx.x];
        if (x) atomicAdd(&stats[ST_AT(slot)], x);
    }
}

// ------------------------------------------------------------------------------------------------
// K1: one thread per (pixel, sample).  generateSample + ray build, FIN/main.cpp:147-162, 281-292
// (dof == 0).  Lanes of a wave hold consecutive samples of the same pixel(s): coherent traversal.
//   mode 0: pixels q0..q0+npix of the chunk, samples j0..j0+ns
//   mode 1: pixels from W.pixel_list[0..counts[CNT_PIXLIST]), samples j0..j0+ns   (second batch)
//   mode 2: rays[] supplied by the caller, one sample each (rt_shade_rays)
// ------------------------------------------------------------------------------------------------
struct PrimaryArgs {
    DevCamera cam; DevTiles tiles;
    uint32_t q0, npix;           // chunk range (mode 0)
    int j0, ns, max_sample, mode;
    const float *rays;           // mode 2
    FastDiv div_ns;
    uint32_t lds_rays;           // k_wavefront: entries of the LDS ray stack to use (0: all of them; the test hook RT_WF_LDS_RAYS makes the stack overflow on small frames)
    DevRayQueue qsrc;            // mode 3 (k_wavefront only): the work is a ray queue (count in *qsrc_count), not primary samples
    const uint32_t *qsrc_count;
};

// Register budget: the texture-free instantiations are held to 168 VGPRs (3 waves/SIMD; a few values
// spill to scratch) -- measured 4 % faster on MI355X than letting them grow to 192 VGPRs at 2 waves.
// sample gid of this launch -> its primary ray (generateSample + ray build, FIN/main.cpp:147-162, 281-292); false = no such sample
__device__ __forceinline__ bool primary_setup(const ShadeCtx &C, const PrimaryArgs &A, unsigned long long gid, unsigned long long total,
                                              bool h_table, const float *s_h2, const float *s_h3, PathIn &in)
{
    in.thr = mk(1.f, 1.f, 1.f); in.absorb = mk(0, 0, 0); in.bounce = C.P.bounce; in.kind = KIND_REFLECT; in.primary = true;
    in.o = mk(0, 0, 0); in.d = mk(0, 0, 1); in.slot = 0; in.node = 1; in.sample = 0;
    in.side_dir = mk(0, 0, 1); in.side_K = mk(0, 0, 0); in.spec = 0;
    if (gid >= total) return false;
    uint32_t pi, jj;
    if (total <= 0xFFFFFFFFull) { pi = fastdiv((uint32_t)gid, A.div_ns); jj = (uint32_t)gid - pi * (uint32_t)A.ns; }
    else { pi = (uint32_t)(gid / (unsigned long long)A.ns); jj = (uint32_t)(gid % (unsigned long long)A.ns); }
    const int j = A.j0 + (int)jj;
    const uint32_t ql = (A.mode == 1) ? C.W.pixel_list[pi] : pi;      // chunk-local pixel
    in.slot = ql * (uint32_t)A.max_sample + (uint32_t)j;
    if (A.mode == 2) {
        const float *r = A.rays + 6 * (size_t)ql;
        in.o = ld3(r); in.d = ld3(r + 3);
        in.sample = A.q0 + ql;                     // caller's ray index
        return true;
    }
    int x, y;
    if (!pixel_of(A.tiles, A.cam, A.q0 + ql, x, y)) return false;
    const V3 tmp = mk(x * A.cam.u, y * A.cam.v, 0) + ld3(A.cam.b);     // :235-236
    float sx = (h_table ? s_h2[jj] : halton(j, 2)) * A.cam.u;          // :153
    float sy = A.cam.v * (h_table ? s_h3[jj] : halton(j, 3));          // :154
    sx += tmp.x; sy += tmp.y;
    const V3 sample = mk(sx, sy, tmp.z);
    const uint32_t pixel_id = (uint32_t)y * (uint32_t)A.cam.width + (uint32_t)x;
    in.sample = pixel_id * (uint32_t)A.max_sample + (uint32_t)j;
    V3 d_campos = mk(0, 0, 0);
    if (A.cam.dof != 0) {
        // :246-262: a table of CAM_SAMPLE lens points per pixel (radius sqrt(Halton(i,2))*dof,
        // random angle), of which every sample picks one at random (:284)
        RngCtx pc; pc.seed = C.P.seed; pc.sample = in.sample; pc.node = 0;
        float u0, u1;
        rng2(pc, RNG_PICK, 0u, u0, u1);
        int pick = (int)(u0 * 64.0f);
        pick = pick > 63 ? 63 : pick;
        RngCtx lc; lc.seed = C.P.seed; lc.sample = pixel_id; lc.node = 0;
        rng2(lc, RNG_LENS, (uint32_t)(pick + 1), u0, u1);
        float r = halton(pick + 1, 2);
        r = sqrtf(r) * A.cam.dof;
        const float theta = (float)(M_PI * 2.0 * (double)u0);
        d_campos = mmul(A.cam.m, mk(r * cosf(theta), r * sinf(theta), 0));
    }
    in.o = ld3(A.cam.pos) + d_campos;                                  // :288
    in.d = normalize(mmul(A.cam.m, sample) - d_campos);                // :289-292
    return true;
}

#endif
