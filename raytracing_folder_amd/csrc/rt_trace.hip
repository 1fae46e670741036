// rt_trace.hip -- the kernels that trace and never shade (gfx950 / CDNA4, wave64), with their launches:
//
//   k_trace         K2  closest-hit only: the parity entry point rt_trace_rays (rtk_launch_trace)
//   k_photon_trace      the photon pass, one thread per emission attempt (rtk_launch_photon_trace)
//
// Includes rt_trace.h (geometry and traversal) and nothing of the shading layer (rt_shade.h).
#include <hip/hip_runtime.h>
#include <math.h>
#include "rt_trace.h"

// K2 alone: n closest-hit queries (rt_trace_rays)
template <int MODEL>
__global__ __launch_bounds__(RT_BLOCK) void k_trace(DevScene S, const float *rays, long long n,
                                                    uint8_t *hit, float *z, float *p, float *N, int32_t *node, uint8_t *front)
{
    __shared__ uint32_t s_stack[RT_BVH_STACK * RT_BLOCK];
    const BvhStack stack = bvh_stack(s_stack, RT_BVH_STACK, S.bvh_spill);
    Counters cnt = {0, 0, 0, 0, 0};
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        Hit h;
        h.z = BIGFLOAT; h.p = mk(0, 0, 0); h.N = mk(0, 0, 0); h.node = -1; h.front = 1;
        const bool ok = trace<false, MODEL>(S, ld3(rays + 6 * i), ld3(rays + 6 * i + 3), BIGFLOAT, h, stack, cnt);
        hit[i] = ok ? 1 : 0;
        z[i] = ok ? h.z : BIGFLOAT;
        p[3 * i] = h.p.x; p[3 * i + 1] = h.p.y; p[3 * i + 2] = h.p.z;
        N[3 * i] = h.N.x; N[3 * i + 1] = h.N.y; N[3 * i + 2] = h.N.z;
        node[i] = ok ? h.node : -1;
        front[i] = (uint8_t)h.front;
    }
}

// ------------------------------------------------------------------------------------------------
// Photon pass: generatePhotonMap / PhotonTracing (FIN/main.cpp:350-459),
// PointLight::RandomPhoton (:489-497) and MtlBlinn::RandomPhotonBounce (FIN/include/materials.h:
// 99-256), one thread per emission attempt.  The reference draws from libc rand(); here every draw
// is Philox-4x32-10 keyed by the seed and counted by (attempt index, draw index), so the photon set
// is a pure function of (scene, seed) whatever the scheduling -- and the CPU oracle, using the same
// generator, reproduces it photon for photon (up to libm rounding).
// ------------------------------------------------------------------------------------------------
struct Philox {
    uint32_t key0, key1, c0, c1, blk; uint32_t o0, o1, o2, o3; int used;
    __host__ __device__ void refill()
    {
        uint32_t x0 = c0, x1 = c1, x2 = blk, x3 = 0, k0 = key0, k1 = key1;
        for (int r = 0; r < 10; r++) {
            const unsigned long long p0 = (unsigned long long)0xD2511F53u * x0, p1 = (unsigned long long)0xCD9E8D57u * x2;
            const uint32_t y0 = (uint32_t)(p1 >> 32) ^ x1 ^ k0, y1 = (uint32_t)p1, y2 = (uint32_t)(p0 >> 32) ^ x3 ^ k1, y3 = (uint32_t)p0;
            x0 = y0; x1 = y1; x2 = y2; x3 = y3;
            k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
        }
        o0 = x0; o1 = x1; o2 = x2; o3 = x3;
        blk++; used = 0;
    }
    // uniform in [0,1): stands in for rand() / (float) RAND_MAX
    __host__ __device__ float next()
    {
        if (used >= 4) refill();
        const uint32_t v = used == 0 ? o0 : (used == 1 ? o1 : (used == 2 ? o2 : o3));
        used++;
        return (float)(v >> 8) * (1.0f / 16777216.0f);
    }
};

// (PhotonArgs: rt_launch.h)

// MtlBlinn::RandomPhotonBounce, FIN/include/materials.h:99-256 (all branches, incl. the glossy ones)
__device__ bool random_photon_bounce(const rt_blinn &m, const Hit &h, V3 &rp, V3 &rd, V3 &c, Philox &rng)
{
    const V3 V = -rd;
    const V3 N = h.N;
    const float NV = dot(N, V);
    const V3 Y = NV > 0.f ? N : -N;
    float ein = 1, eout = m.ior;
    if (!h.front) { ein = m.ior; eout = 1; }
    const float eta = ein / eout;
    const V3 Z = cross(V, Y);
    const V3 X = normalize(cross(Y, Z));
    const float cosI = NV;
    const float sinI = sqrtf(fmaxf(0.0f, 1 - cosI * cosI));
    const float sinO = RMAX(0.f, RMIN(1.f, sinI * eta));
    const float cosO = sqrtf(1.f - sinO * sinO);
    const V3 tDir = (-X) * sinO - Y * cosO;
    const V3 rDir = (N * 2.f) * NV - V;
    const float C0 = (eta - 1.f) * (eta - 1.f) / ((eta + 1.f) * (eta + 1.f));
    const float rC = C0 + (1.f - C0) * powf(1.f - fabsf(cosI), 5.f);
    const float tC = 1.f - rC;
    const bool tot = (eta * sinI) > 1.001f;
    const V3 tK = ld3(m.refraction), rK = ld3(m.reflection);
    const V3 sRefr = tot ? mk(0, 0, 0) : tK * tC;
    const V3 sRefl = tot ? (rK + tK) : (rK + tK * rC);
    const V3 sDiff = ld3(m.diffuse), sSpec = ld3(m.specular);
    const float random = rng.next();                                    // :150
    float diffuseProb = gray(sDiff), refractionProb = gray(sRefr), reflectionProb = gray(sRefl), absorptionProb = gray(ld3(m.absorption));
    const float total = diffuseProb + reflectionProb + refractionProb + absorptionProb;
    diffuseProb /= total; refractionProb /= total; reflectionProb /= total;
    const float rcp = 1.f / total;
    const float select = random * total;                                // :163 (compared with the NORMALISED probabilities)
    const float luma = 0.00001f;
    int selected; float scale = 1.f;
    if (select <= refractionProb && refractionProb > luma) { selected = 0; scale = refractionProb * rcp; }
    else if (select > refractionProb && select <= refractionProb + reflectionProb && reflectionProb > luma) { selected = 1; scale = reflectionProb * rcp; }
    else if (select > refractionProb + reflectionProb && select < refractionProb + reflectionProb + diffuseProb && diffuseProb > luma) { selected = 2; scale = diffuseProb * rcp; }
    else selected = 3;
    V3 dir, BxDF;
    if (selected == 0) {
        if (m.refraction_glossiness > 0.f) {               // :183-190: SampleHemisphere (:40-48), in ITS frame, used as is
            const float u1 = rng.next(), u2 = rng.next();
            const float r = sqrtf(1.0f - u1 * u1);
            const float phi = (float)(2 * M_PI * (double)u2);
            dir = mk(cosf(phi) * r, sinf(phi) * r, u1);
            const V3 L = normalize(dir);
            const V3 H = normalize(V + L);
            const float cosVH = RMAX(0.f, dot(V, H));
            BxDF = sRefr * powf(cosVH, m.refraction_glossiness);
        } else { dir = tDir; BxDF = sRefr; }
    } else if (selected == 1) {
        if (m.reflection_glossiness > 0.f) {               // :200-207: CosineSampleHemisphere (:27-38)
            const float u1 = rng.next(), u2 = rng.next();
            const float r = sqrtf(u1);
            const float theta = (float)(2 * M_PI * (double)u2);
            dir = mk(r * cosf(theta), r * sinf(theta), sqrtf(fmaxf(0.0f, 1 - u1)));
            const V3 L = normalize(dir);
            const V3 H = normalize(V + L);
            const float cosNH = RMAX(0.f, dot(N, H));
            BxDF = sRefl * powf(cosNH, m.reflection_glossiness);
        } else { dir = rDir; BxDF = sRefl; }
    } else if (selected == 2) {
        if (!h.front) return false;
        // createCoordinateSystem, materials.h:50-59
        V3 Nt = dot(N, mk(1, 0, 0)) < 0.4f ? cross(N, mk(1, 0, 0)) : cross(N, mk(0, 0, 1));
        Nt = normalize(Nt);
        const V3 Nb = cross(N, Nt);
        const float theta = (float)((double)rng.next() * M_PI_2);       // :227
        const float phi = (float)((double)rng.next() * (2.0 * M_PI));   // :228
        dir = (Nt * cosf(phi)) * sinf(theta) + (Nb * sinf(phi)) * sinf(theta) + N * cosf(theta);
        const V3 L = normalize(dir);
        const V3 H = normalize(V + L);
        const float cosNH = RMAX(0.f, dot(N, H));
        BxDF = sDiff + sSpec * powf(cosNH, m.glossiness);
    } else return false;
    rp = h.p; rd = normalize(dir);
    c = (c * BxDF) / (1.f * scale);                                     // c * BxDF / (PDF * scale)
    if (!h.front) c = c * attenuation(ld3(m.absorption), h.z);
    return true;
}

#define RT_PHOTON_SLOTS 8
__global__ __launch_bounds__(RT_BLOCK) void k_photon_trace(DevScene S, PhotonArgs A)
{
    __shared__ uint32_t s_stack[RT_BVH_STACK * RT_BLOCK];
    const BvhStack stack = bvh_stack(s_stack, RT_BVH_STACK, S.bvh_spill);
    Counters cnt = {0, 0, 0, 0, 0};
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= A.n_attempts) return;
    const unsigned long long attempt = A.first_attempt + i;
    Philox rng;
    rng.key0 = A.seed; rng.key1 = 0x52544D49u; rng.c0 = (uint32_t)attempt; rng.c1 = (uint32_t)(attempt >> 32); rng.blk = 0; rng.used = 4;
    // choose one photon source uniformly (the reference hard-codes two lights, :367-370)
    int npl = 0;
    for (int l = 0; l < S.n_lights; l++) if (S.lights[l].type == RT_LIGHT_POINT) npl++;
    uint32_t stored = 0, hits = 0;
    float *out = A.out + (size_t)i * RT_PHOTON_SLOTS * 9;
    if (npl > 0) {
        int pick = (int)(rng.next() * (float)npl);
        if (pick >= npl) pick = npl - 1;
        int li = 0;
        for (int l = 0; l < S.n_lights; l++) if (S.lights[l].type == RT_LIGHT_POINT) { if (pick == 0) { li = l; break; } pick--; }
        const rt_light &L = S.lights[li];
        V3 c = ld3(L.intensity);
        const V3 position = ld3(L.position);
        // PointLight::RandomPhoton, :489-497
        const float x = 2 * rng.next() - 1, y = 2 * rng.next() - 1, z = 2 * rng.next() - 1;
        V3 rp = position;
        V3 rd = normalize((mk(x, y, z) + position) - position);
        Hit h;
        if (A.mode == 1) {
            // caustic pass (P13/main.cpp:383-398 + CausticTracing :431-457): the first hit sets hitspec (0 on a photon
            // surface, else 1); then every diffuse hit is COUNTED and, behind more than one specular hit, STORED
            if (trace<false, RT_SHADE_FIN>(S, rp, rd, BIGFLOAT, h, stack, cnt)) {
                const rt_blinn *m = &S.materials[S.node_material[h.node]];
                int hitspec = gray(ld3(m->diffuse)) > 0 ? 0 : 1;
                int bounce = A.max_bounce;
                while (bounce > 0 && random_photon_bounce(*m, h, rp, rd, c, rng)) {
                    Hit nh;
                    if (!trace<false, RT_SHADE_FIN>(S, rp, rd, BIGFLOAT, nh, stack, cnt)) break;
                    m = &S.materials[S.node_material[nh.node]];
                    if (gray(ld3(m->diffuse)) > 0) {
                        if (hitspec > 1 && stored < RT_PHOTON_SLOTS) {
                            float *o = out + 9 * stored;
                            o[0] = nh.p.x; o[1] = nh.p.y; o[2] = nh.p.z; o[3] = rd.x; o[4] = rd.y; o[5] = rd.z; o[6] = c.x; o[7] = c.y; o[8] = c.z;
                            stored++;
                        }
                        hits++;
                    } else hitspec++;
                    bounce--;
                    h = nh;
                }
            }
        } else
        if (trace<false, RT_SHADE_FIN>(S, rp, rd, BIGFLOAT, h, stack, cnt)) {
            const rt_blinn *m = &S.materials[S.node_material[h.node]];
            if (gray(ld3(m->diffuse)) > 0) {                             // IsPhotonSurface, materials.h:97
                int bounce = A.max_bounce;
                while (bounce > 0 && random_photon_bounce(*m, h, rp, rd, c, rng)) {      // PhotonTracing :439-459
                    Hit nh;
                    if (!trace<false, RT_SHADE_FIN>(S, rp, rd, BIGFLOAT, nh, stack, cnt)) break;
                    m = &S.materials[S.node_material[nh.node]];
                    if (gray(ld3(m->diffuse)) > 0 && stored < RT_PHOTON_SLOTS) {
                        float *o = out + 9 * stored;
                        o[0] = nh.p.x; o[1] = nh.p.y; o[2] = nh.p.z; o[3] = rd.x; o[4] = rd.y; o[5] = rd.z; o[6] = c.x; o[7] = c.y; o[8] = c.z;
                        stored++;
                    }
                    bounce--;
                    h = nh;
                }
            }
        }
    }
    A.count[i] = stored | (hits << 16);
}

void rtk_launch_photon_trace(hipStream_t st, const DevScene &S, const PhotonArgs &A)
{
    hipLaunchKernelGGL(k_photon_trace, dim3((A.n_attempts + RT_BLOCK - 1) / RT_BLOCK), dim3(RT_BLOCK), 0, st, S, A);
}

void rtk_launch_trace(hipStream_t st, const DevScene &S, int model, const float *rays, long long n, const TraceOut &o)
{
    const int grid = grid_for((unsigned long long)n, RT_BLOCK, RT_SPILL_BLOCKS);
    if (model == RT_SHADE_P3) hipLaunchKernelGGL(k_trace<RT_SHADE_P3>, dim3(grid), dim3(RT_BLOCK), 0, st, S, rays, n, o.hit, o.z, o.p, o.N, o.node, o.front);
    else if (model != RT_SHADE_FIN) hipLaunchKernelGGL(k_trace<RT_SHADE_P13>, dim3(grid), dim3(RT_BLOCK), 0, st, S, rays, n, o.hit, o.z, o.p, o.N, o.node, o.front);
    else hipLaunchKernelGGL(k_trace<RT_SHADE_FIN>, dim3(grid), dim3(RT_BLOCK), 0, st, S, rays, n, o.hit, o.z, o.p, o.N, o.node, o.front);
}
