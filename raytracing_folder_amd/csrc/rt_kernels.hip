// rt_kernels.hip -- the hand-written HIP kernels (gfx950 / CDNA4, wave64) that shade, and their launch layer.
//
//   k_wavefront K1+K2+K3+K4  the whole ray tree of a chunk in one persistent launch: primary-ray generation,
//                            closest-hit traversal, Blinn shade with an any-hit shadow ray per light, children
//                            pushed onto the workgroup's ray stack in LDS and popped 256 at a time (FIN, P13)
//   k_primary   K1+K2+K3+K4  the same for the primary rays only, children to the global SoA ray queues
//   k_bounce    K2+K3+K4     one level of the reflection/refraction ray tree from a global queue (the other
//                            shading models; rays k_wavefront could not keep in LDS)
//   k_mark_second, k_features  the first-hit feature planes of a chunk (opt-in)
//   (k_trace    K2           closest-hit only, and k_photon_trace, the photon pass: rt_trace.hip)
//   (k_gather   K5           the k-nearest photon gather: rt_gather.hip)
//   (k_resolve  K6           per-pixel average / variance gate / gamma / Color24 pack, k_fold_fx and the two
//                            unpack kernels: rt_resolve.hip)
//
// The device functions the kernels are made of are in rt_shade.h (shading) and, below it, rt_trace.h (geometry and
// traversal; it also says how the arithmetic follows the reference).  This file includes rt_shade.h and holds
// the kernels, their RT_WF_* tuning defines and the launch layer: environment hooks, make_ctx, make_slotmap,
// dispatch and the five rtk_launch_* wrappers.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>
#include <stdlib.h>
#include <type_traits>
#include "rt_shade.h"

#ifndef RT_WF_GRAB
#define RT_WF_GRAB 2           // rounds of 256 primary samples (or queued rays) a workgroup of k_wavefront takes per atomic on the work counter
#endif

#define RT_TRACE_OCC __attribute__((amdgpu_waves_per_eu(TEX ? 2 : 3)))
template <int MODEL, bool TEX, bool FX = false>
RT_TRACE_OCC __global__ __launch_bounds__(RT_BLOCK) void k_primary(ShadeCtx C, PrimaryArgs A)
{
    __shared__ uint32_t s_stack[RT_BVH_STACK * RT_BLOCK];
    const BvhStack stack = bvh_stack(s_stack, RT_BVH_STACK, C.S.bvh_spill);
    Counters cnt = {0, 0, 0, 0, 0};
    uint32_t nprim = 0;
    const uint32_t npix = (A.mode == 1) ? C.W.counts[CNT_PIXLIST] : A.npix;
    const unsigned long long total = (unsigned long long)npix * (unsigned long long)A.ns;
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    // Halton(j, 2) and Halton(j, 3) of this launch's sample indices, once per workgroup (the loop in
    // halton() divides; the values are the same floats either way)
    __shared__ float s_h2[RT_BLOCK], s_h3[RT_BLOCK];
    const bool h_table = A.mode != 2 && A.ns <= RT_BLOCK;
    if (h_table && (int)threadIdx.x < A.ns) { s_h2[threadIdx.x] = halton(A.j0 + (int)threadIdx.x, 2); s_h3[threadIdx.x] = halton(A.j0 + (int)threadIdx.x, 3); }
    __syncthreads();
    // every lane iterates the same number of times (wave-collective pushes inside shade_path)
    for (unsigned long long base = (unsigned long long)blockIdx.x * blockDim.x; base < total; base += stride) {
        PathIn in;
        const bool active = primary_setup(C, A, base + threadIdx.x, total, h_table, s_h2, s_h3, in);
        if (active) nprim++;
        shade_path<MODEL, TEX, FX>(C, in, active, stack, cnt);
    }
    flush_counters(C.W.stats, cnt, nprim, 0, 0);
}

// K2-K4 for one level of the ray tree: reads queue `qin` (count in counts[level]).
template <int MODEL, bool TEX, bool FX = false>
RT_TRACE_OCC __global__ __launch_bounds__(RT_BLOCK) void k_bounce(ShadeCtx C, DevRayQueue qin, int level)
{
    __shared__ uint32_t s_stack[RT_BVH_STACK * RT_BLOCK];
    const BvhStack stack = bvh_stack(s_stack, RT_BVH_STACK, C.S.bvh_spill);
    Counters cnt = {0, 0, 0, 0, 0};
    uint32_t nrefl = 0, nrefr = 0;
    uint32_t total = C.W.counts[level];
    if (total > qin.cap) total = qin.cap;
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t base = blockIdx.x * blockDim.x; base < total; base += stride) {
        const uint32_t gid = base + threadIdx.x;
        const bool active = gid < total;
        PathIn in;
        in.primary = false; in.thr = mk(0, 0, 0); in.absorb = mk(0, 0, 0); in.o = mk(0, 0, 0); in.d = mk(0, 0, 1);
        in.slot = 0; in.bounce = 0; in.kind = 0; in.node = 1; in.sample = 0; in.spec = 0;
        in.side_dir = mk(0, 0, 1); in.side_K = mk(0, 0, 0);
        if (active) {
            const uint32_t src = gid;
            const float4 a = qin.a[src], b = qin.b[src], c = qin.c[src];
            const uint4 dd = qin.d[src];
            in.o = mk(a.x, a.y, a.z); in.d = mk(a.w, b.x, b.y);
            in.thr = mk(b.z, b.w, c.x); in.absorb = mk(c.y, c.z, c.w);
            in.slot = dd.x; in.bounce = (int)(dd.y & 0xFFu); in.kind = (dd.y >> 8) & 0xFFu; in.spec = (dd.y >> 16) & 0xFFu; in.node = dd.z; in.sample = dd.w;
            if (MODEL == RT_SHADE_P6 && in.kind == KIND_REFRACT) {
                const float4 e = qin.e[src];
                in.side_dir = mk(e.x, e.y, e.z); in.side_K = mk(e.w, c.z, c.w);
                in.absorb = mk(c.y, 0, 0);
            }
            if (in.kind == KIND_REFLECT) nrefl++; else nrefr++;
        }
        shade_path<MODEL, TEX, FX>(C, in, active, stack, cnt);
    }
    flush_counters(C.W.stats, cnt, 0, nrefl, nrefr);
}

// ------------------------------------------------------------------------------------------------
// The whole ray tree of a chunk in ONE launch: a persistent grid of workgroups, each with its own ray stack in
// LDS (BASELINE.json north_star: "persistent-threads wavefront tracer with ray queues in LDS").  A workgroup
// takes 256 primary samples at a time from a device-side counter; the reflection/refraction children its rays
// spawn are pushed onto ITS stack (wave-aggregated LDS atomic) and popped 256 at a time -- whenever 256 are
// waiting, or when the primary samples have run out -- so the deep, sparse levels of the tree are traced by
// full wavefronts next to other workgroups' primary rays instead of in launches of their own that cannot fill
// 256 CUs.  Nothing is handed between workgroups (no cross-CU visibility protocol needed); a ray that finds
// the stack full goes to the global queue and is picked up by the per-level k_bounce launches that follow
// (normally empty).  FIN and P13 models (at most two children per hit); the others keep the per-level kernels.
// ------------------------------------------------------------------------------------------------
// Configuration: the texture-free instantiations run THREE workgroups per CU (3 waves/SIMD: the traversal waits on dependent
// loads for 0.44 of its wave cycles at two) -- 168 VGPRs, and per workgroup at most 53 760 B of LDS (160 KB / 3 in 1280-byte
// granules): RT_BVH_LDS = 8 BVH stack entries per lane (8 KB; a deeper traversal continues in the HBM spill part, rt_dev.h) + a
// 928-ray stack of 48-byte records (44.5 KB) + two 64-entry Halton tables.  (Round 3 and the start of round 4: 24 entries + 592
// rays.  The rays that do not fit the stack take the global queue, a second pass and the per-level launches: 7.8 M of the Cornell
// frame's 42 M secondary rays and 1.8 ms at 592 rays, 0.6 M and 0.36 ms at 928; C3: 27 -> 13 ms.)  The textured
// instantiations get the same configuration (the compiler would take 255 VGPRs for them; held to 168 the texture lookups'
// temporaries go to scratch, which costs less than the third wave buys).  RT_WF_WAVES=2 / RT_WF_TEX_WAVES=2: two workgroups
// per CU, 32-entry BVH stacks, 1008 rays (A/B builds).
#ifndef RT_WF_WAVES
#define RT_WF_WAVES 3          // waves per SIMD = workgroups per CU of the texture-free instantiations
#endif
#ifndef RT_WF_TEX_WAVES
#define RT_WF_TEX_WAVES 3      // ... of the textured ones (measured on the 102 k-triangle frame under a PNG sky: 40.5 ms at two, 31.2 ms at three)
#endif
#define RT_WF_HALTON 64
template <bool TEX> struct WfCfg {
    static constexpr int WAVES = TEX ? RT_WF_TEX_WAVES : RT_WF_WAVES;
#ifndef RT_WF_STACK
#define RT_WF_STACK 928
#endif
    static constexpr int BVH = WAVES >= 3 ? RT_BVH_LDS : RT_BVH_STACK;
    static constexpr int STACK = WAVES >= 3 ? RT_WF_STACK : 1008;
    // pop a round as soon as a round of primary rays (two children each) could no longer be sure to fit
    static constexpr int POP = STACK - 2 * RT_BLOCK + 1 < RT_BLOCK ? STACK - 2 * RT_BLOCK + 1 : RT_BLOCK;
    static_assert(BVH * RT_BLOCK * 4 + STACK * 48 + 2 * RT_WF_HALTON * 4 + 16 <= (WAVES >= 3 ? 53760 : 81920), "LDS budget of the occupancy the kernel is built for");
};
// global sample id of a chunk slot (see SlotMap)
__device__ __forceinline__ uint32_t sample_of_slot(const SlotMap &M, uint32_t slot)
{
    if (M.mode == 2) return M.q0 + slot;
    const uint32_t ql = fastdiv(slot, M.div_ms), j = slot - ql * (uint32_t)M.max_sample;
    DevCamera cam; cam.width = M.width; cam.height = M.height;
    int x = 0, y = 0;
    pixel_of(M.tiles, cam, M.q0 + ql, x, y);
    return ((uint32_t)y * (uint32_t)M.width + (uint32_t)x) * (uint32_t)M.max_sample + j;
}
template <int MODEL, bool TEX, bool FX = false>
__attribute__((amdgpu_waves_per_eu(TEX ? RT_WF_TEX_WAVES : RT_WF_WAVES, TEX ? RT_WF_TEX_WAVES : RT_WF_WAVES))) __global__ __launch_bounds__(RT_BLOCK) void k_wavefront(ShadeCtx C, PrimaryArgs A)
{
    using Cfg = WfCfg<TEX>;
    __shared__ uint32_t s_stack[Cfg::BVH * RT_BLOCK];
    __shared__ float4 s_qa[Cfg::STACK], s_qb[Cfg::STACK], s_qc[Cfg::STACK];
    __shared__ uint32_t s_count, s_batch;
    __shared__ float s_h2[RT_WF_HALTON], s_h3[RT_WF_HALTON];
  if constexpr (RT_WF_PERWAVE && MODEL == RT_SHADE_P12) {
    // RayTracingProj12's paths (one hemisphere ray per hit, eight levels deep: every round is a pop round): every WAVE runs its
    // own rounds on its own quarter of the ray stack, no workgroup barrier anywhere in the loop.  A round's length varies by
    // an order of magnitude with what its 64 rays meet, and with a shared stack the four waves of a workgroup meet at three
    // barriers per round (C3: 307 -> 272 ms).  Not for the FIN / P13 trees: their glass doubles the rays level by level, a
    // quarter stack overflows into the global queue and its per-level launches (Cornell tracer 16.8 -> 32.2 ms, measured).
    constexpr int NW = RT_BLOCK / 64;
    constexpr uint32_t STACK_W = (uint32_t)Cfg::STACK / NW;
    constexpr uint32_t POP_W = STACK_W > 128u ? (STACK_W - 127u < 64u ? STACK_W - 127u : 64u) : 1u;   // pop before a round of primaries (two children each) could overflow
    __shared__ uint32_t s_countw[NW];
    const int wv = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
    float4 *qa = s_qa + wv * STACK_W, *qb = s_qb + wv * STACK_W, *qc = s_qc + wv * STACK_W;
    const BvhStack stack = bvh_stack(s_stack, Cfg::BVH, C.S.bvh_spill);
    Counters cnt = {0, 0, 0, 0, 0};
    uint32_t nprim = 0, nrefl = 0, nrefr = 0;
    const uint32_t npix = (A.mode == 1) ? C.W.counts[CNT_PIXLIST] : A.npix;
    const unsigned long long total = A.mode == 3 ? (unsigned long long)min(*A.qsrc_count, A.qsrc.cap)
                                                 : (unsigned long long)npix * (unsigned long long)A.ns;
    const unsigned long long n_batches = (total + 63ull) / 64ull;
    const bool h_table = A.mode < 2 && A.ns <= RT_WF_HALTON;
    uint32_t *next_batch = C.W.counts + (A.mode == 3 ? CNT_WF2_NEXT : CNT_PRIMARY_NEXT);
    if (h_table && (int)threadIdx.x < A.ns) { s_h2[threadIdx.x] = halton(A.j0 + (int)threadIdx.x, 2); s_h3[threadIdx.x] = halton(A.j0 + (int)threadIdx.x, 3); }
    if (lane == 0) s_countw[wv] = 0;
    C.lds_a = qa; C.lds_b = qb; C.lds_c = qc; C.lds_count = &s_countw[wv]; C.lds_cap = STACK_W;
    __syncthreads();                                      // the Halton table (the only thing the waves share)
    (void)s_count; (void)s_batch;
    auto wsync = []() {                                   // LDS operations of one wave complete in issue order: only the compiler has to be held
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    };
    bool more_primaries = true;                           // wave-uniform
    for (;;) {
        wsync();                                          // last round's pushes are complete
        uint32_t waiting = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_countw[wv]);
        if (waiting > STACK_W) waiting = STACK_W;         // the excess went to the global queue
        const bool pop = waiting >= POP_W || (!more_primaries && waiting > 0);
        if (!pop && !more_primaries) break;
        PathIn in;
        bool active;
        if (pop) {
            const uint32_t n = min(waiting, 64u);
            active = (uint32_t)lane < n;
            in.primary = false; in.thr = mk(0, 0, 0); in.absorb = mk(0, 0, 0); in.o = mk(0, 0, 0); in.d = mk(0, 0, 1);
            in.slot = 0; in.bounce = 0; in.kind = 0; in.node = 1; in.sample = 0; in.spec = 0;
            in.side_dir = mk(0, 0, 1); in.side_K = mk(0, 0, 0);
            if (active) {
                const uint32_t src = waiting - 1u - (uint32_t)lane;       // newest (deepest) first: the stack stays shallow
                const float4 a = qa[src], b = qb[src], c = qc[src];
                in.o = mk(a.x, a.y, a.z); in.d = mk(a.w, b.x, b.y);
                in.thr = mk(b.z, b.w, c.x);
                in.slot = __float_as_uint(c.y);
                const uint32_t pk = __float_as_uint(c.z);
                in.bounce = (int)(pk & 0xFu); in.kind = (pk >> 4) & 0xFu; in.spec = (pk >> 8) & 0xFFu; in.node = __float_as_uint(c.w);
                const float *ab = C.S.materials[pk >> 16].absorption;
                in.absorb = (MODEL == RT_SHADE_FIN) ? ld3(ab) : mk(ab[0], 0, 0);
                if (C.S.stochastic || MODEL == RT_SHADE_P12) in.sample = sample_of_slot(C.sm, in.slot);     // P12 draws its hemisphere rays
                if (in.kind == KIND_REFLECT) nrefl++; else nrefr++;
            }
            wsync();                                      // all pops read before anything is pushed over them
            if (lane == 0) s_countw[wv] = waiting - n;
        } else {
            uint32_t bt = 0;
            if (lane == 0) { bt = atomicAdd(next_batch, 1u); if (s_countw[wv] > STACK_W) s_countw[wv] = STACK_W; }
            const unsigned long long batch = (uint32_t)__builtin_amdgcn_readfirstlane((int)bt);
            if (batch >= n_batches) { more_primaries = false; continue; }
            if (A.mode == 3) {
                const unsigned long long src = batch * 64ull + (unsigned)lane;
                active = src < total;
                in.primary = false; in.thr = mk(0, 0, 0); in.absorb = mk(0, 0, 0); in.o = mk(0, 0, 0); in.d = mk(0, 0, 1);
                in.slot = 0; in.bounce = 0; in.kind = 0; in.node = 1; in.sample = 0; in.spec = 0;
                in.side_dir = mk(0, 0, 1); in.side_K = mk(0, 0, 0);
                if (active) {
                    const float4 a = A.qsrc.a[src], b = A.qsrc.b[src], c = A.qsrc.c[src];
                    const uint4 dd = A.qsrc.d[src];
                    in.o = mk(a.x, a.y, a.z); in.d = mk(a.w, b.x, b.y);
                    in.thr = mk(b.z, b.w, c.x); in.absorb = mk(c.y, c.z, c.w);
                    in.slot = dd.x; in.bounce = (int)(dd.y & 0xFFu); in.kind = (dd.y >> 8) & 0xFFu; in.spec = (dd.y >> 16) & 0xFFu; in.node = dd.z; in.sample = dd.w;
                    if (in.kind == KIND_REFLECT) nrefl++; else nrefr++;
                }
            } else {
                active = primary_setup(C, A, batch * 64ull + (unsigned)lane, total, h_table, s_h2, s_h3, in);
                if (active) nprim++;
            }
        }
        wsync();                                          // the count is settled before this round's pushes
        shade_path<MODEL, TEX, FX>(C, in, active, stack, cnt);
    }
    flush_counters(C.W.stats, cnt, nprim, nrefl, nrefr);
  } else {
    const BvhStack stack = bvh_stack(s_stack, Cfg::BVH, C.S.bvh_spill);
    Counters cnt = {0, 0, 0, 0, 0};
    uint32_t nprim = 0, nrefl = 0, nrefr = 0;
    const uint32_t npix = (A.mode == 1) ? C.W.counts[CNT_PIXLIST] : A.npix;
    // mode 3: the rays that did not fit the LDS stacks of the pass before (they sit in a global queue) are the work items;
    // their descendants live on this pass's LDS stacks like everybody else's
    const unsigned long long total = A.mode == 3 ? (unsigned long long)min(*A.qsrc_count, A.qsrc.cap)
                                                 : (unsigned long long)npix * (unsigned long long)A.ns;
    const unsigned long long n_batches = (total + RT_BLOCK - 1) / RT_BLOCK;
    const bool h_table = A.mode < 2 && A.ns <= RT_WF_HALTON;
    uint32_t *next_batch = C.W.counts + (A.mode == 3 ? CNT_WF2_NEXT : CNT_PRIMARY_NEXT);
    if (h_table && (int)threadIdx.x < A.ns) { s_h2[threadIdx.x] = halton(A.j0 + (int)threadIdx.x, 2); s_h3[threadIdx.x] = halton(A.j0 + (int)threadIdx.x, 3); }
    if (threadIdx.x == 0) s_count = 0;
    C.lds_a = s_qa; C.lds_b = s_qb; C.lds_c = s_qc; C.lds_count = &s_count; C.lds_cap = (A.lds_rays && A.lds_rays < (uint32_t)Cfg::STACK) ? A.lds_rays : (uint32_t)Cfg::STACK;
    bool more_primaries = true;                           // workgroup-uniform
    // A workgroup takes RT_WF_GRAB rounds of 256 per atomic on the work counter when the launch has plenty: the returning atomic is a
    // round trip to the memory side with the whole workgroup at the barrier behind it (r4, pairs: -2.7 % on the 102 k-triangle frame,
    // Cornell tracer 13.67 -> 13.35 ms with its gather 0.13 ms slower for the changed order of its queue; fours: the gather loses more).
    // The per-wave rounds of P12 keep one round per atomic: pairs cost C3 0.9 %, fours 3 %.
    const uint32_t grab = n_batches >= 128ull * gridDim.x ? (uint32_t)RT_WF_GRAB : 1u;
    unsigned long long grabbed = 0; uint32_t in_hand = 0; // workgroup-uniform: the rounds this workgroup holds
    for (;;) {
        __syncthreads();                                  // last round's pushes are complete
        const uint32_t packed = s_count;
        const uint32_t w0 = packed & 0xFFFFu, w1 = packed >> 16;
        const uint32_t pside = w1 > w0 ? 1u : 0u;         // the fuller side is popped
        const uint32_t waiting = w0 + w1;                 // never beyond the stack: a push that does not fit takes its count back (push_ray)
        // pop a full workgroup's worth when there is one -- and already earlier when a round of primary rays (up to two
        // children each) could no longer be sure to fit: rays that do not fit go through the global queue and the
        // per-level launches, the slow path (measured: 5 ms per Cornell frame before this rule)
        const bool pop = waiting >= (uint32_t)Cfg::POP || (!more_primaries && waiting > 0);
        if (!pop && !more_primaries) break;
        __syncthreads();                                  // everyone has read s_count
        PathIn in;
        bool active;
        if (pop) {
            // always a whole workgroup's worth when there is one: shrinking the round so that a nearly full stack could not
            // overflow was measured slower (rounds of n >= 64 / 128 / 192: Cornell trace 28.1 / 26.8 / 25.7 ms vs 24.9; with no
            // floor, rounds of a handful of rays whose children refill the stack at once: 66.5 ms) -- the few rays that do not
            // fit take the global queue
            const uint32_t wside = pside ? w1 : w0;
            const uint32_t n = min(wside, (uint32_t)RT_BLOCK);
            active = threadIdx.x < n;
            in.primary = false; in.thr = mk(0, 0, 0); in.absorb = mk(0, 0, 0); in.o = mk(0, 0, 0); in.d = mk(0, 0, 1);
            in.slot = 0; in.bounce = 0; in.kind = 0; in.node = 1; in.sample = 0; in.spec = 0;
            in.side_dir = mk(0, 0, 1); in.side_K = mk(0, 0, 0);
            if (active) {
                const uint32_t src = pside ? C.lds_cap - wside + threadIdx.x : wside - 1u - threadIdx.x;
                const float4 a = s_qa[src], b = s_qb[src], c = s_qc[src];
                in.o = mk(a.x, a.y, a.z); in.d = mk(a.w, b.x, b.y);
                in.thr = mk(b.z, b.w, c.x);
                in.slot = __float_as_uint(c.y);
                const uint32_t pk = __float_as_uint(c.z);
                in.bounce = (int)(pk & 0xFu); in.kind = (pk >> 4) & 0xFu; in.spec = (pk >> 8) & 0xFFu; in.node = __float_as_uint(c.w);
                // what the child needs of its parent's material on arrival: Attenuation(absorption, z) (FIN/main.cpp:620,632),
                // exp(-absorption.r * z) (P13/main.cpp:728)
                const float *ab = C.S.materials[pk >> 16].absorption;
                in.absorb = (MODEL == RT_SHADE_FIN) ? ld3(ab) : mk(ab[0], 0, 0);
                if (C.S.stochastic || MODEL == RT_SHADE_P12) in.sample = sample_of_slot(C.sm, in.slot);     // P12 draws its hemisphere rays
                if (in.kind == KIND_REFLECT) nrefl++; else nrefr++;
            }
            __syncthreads();                              // all pops read before anything is pushed over them
            if (threadIdx.x == 0) s_count = packed - (n << (16u * pside));
        } else {
            if (in_hand == 0) {                           // `grab` rounds per visit of the work counter
                if (threadIdx.x == 0) s_batch = atomicAdd(next_batch, 1u);
                __syncthreads();
                grabbed = (unsigned long long)s_batch * grab;
                in_hand = grab;
            }
            const unsigned long long batch = grabbed + (grab - in_hand);
            in_hand--;
            if (batch >= n_batches) { more_primaries = false; continue; }
            if (A.mode == 3) {
                const unsigned long long src = batch * RT_BLOCK + threadIdx.x;
                active = src < total;
                in.primary = false; in.thr = mk(0, 0, 0); in.absorb = mk(0, 0, 0); in.o = mk(0, 0, 0); in.d = mk(0, 0, 1);
                in.slot = 0; in.bounce = 0; in.kind = 0; in.node = 1; in.sample = 0; in.spec = 0;
                in.side_dir = mk(0, 0, 1); in.side_K = mk(0, 0, 0);
                if (active) {
                    const float4 a = A.qsrc.a[src], b = A.qsrc.b[src], c = A.qsrc.c[src];
                    const uint4 dd = A.qsrc.d[src];
                    in.o = mk(a.x, a.y, a.z); in.d = mk(a.w, b.x, b.y);
                    in.thr = mk(b.z, b.w, c.x); in.absorb = mk(c.y, c.z, c.w);
                    in.slot = dd.x; in.bounce = (int)(dd.y & 0xFFu); in.kind = (dd.y >> 8) & 0xFFu; in.spec = (dd.y >> 16) & 0xFFu; in.node = dd.z; in.sample = dd.w;
                    if (in.kind == KIND_REFLECT) nrefl++; else nrefr++;
                }
            } else {
                active = primary_setup(C, A, batch * RT_BLOCK + threadIdx.x, total, h_table, s_h2, s_h3, in);
                if (active) nprim++;
            }
        }
        __syncthreads();                                  // s_count settled before this round's pushes
        shade_path<MODEL, TEX, FX>(C, in, active, stack, cnt);
    }
    flush_counters(C.W.stats, cnt, nprim, nrefl, nrefr);
  }
}

// ------------------------------------------------------------------------------------------------
// First-hit feature planes (opt-in): normal, albedo, alpha, object id of every pixel of a chunk, from the chunk's finished
// working set.  The reference averages a pixel over its HIT samples only (RenderPixel, FIN/main.cpp:273-338), so with J the
// samples the final resolve used and H the hit ones among them (n = |H|, in sample order):
//   normal = sum_H N_j * (1/n)        N_j = Hit::N of the primary ray as trace<>() returns it; not renormalised
//   albedo = sum_H kd_j * (1/n)       kd of material_colors<TEX>(): diffuse x its map at the hit's uvw (FIN/main.cpp:531)
//   alpha  = n / |J|                  the coverage k_resolve knows and drops
//   object_id = Hit::node of the LAST hit sample, the one the z plane is taken from
// and 0, 0, 0, -1 for an all-miss pixel.  Run once per chunk after its last k_resolve, never in a default render.
//
// The primary Hit is not kept per sample (28 B x samples) and the tracing kernels carry no feature template: this kernel
// traces the hit primary samples again, closest hit only, through primary_setup + trace<false, MODEL, TEX> -- the same ray,
// the same intersection code, hence the same Hit bit for bit.  ONE LANE PER PIXEL walks its samples in index order, so the
// sums have one order by construction (no atomics): the planes are byte-identical whatever the chunking, streams, tiles and
// entry point.  Lanes of a wave hold consecutive pixels of a tile row and trace the same sample index together.
// ------------------------------------------------------------------------------------------------
struct FeatureArgs {
    DevCamera cam; DevTiles tiles;
    uint32_t q0, npix;
    int min_sample, max_sample;
    FastDiv div_ms;
    const uint8_t *second;      // [npix] 1: the pixel took the second batch (k_mark_second), so J is all max_sample samples
    int by_walk;                // 0: planes are image-sized, pixel (x, y) at y*width + x; 1: indexed by the tile walk, q0 + ql
    float *normal, *albedo, *alpha; int32_t *object_id;      // any of them may be NULL
};

// second[ql] = 1 for the pixels k_resolve's first phase put on the chunk's pixel list (the list survives the second phase)
__global__ __launch_bounds__(256) void k_mark_second(DevWork W, uint8_t *second, uint32_t npix)
{
    const uint32_t n = W.counts[CNT_PIXLIST];
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const uint32_t ql = W.pixel_list[i];
        if (ql < npix) second[ql] = 1;
    }
}

// LDS: the traversal stack of k_primary (32 entries x 256 lanes = 32 KB) + 2 KB of Halton tables: four workgroups, i.e. four
// waves per SIMD, fit a CU's 160 KB, which the 128-VGPR budget of four waves matches -- the kernel only traces, it does not
// shade (120 VGPRs, no scratch).  With textures the bilinear lookups do not fit that budget (60 VGPRs spilled at four waves,
// 20 at three): three waves per SIMD there.
template <int MODEL, bool TEX>
__attribute__((amdgpu_waves_per_eu(TEX ? 3 : 4, TEX ? 3 : 4))) __global__ __launch_bounds__(RT_BLOCK) void k_features(ShadeCtx C, FeatureArgs F)
{
    __shared__ uint32_t s_stack[RT_BVH_STACK * RT_BLOCK];
    const BvhStack stack = bvh_stack(s_stack, RT_BVH_STACK, C.S.bvh_spill);
    Counters cnt = {0, 0, 0, 0, 0};                 // trace<>() counts into it; never flushed: the statistics are the render's
    // primary_setup as k_primary calls it for samples 0..max_sample-1 of every pixel: gid = ql*max_sample + j
    PrimaryArgs A;
    A.cam = F.cam; A.tiles = F.tiles; A.q0 = F.q0; A.npix = F.npix; A.j0 = 0; A.ns = F.max_sample; A.max_sample = F.max_sample; A.mode = 0;
    A.rays = nullptr; A.div_ns = F.div_ms; A.lds_rays = 0; A.qsrc_count = nullptr;
    const unsigned long long total = (unsigned long long)F.npix * (unsigned long long)F.max_sample;
    __shared__ float s_h2[RT_BLOCK], s_h3[RT_BLOCK];
    const bool h_table = F.max_sample <= RT_BLOCK;
    if (h_table && (int)threadIdx.x < F.max_sample) { s_h2[threadIdx.x] = halton((int)threadIdx.x, 2); s_h3[threadIdx.x] = halton((int)threadIdx.x, 3); }
    __syncthreads();
    const bool need_trace = F.normal != nullptr || F.albedo != nullptr || F.object_id != nullptr;
    for (uint32_t ql = blockIdx.x * blockDim.x + threadIdx.x; ql < F.npix; ql += gridDim.x * blockDim.x) {
        int x = 0, y = 0;
        if (!pixel_of(F.tiles, F.cam, F.q0 + ql, x, y)) continue;
        const int ns = F.second[ql] ? F.max_sample : F.min_sample;
        const uint8_t *hitf = C.W.sample_hit + (size_t)ql * F.max_sample;
        int n = 0;
        for (int j = 0; j < ns; j++) n += hitf[j] ? 1 : 0;
        V3 nrm = mk(0, 0, 0), alb = mk(0, 0, 0);
        int id = -1;
        if (n > 0 && need_trace) {
            const float inv = 1 / (float)n;
            for (int j = 0; j < ns; j++) {
                if (!hitf[j]) continue;
                PathIn in;
                if (!primary_setup(C, A, (unsigned long long)ql * (unsigned)F.max_sample + (unsigned)j, total, h_table, s_h2, s_h3, in)) continue;
                Hit h;
                if (!trace<false, MODEL, TEX>(C.S, in.o, in.d, BIGFLOAT, h, stack, cnt)) continue;
                nrm = nrm + h.N * inv;
                if (F.albedo) {
                    V3 kd, ks;
                    material_colors<TEX>(C.S, h, C.S.materials[C.S.node_material[h.node]], kd, ks);
                    alb = alb + kd * inv;
                }
                id = h.node;
            }
        }
        const size_t o = F.by_walk ? (size_t)F.q0 + ql : (size_t)y * F.cam.width + x;
        if (F.normal) { F.normal[3 * o] = nrm.x; F.normal[3 * o + 1] = nrm.y; F.normal[3 * o + 2] = nrm.z; }
        if (F.albedo) { F.albedo[3 * o] = alb.x; F.albedo[3 * o + 1] = alb.y; F.albedo[3 * o + 2] = alb.z; }
        if (F.alpha) F.alpha[o] = (float)n / (float)ns;
        if (F.object_id) F.object_id[o] = id;
    }
}

// ------------------------------------------------------------------------------------------------
// host-callable launch wrappers (C++ linkage, used by rt_lower.cpp and rt_render.cpp)
// ------------------------------------------------------------------------------------------------
// Environment hooks of the launch layer.  The first three are read once per process, RT_WF_LDS_RAYS on every launch.
//   RT_TRACER=levels       the per-level kernels instead of k_wavefront (A/B)
//   RT_P12_TRACER=levels   the same for the P12 model alone
//   RT_WF_QUEUE_PASS=0     no second k_wavefront pass over the overflow queue: straight to the per-level launches
//   RT_WF_LDS_RAYS=n       test hook: k_wavefront's workgroup rounds use only n entries of their LDS ray stack, so that a small
//                          frame already sends rays through the global queue, the second pass and the per-level launches
static bool env_is(const char *name, const char *value) { const char *e = getenv(name); return e && !strcmp(e, value); }
static bool env_wavefront() { static const bool on = !env_is("RT_TRACER", "levels"); return on; }
static bool env_p12_wavefront() { static const bool on = !env_is("RT_P12_TRACER", "levels"); return on; }
static bool env_queue_pass() { static const bool on = !(getenv("RT_WF_QUEUE_PASS") && getenv("RT_WF_QUEUE_PASS")[0] == '0'); return on; }
static uint32_t env_lds_rays()
{
    const char *e = getenv("RT_WF_LDS_RAYS");
    const long v = e ? atol(e) : 0;
    return v > 0 ? (uint32_t)v : 0u;
}

// whether the scene samples textures: selects the TEX instantiations
static bool scene_textured(const DevScene &S) { return S.material_maps != nullptr || S.env_map.texture != RT_MAP_NONE; }

// k_wavefront serves the FIN, P13 and P12 models when every mesh's BVH fits its traversal stack (RT_BVH_LDS entries per lane in LDS
// + RT_BVH_SPILL per thread in HBM; the host refuses meshes beyond that)
bool rtk_wavefront_usable(const DevScene &S, const rt_params &P)
{
    const bool wavefront = env_wavefront(), p12 = env_p12_wavefront();     // both read on the first call, whatever its model
    // P12 (live GI): a hit spawns its hemisphere rays next to the reflection / refraction pair -- one per hit below the first
    // level, hemisphere_sample on it; with up to two of them the LDS stacks hold the tree like FIN's (what does not fit
    // takes the global queue as always)
    const bool model_ok = P.shade_model == RT_SHADE_FIN || P.shade_model == RT_SHADE_P13 ||
                          (P.shade_model == RT_SHADE_P12 && p12 && P.hemisphere_sample <= 2);
    if (!wavefront || !model_ok) return false;
    // (the traversal stack: the kernel's LDS part plus, when the scene has the spill buffer, RT_BVH_SPILL entries per thread behind it)
    return S.max_bvh_depth <= (scene_textured(S) ? WfCfg<true>::BVH : WfCfg<false>::BVH) + (S.max_bvh_depth > RT_BVH_LDS ? RT_BVH_SPILL : 0);
}
// a full persistent grid of k_wavefront: its resident workgroups per CU (LDS) on 256 CUs
static int wavefront_blocks(const DevScene &S) { return 256 * (scene_textured(S) ? RT_WF_TEX_WAVES : RT_WF_WAVES); }

// The context of a launch in its neutral state: no output queue, no LDS ray stack, no slot map, no secondary plane.
static ShadeCtx make_ctx(const DevScene &S, const DevWork &W, const rt_params &P)
{
    ShadeCtx C = {};
    C.S = S; C.S.bvh_spill = W.bvh_spill; C.W = W; C.P = P;
    return C;
}
// ... writing the rays it spawns to the queue of tree level `level` (rt_launch.h)
static ShadeCtx make_ctx(const DevScene &S, const DevWork &W, const rt_params &P, int level, unsigned long long *fx)
{
    ShadeCtx C = make_ctx(S, W, P);
    C.qout = W.rq[level & 1]; C.qout_count = W.counts + level; C.fx = fx;
    return C;
}
static SlotMap make_slotmap(const RenderPass &pass, const DevTiles &tiles_prepared)
{
    SlotMap m; m.tiles = tiles_prepared; m.width = pass.cam.width; m.height = pass.cam.height; m.q0 = pass.q0; m.max_sample = pass.max_sample; m.mode = pass.mode;
    m.div_ms = fastdiv_make((uint32_t)(pass.max_sample > 0 ? pass.max_sample : 1));
    return m;
}

// The one place where the run-time triple (shade model, textures, reproducible mode) becomes template arguments:
// launch(model, tex, fx) is called with three std::integral_constant values.  A kernel template names the models it exists
// for -- FALLBACK serves every model outside the list -- and whether it has reproducible (FX) instantiations at all, so that
// nothing is instantiated that no launch can select.
template <int M> using Model = std::integral_constant<int, M>;
template <bool HAS_FX, int M, class F>
static void dispatch_flags(bool tex, bool fx, F &launch)
{
    if constexpr (HAS_FX) {
        if (fx) { if (tex) launch(Model<M>{}, std::true_type{}, std::true_type{}); else launch(Model<M>{}, std::false_type{}, std::true_type{}); return; }
    }
    if (tex) launch(Model<M>{}, std::true_type{}, std::false_type{}); else launch(Model<M>{}, std::false_type{}, std::false_type{});
}
template <bool HAS_FX, int FALLBACK, int... MODELS, class F>
static void dispatch(int model, bool tex, bool fx, F &&launch)
{
    // the first listed model that matches launches; `found` says whether one did
    const bool found = ((model == MODELS ? (dispatch_flags<HAS_FX, MODELS>(tex, fx, launch), true) : false) || ...);
    if (!found) dispatch_flags<HAS_FX, FALLBACK>(tex, fx, launch);
}
// k_wavefront exists for FIN, P13 and P12; anything that is neither FIN nor P12 takes P13
static void launch_wavefront(hipStream_t st, int grid, const ShadeCtx &C, const PrimaryArgs &A)
{
    dispatch<true, RT_SHADE_P13, RT_SHADE_FIN, RT_SHADE_P12>(C.P.shade_model, scene_textured(C.S), C.fx != nullptr, [&](auto m, auto tex, auto fx) {
        hipLaunchKernelGGL((k_wavefront<m(), tex(), fx()>), dim3(grid), dim3(RT_BLOCK), 0, st, C, A);
    });
}

void rtk_launch_primary(hipStream_t st, const DevScene &S, const DevWork &W, const rt_params &P, const RenderPass &pass, int max_blocks)
{
    ShadeCtx C = make_ctx(S, W, P, 1, pass.fx);
    PrimaryArgs A; A.cam = pass.cam; A.tiles = pass.tiles; A.q0 = pass.q0; A.npix = pass.npix; A.j0 = pass.j0; A.ns = pass.ns;
    A.max_sample = pass.max_sample; A.mode = pass.mode; A.rays = pass.rays; A.lds_rays = env_lds_rays();
    tiles_prepare(A.tiles);
    A.div_ns = fastdiv_make((uint32_t)(pass.ns > 0 ? pass.ns : 1));
    C.sm = make_slotmap(pass, A.tiles);
    const unsigned long long samples = (unsigned long long)pass.npix * pass.ns;
    // default: the whole ray tree in one persistent launch with LDS ray stacks (FIN / P13 / P12 models); RT_TRACER=levels: one
    // launch per level of the tree (round 1's structure, kept for the other models and for A/B: DESIGN.md section 3)
    if (rtk_wavefront_usable(S, P)) { launch_wavefront(st, grid_for(samples, RT_BLOCK, wavefront_blocks(S)), C, A); return; }
    const int grid = grid_for(samples, RT_BLOCK, max_blocks);
    dispatch<true, RT_SHADE_FIN, RT_SHADE_P13, RT_SHADE_P12, RT_SHADE_P6, RT_SHADE_P3>(P.shade_model, scene_textured(S), pass.fx != nullptr, [&](auto m, auto tex, auto fx) {
        hipLaunchKernelGGL((k_primary<m(), tex(), fx()>), dim3(grid), dim3(RT_BLOCK), 0, st, C, A);
    });
}

bool rtk_launch_wavefront_queue(hipStream_t st, const DevScene &S, const DevWork &W, const rt_params &P, const RenderPass &pass)
{
    if (!env_queue_pass() || !rtk_wavefront_usable(S, P)) return false;
    ShadeCtx C = make_ctx(S, W, P, 2, pass.fx);
    DevTiles tp = pass.tiles;
    tiles_prepare(tp);
    C.sm = make_slotmap(pass, tp);
    PrimaryArgs A;
    memset(&A, 0, sizeof A);
    A.mode = 3; A.ns = 1; A.qsrc = W.rq[1]; A.qsrc_count = W.counts + 1; A.lds_rays = env_lds_rays();
    A.div_ns = fastdiv_make(1u);
    launch_wavefront(st, wavefront_blocks(S), C, A);       // the count is on the device: a full persistent grid, idle workgroups leave at once
    return true;
}

void rtk_launch_bounce(hipStream_t st, const DevScene &S, const DevWork &W, const rt_params &P, int level, int max_blocks, unsigned long long *fx)
{
    if (P.shade_model == RT_SHADE_P3) return;                // P3 has no secondary rays (and no k_bounce)
    const ShadeCtx C = make_ctx(S, W, P, level + 1, fx);
    const DevRayQueue &qin = W.rq[level & 1];
    dispatch<true, RT_SHADE_FIN, RT_SHADE_P13, RT_SHADE_P12, RT_SHADE_P6>(P.shade_model, scene_textured(S), fx != nullptr, [&](auto m, auto tex, auto fx_) {
        hipLaunchKernelGGL((k_bounce<m(), tex(), fx_()>), dim3(max_blocks), dim3(RT_BLOCK), 0, st, C, qin, level);
    });
}

// The grid stays within RT_TRACE_BLOCKS <= RT_SPILL_BLOCKS, like every launch that uses the spill part of the traversal stack.
void rtk_launch_features(hipStream_t st, const DevScene &S, const DevWork &W, const rt_params &P, const RenderPass &pass,
                         uint8_t *second, const DevFeatures &out, bool by_walk)
{
    const uint32_t npix = pass.npix;
    if (npix == 0) return;
    (void)hipMemsetAsync(second, 0, npix, st);
    if (P.max_sample > P.min_sample) hipLaunchKernelGGL(k_mark_second, dim3(grid_for(npix, 256, 1024)), dim3(256), 0, st, W, second, npix);
    const ShadeCtx C = make_ctx(S, W, P);
    FeatureArgs F; F.cam = pass.cam; F.tiles = pass.tiles; F.q0 = pass.q0; F.npix = npix; F.min_sample = P.min_sample; F.max_sample = P.max_sample;
    tiles_prepare(F.tiles);
    F.div_ms = fastdiv_make((uint32_t)(P.max_sample > 0 ? P.max_sample : 1));
    F.second = second; F.by_walk = by_walk ? 1 : 0;
    F.normal = out.normal; F.albedo = out.albedo; F.alpha = out.alpha; F.object_id = out.object_id;
    const int grid = grid_for(npix, RT_BLOCK, RT_TRACE_BLOCKS);
    dispatch<false, RT_SHADE_FIN, RT_SHADE_P13, RT_SHADE_P12, RT_SHADE_P6, RT_SHADE_P3>(P.shade_model, scene_textured(S), false, [&](auto m, auto tex, auto) {
        hipLaunchKernelGGL((k_features<m(), tex()>), dim3(grid), dim3(RT_BLOCK), 0, st, C, F);
    });
}
