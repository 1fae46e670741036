// rt_bloom.hip -- bloom: the image-space stage ahead of exposure and tone mapping.  The definition the kernels follow step by step
// is in include/rt_mi355x.h ("bloom"); the reference has no counterpart.  A bright pass, a pyramid of halved levels down, a lerp
// per level up again, and the result added to the frame:
//
//   k_bloom_prefilter  a 16 x 16 tile of level 0 per workgroup: the 34 x 34 source pixels it needs go through the bright pass once
//                      each into LDS (scale loaded from the exposure state -- no host synchronisation), then the 4 x 4 taps
//   k_bloom_down       the same tile kernel without the bright pass: level l -> level l + 1
//   k_bloom_tail       (RT_BLOOM_TAIL=1 builds only) ONE workgroup: the first level that fits LDS with everything below it
//                      (RT_BLOOM_TAIL_TEXELS) is loaded, every level below it is built and recombined inside LDS, and that
//                      level's U is written back.  The small levels are a few thousand texels, where a launch costs more than
//                      the work
//   k_bloom_up         U_l = a B_l + spread up(U_{l+1}), in place over B_l, one lane per texel
//   k_bloom_combine    one lane per pixel: out = rgb + intensity up(U_0); a lane reads its pixel before it writes it (in place)
//
// The arithmetic of a texel is one set of device functions (bloom_down_texel, bloom_up_texel, bloom_lerp) whichever kernel runs
// it, so the build with the tail (`make variant NAME=tail DEFS=-DRT_BLOOM_TAIL=1`, or `make bloom_tail`, which compiles this
// file alone) computes the same bits as the shipped one, in which every level is a launch of its own.  Which is faster, and where
// the tail should start, is measured by tools_bloom_timing.py ("Bloom"): at 1080p the call takes 65.3 us
// without the tail, 65.3 us with the tail from level 4 (64 KB) and 69.4 us with the tail from level 3 (156 KB).  The tail does
// not win, so the plainer form is the default.
// No atomics; contraction is off for the whole library and the filters pin it with __fmul_rn / __fadd_rn on top.
#include <hip/hip_runtime.h>

#include "rt_kernel_util.h"
#include "rt_launch.h"

#ifndef RT_BLOOM_TAIL
#define RT_BLOOM_TAIL 0
#endif
#ifndef RT_BLOOM_TAIL_TEXELS
#define RT_BLOOM_TAIL_TEXELS 5461           /* 64 KB of LDS at 12 bytes a texel: a 64 x 64 level and what is below it.  Measured */
                                            /* (DESIGN 3): 13312 texels, 156 KB of gfx950's 160 KB, makes the call 4 us slower    */
#endif
#define RT_BLOOM_BLOCK 256
#define RT_BLOOM_TILE 16                    /* a workgroup's tile of the destination level, 16 x 16 */
#define RT_BLOOM_SRC (2 * RT_BLOOM_TILE + 2) /* and the source texels it reads, 34 x 34 */
#define RT_BLOOM_TAIL_THREADS 1024

typedef ToneMapRequest::State ExposureState;

struct Rgb { float r, g, b; };

// step 3's f(a, b, c, d) = ((a + 3 b) + (3 c + d)) / 8 and g(n, f) = 0.75 n + 0.25 f; step 4's lerp
__device__ __forceinline__ float bloom_f(float a, float b, float c, float d)
{
    return __fmul_rn(__fadd_rn(__fadd_rn(a, __fmul_rn(3.0f, b)), __fadd_rn(__fmul_rn(3.0f, c), d)), 0.125f);
}
__device__ __forceinline__ float bloom_g(float n, float f) { return __fadd_rn(__fmul_rn(0.75f, n), __fmul_rn(0.25f, f)); }
__device__ __forceinline__ Rgb bloom_f(const Rgb &a, const Rgb &b, const Rgb &c, const Rgb &d)
{
    return {bloom_f(a.r, b.r, c.r, d.r), bloom_f(a.g, b.g, c.g, d.g), bloom_f(a.b, b.b, c.b, d.b)};
}
__device__ __forceinline__ Rgb bloom_g(const Rgb &n, const Rgb &f) { return {bloom_g(n.r, f.r), bloom_g(n.g, f.g), bloom_g(n.b, f.b)}; }
__device__ __forceinline__ Rgb bloom_lerp(float a, const Rgb &B, float spread, const Rgb &up)
{
    return {__fadd_rn(__fmul_rn(a, B.r), __fmul_rn(spread, up.r)), __fadd_rn(__fmul_rn(a, B.g), __fmul_rn(spread, up.g)),
            __fadd_rn(__fmul_rn(a, B.b), __fmul_rn(spread, up.b))};
}

__device__ __forceinline__ Rgb bloom_load(const float *plane, size_t texel)
{
    const float *p = plane + texel * 3;
    return {p[0], p[1], p[2]};
}
__device__ __forceinline__ void bloom_store(float *plane, size_t texel, const Rgb &v)
{
    float *p = plane + texel * 3;
    p[0] = v.r; p[1] = v.g; p[2] = v.b;
}

__device__ __forceinline__ int bloom_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// step 3, downsample: texel (i, j) of the level below a w x h source that `fetch(x, y)` reads (x, y inside the source)
template <class Fetch>
__device__ __forceinline__ Rgb bloom_down_texel(Fetch fetch, int w, int h, int i, int j)
{
    const int x0 = bloom_clamp(2 * i - 1, w - 1), x1 = 2 * i, x2 = bloom_clamp(2 * i + 1, w - 1), x3 = bloom_clamp(2 * i + 2, w - 1);
    const int y0 = bloom_clamp(2 * j - 1, h - 1), y1 = 2 * j, y2 = bloom_clamp(2 * j + 1, h - 1), y3 = bloom_clamp(2 * j + 2, h - 1);
    const Rgb r0 = bloom_f(fetch(x0, y0), fetch(x1, y0), fetch(x2, y0), fetch(x3, y0));
    const Rgb r1 = bloom_f(fetch(x0, y1), fetch(x1, y1), fetch(x2, y1), fetch(x3, y1));
    const Rgb r2 = bloom_f(fetch(x0, y2), fetch(x1, y2), fetch(x2, y2), fetch(x3, y2));
    const Rgb r3 = bloom_f(fetch(x0, y3), fetch(x1, y3), fetch(x2, y3), fetch(x3, y3));
    return bloom_f(r0, r1, r2, r3);
}

// step 3, upsample: up(X) at the texel (x, y) of the next finer grid, X being w x h and read by `fetch`
template <class Fetch>
__device__ __forceinline__ Rgb bloom_up_texel(Fetch fetch, int w, int h, int x, int y)
{
    const int nx = x >> 1, fx = (x & 1) ? (nx + 1 < w ? nx + 1 : w - 1) : (nx > 0 ? nx - 1 : 0);
    const int ny = y >> 1, fy = (y & 1) ? (ny + 1 < h ? ny + 1 : h - 1) : (ny > 0 ? ny - 1 : 0);
    return bloom_g(bloom_g(fetch(nx, ny), fetch(fx, ny)), bloom_g(fetch(nx, fy), fetch(fx, fy)));
}

// step 2: what a source pixel contributes.  den = 4 k + 1e-5f, taken once on the host
__device__ __forceinline__ Rgb bloom_bright(Rgb p, float scale, float t, float k, float den)
{
    p.r = (p.r >= 0.0f && p.r < INFINITY) ? p.r : 0.0f;         // a NaN fails the first comparison
    p.g = (p.g >= 0.0f && p.g < INFINITY) ? p.g : 0.0f;
    p.b = (p.b >= 0.0f && p.b < INFINITY) ? p.b : 0.0f;
    if (t == 0.0f) return p;
    const float Ys = __fmul_rn(scale, tonemap_luminance(p.r, p.g, p.b));
    if (!(Ys < INFINITY)) return p;
    const float d = __fsub_rn(Ys, t);
    const float x = fminf(fmaxf(__fadd_rn(d, k), 0.0f), 2.0f * k);
    const float s = __fmul_rn(x, x) / den;
    const float wgt = fmaxf(s, d) / fmaxf(Ys, 1e-5f);
    return {__fmul_rn(p.r, wgt), __fmul_rn(p.g, wgt), __fmul_rn(p.b, wgt)};
}

// the kernels' arguments: members, order and types are their layout
struct BloomDownArgs {
    const float *src; float *dst;       // sw x sh -> dw x dh = ceil(sw / 2) x ceil(sh / 2)
    int sw, sh, dw, dh;
    uint32_t tiles_x;
    const ExposureState *state;         // k_bloom_prefilter only, as are the rest
    float scale, t, k, den;
};

// A 16 x 16 tile of the destination per workgroup.  The tile's source texels, clamped to the source's edge as the definition
// clamps them, are staged in LDS (PRE: after the bright pass, which a pixel then goes through once instead of four times).
template <bool PRE>
__device__ __forceinline__ void bloom_down_tile(const BloomDownArgs &A, float (*tile)[3])
{
    const uint32_t tyi = blockIdx.x / A.tiles_x, txi = blockIdx.x - tyi * A.tiles_x;
    const int ox0 = (int)txi * RT_BLOOM_TILE, oy0 = (int)tyi * RT_BLOOM_TILE;
    float scale = 0.0f;
    if (PRE) scale = (A.state && A.state->holds) ? A.state->scale : A.scale;
    for (int idx = threadIdx.x; idx < RT_BLOOM_SRC * RT_BLOOM_SRC; idx += RT_BLOOM_BLOCK) {
        const int ty = idx / RT_BLOOM_SRC, tx = idx - ty * RT_BLOOM_SRC;
        const int sx = bloom_clamp(2 * ox0 - 1 + tx, A.sw - 1), sy = bloom_clamp(2 * oy0 - 1 + ty, A.sh - 1);
        Rgb p = bloom_load(A.src, (size_t)sy * (size_t)A.sw + (size_t)sx);
        if (PRE) p = bloom_bright(p, scale, A.t, A.k, A.den);
        tile[idx][0] = p.r; tile[idx][1] = p.g; tile[idx][2] = p.b;
    }
    __syncthreads();
    const int lx = threadIdx.x & (RT_BLOOM_TILE - 1), ly = threadIdx.x / RT_BLOOM_TILE;
    const int ox = ox0 + lx, oy = oy0 + ly;
    if (ox >= A.dw || oy >= A.dh) return;
    // tile column c holds the source column clamp(2 ox0 - 1 + c): the four taps of ox are columns 2 lx .. 2 lx + 3
    auto at = [&](int c, int r) { const float *p = tile[(2 * ly + r) * RT_BLOOM_SRC + 2 * lx + c]; return Rgb{p[0], p[1], p[2]}; };
    const Rgb r0 = bloom_f(at(0, 0), at(1, 0), at(2, 0), at(3, 0));
    const Rgb r1 = bloom_f(at(0, 1), at(1, 1), at(2, 1), at(3, 1));
    const Rgb r2 = bloom_f(at(0, 2), at(1, 2), at(2, 2), at(3, 2));
    const Rgb r3 = bloom_f(at(0, 3), at(1, 3), at(2, 3), at(3, 3));
    bloom_store(A.dst, (size_t)oy * (size_t)A.dw + (size_t)ox, bloom_f(r0, r1, r2, r3));
}

__global__ __launch_bounds__(RT_BLOOM_BLOCK) void k_bloom_prefilter(BloomDownArgs A)
{
    __shared__ float tile[RT_BLOOM_SRC * RT_BLOOM_SRC][3];
    bloom_down_tile<true>(A, tile);
}

__global__ __launch_bounds__(RT_BLOOM_BLOCK) void k_bloom_down(BloomDownArgs A)
{
    __shared__ float tile[RT_BLOOM_SRC * RT_BLOOM_SRC][3];
    bloom_down_tile<false>(A, tile);
}

struct BloomUpArgs {
    float *fine; const float *coarse;   // B_l -> U_l in place (fw x fh); U_{l+1} (cw x ch)
    int fw, fh, cw, ch;
    uint32_t n;                         // fw * fh
    float a, spread;
};

__global__ __launch_bounds__(RT_BLOOM_BLOCK) void k_bloom_up(BloomUpArgs A)
{
    const uint32_t t = blockIdx.x * RT_BLOOM_BLOCK + threadIdx.x;
    if (t >= A.n) return;
    const int y = (int)(t / (uint32_t)A.fw), x = (int)(t - (uint32_t)y * (uint32_t)A.fw);
    const Rgb up = bloom_up_texel([&](int cx, int cy) { return bloom_load(A.coarse, (size_t)cy * (size_t)A.cw + (size_t)cx); }, A.cw, A.ch, x, y);
    bloom_store(A.fine, t, bloom_lerp(A.a, bloom_load(A.fine, t), A.spread, up));
}

#if RT_BLOOM_TAIL
struct BloomTailArgs {
    float *level;                       // B_T in, U_T out (w x h)
    int w, h, m;                        // m >= 2 levels: T .. T + m - 1; their texels together <= RT_BLOOM_TAIL_TEXELS
    float a, spread;
};

// Levels T .. T + m - 1 one behind the other in LDS, 3 floats a texel (a stride of 3 words: a wave's lanes fall on different banks).
__global__ __launch_bounds__(RT_BLOOM_TAIL_THREADS) void k_bloom_tail(BloomTailArgs A)
{
    extern __shared__ float lds[];
    const uint32_t n0 = (uint32_t)A.w * (uint32_t)A.h;
    for (uint32_t i = threadIdx.x; i < n0 * 3; i += RT_BLOOM_TAIL_THREADS) lds[i] = A.level[i];
    __syncthreads();
    int w = A.w, h = A.h;
    uint32_t off = 0;
    for (int l = 1; l < A.m; l++) {                             // down: level l from level l - 1
        const int w2 = (w + 1) >> 1, h2 = (h + 1) >> 1;
        const uint32_t off2 = off + (uint32_t)w * (uint32_t)h, n2 = (uint32_t)w2 * (uint32_t)h2;
        const float *src = lds + off * 3;
        float *dst = lds + off2 * 3;
        for (uint32_t t = threadIdx.x; t < n2; t += RT_BLOOM_TAIL_THREADS) {
            const int j = (int)(t / (uint32_t)w2), i = (int)(t - (uint32_t)j * (uint32_t)w2);
            bloom_store(dst, t, bloom_down_texel([&](int x, int y) { return bloom_load(src, (size_t)(y * w + x)); }, w, h, i, j));
        }
        __syncthreads();
        w = w2; h = h2; off = off2;
    }
    for (int l = A.m - 2; l >= 0; l--) {                        // up: U_l over B_l from U_{l+1}
        int fw = A.w, fh = A.h;
        uint32_t foff = 0;
        for (int q = 0; q < l; q++) { foff += (uint32_t)fw * (uint32_t)fh; fw = (fw + 1) >> 1; fh = (fh + 1) >> 1; }
        const int cw = (fw + 1) >> 1, ch = (fh + 1) >> 1;
        const uint32_t n = (uint32_t)fw * (uint32_t)fh;
        float *fine = lds + foff * 3;
        const float *coarse = lds + (foff + n) * 3;
        for (uint32_t t = threadIdx.x; t < n; t += RT_BLOOM_TAIL_THREADS) {
            const int y = (int)(t / (uint32_t)fw), x = (int)(t - (uint32_t)y * (uint32_t)fw);
            const Rgb up = bloom_up_texel([&](int cx, int cy) { return bloom_load(coarse, (size_t)(cy * cw + cx)); }, cw, ch, x, y);
            bloom_store(fine, t, bloom_lerp(A.a, bloom_load(fine, t), A.spread, up));
        }
        __syncthreads();
    }
    for (uint32_t i = threadIdx.x; i < n0 * 3; i += RT_BLOOM_TAIL_THREADS) A.level[i] = lds[i];
}

#endif

struct BloomCombineArgs {
    const float *rgb; float *out, *out_bloom;
    const float *u0;                    // U_0, w0 x h0
    int width, w0, h0;
    uint32_t n;                         // width * height <= 2^30
    float intensity;
};

__global__ __launch_bounds__(RT_BLOOM_BLOCK) void k_bloom_combine(BloomCombineArgs A)
{
    const uint32_t p = blockIdx.x * RT_BLOOM_BLOCK + threadIdx.x;
    if (p >= A.n) return;
    const int y = (int)(p / (uint32_t)A.width), x = (int)(p - (uint32_t)y * (uint32_t)A.width);
    const Rgb up = bloom_up_texel([&](int cx, int cy) { return bloom_load(A.u0, (size_t)cy * (size_t)A.w0 + (size_t)cx); }, A.w0, A.h0, x, y);
    if (A.out) {
        const Rgb c = bloom_load(A.rgb, p);
        bloom_store(A.out, p, {__fadd_rn(c.r, __fmul_rn(A.intensity, up.r)), __fadd_rn(c.g, __fmul_rn(A.intensity, up.g)),
                               __fadd_rn(c.b, __fmul_rn(A.intensity, up.b))});
    }
    if (A.out_bloom) bloom_store(A.out_bloom, p, up);
}

BloomPlan rtk_bloom_plan(int width, int height, int levels)
{
    BloomPlan P = {};
    int w = (width + 1) / 2, h = (height + 1) / 2, l = 0;
    size_t off = 0;
    for (;;) {
        P.w[l] = w; P.h[l] = h; P.off[l] = off;
        off += (size_t)w * (size_t)h;
        l++;
        if (l >= levels || l >= RT_BLOOM_MAX_LEVELS || (w == 1 && h == 1)) break;
        w = (w + 1) / 2; h = (h + 1) / 2;
    }
    P.levels = l; P.off[l] = off; P.tail = -1;
#if RT_BLOOM_TAIL
    for (int t = 0; t < l - 1; t++)                             // the first level that fits with everything below it; at least two levels
        if (off - P.off[t] <= (size_t)RT_BLOOM_TAIL_TEXELS) { P.tail = t; break; }
#endif
    return P;
}

static uint32_t bloom_blocks(size_t n) { return (uint32_t)((n + RT_BLOOM_BLOCK - 1) / RT_BLOOM_BLOCK); }

hipError_t rtk_launch_bloom(hipStream_t st, const BloomRequest &R)
{
    const BloomPlan &P = R.plan;
    const int L = P.levels, T = P.tail;
    auto level = [&](int l) { return R.pyramid + P.off[l] * 3; };
    auto tiles = [&](int l) { return dim3((uint32_t)((P.w[l] + RT_BLOOM_TILE - 1) / RT_BLOOM_TILE) * (uint32_t)((P.h[l] + RT_BLOOM_TILE - 1) / RT_BLOOM_TILE)); };
    BloomDownArgs D = {};
    D.src = R.rgb_linear; D.dst = level(0); D.sw = R.width; D.sh = R.height; D.dw = P.w[0]; D.dh = P.h[0];
    D.tiles_x = (uint32_t)((P.w[0] + RT_BLOOM_TILE - 1) / RT_BLOOM_TILE);
    D.state = R.state; D.scale = R.scale; D.t = R.threshold; D.k = R.knee_k; D.den = 4.0f * R.knee_k + 1e-5f;
    hipLaunchKernelGGL(k_bloom_prefilter, tiles(0), dim3(RT_BLOOM_BLOCK), 0, st, D);
    const int deepest = T >= 0 ? T : L - 1;                     // the last level that gets a launch of its own on the way down
    for (int l = 1; l <= deepest; l++) {
        BloomDownArgs A = {};
        A.src = level(l - 1); A.dst = level(l); A.sw = P.w[l - 1]; A.sh = P.h[l - 1]; A.dw = P.w[l]; A.dh = P.h[l];
        A.tiles_x = (uint32_t)((P.w[l] + RT_BLOOM_TILE - 1) / RT_BLOOM_TILE);
        hipLaunchKernelGGL(k_bloom_down, tiles(l), dim3(RT_BLOOM_BLOCK), 0, st, A);
    }
#if RT_BLOOM_TAIL
    if (T >= 0) {
        const size_t bytes = (P.off[L] - P.off[T]) * 12;        // <= RT_BLOOM_TAIL_TEXELS * 12 by the plan
        if (bytes > 65536) {            // only a build with RT_BLOOM_TAIL_TEXELS above 5461 asks for more than a launch gets by default
            const hipError_t e = hipFuncSetAttribute((const void *)k_bloom_tail, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
            if (e != hipSuccess) return e;
        }
        const BloomTailArgs A = {level(T), P.w[T], P.h[T], L - T, R.one_minus_spread, R.spread};
        hipLaunchKernelGGL(k_bloom_tail, dim3(1), dim3(RT_BLOOM_TAIL_THREADS), bytes, st, A);
    }
#endif
    for (int l = (T >= 0 ? T : L - 1) - 1; l >= 0; l--) {
        const uint32_t n = (uint32_t)((size_t)P.w[l] * (size_t)P.h[l]);
        const BloomUpArgs A = {level(l), level(l + 1), P.w[l], P.h[l], P.w[l + 1], P.h[l + 1], n, R.one_minus_spread, R.spread};
        hipLaunchKernelGGL(k_bloom_up, dim3(bloom_blocks(n)), dim3(RT_BLOOM_BLOCK), 0, st, A);
    }
    BloomCombineArgs C = {};
    C.rgb = R.rgb_linear; C.out = R.out; C.out_bloom = R.out_bloom; C.u0 = level(0);
    C.width = R.width; C.w0 = P.w[0]; C.h0 = P.h[0];
    C.n = (uint32_t)((size_t)R.width * (size_t)R.height);       // <= 2^30 (the caller's check)
    C.intensity = R.intensity;
    hipLaunchKernelGGL(k_bloom_combine, dim3(bloom_blocks(C.n)), dim3(RT_BLOOM_BLOCK), 0, st, C);
    return hipGetLastError();
}
