// rt_tonemap.hip -- auto-exposure and tone mapping: the last image-space stage, from a linear plane to what a display takes.  The
// definition the kernels follow step by step is in include/rt_mi355x.h ("exposure and tone mapping"); the reference has no
// counterpart.  It is the first image-space stage that reduces over the whole frame (a luminance histogram), hence three kernels
// on one stream, each its own launch -- stream order is all the visibility they need:
//
//   k_luminance_hist   grid-stride pass over the frame: luminance (products and sums rounded one by one), the bin off the bit
//                      pattern, integer atomicAdd into a 256-bin histogram in LDS, then the non-empty bins into the state's 256
//                      words with integer global atomics.  Integer sums are associative: the histogram does not depend on the
//                      order workgroups or atomics arrive in.
//   k_exposure_meter   one workgroup: prefix counts, the percentile window [lo, hi) in integers, Lbar, target, adaptation; copies
//                      the histogram to the "last metered" copy and leaves the working one zero for the next call.
//   k_tonemap<OP>      one lane per pixel: scale (loaded from the state -- no host synchronisation), the operator, the float
//                      display plane and / or the gamma-encoded bytes.  A lane reads its pixel before it writes it (in place).
//
// A flat wall or a background puts most of a wave into one bin, and a ds_add of 64 lanes on one address is taken one lane after
// the other.  RT_TONEMAP_HIST selects what is done about it:
//   0  one histogram per workgroup, every metered lane adds 1 (the default)
//   1  one sub-histogram per wave (the waves of a workgroup do not meet; a wave's own lanes still do)
//   2  the lanes whose bin equals the first metered lane's are added by that lane as one count, the others add 1 each
// Measured on the MI355X at 1080p (tools_tonemap_timing.py; `make variant NAME=x DEFS=-DRT_TONEMAP_HIST=1` builds
// the others): 0 and 1 agree within 0.3 us, 2 is 1.3 us slower, and the constant frame is the faster one on all three -- so the
// plainest one is the default.  What does matter is the number of workgroups (RT_TONEMAP_HIST_MAX_BLOCKS, same tool):
// 2048 / 1024 / 512 / 256 take 32.0 / 21.8 / 18.6 / 20.4 us on the Cornell frame and 28.6 / 19.6 / 15.5 / 19.4 us on the constant one.
// No fast intrinsics (powf, exp2, IEEE division); contraction is off for the whole library and step 1 pins it with __fmul_rn /
// __fadd_rn on top.
#include <hip/hip_runtime.h>

#include "rt_kernel_util.h"
#include "rt_launch.h"

#ifndef RT_TONEMAP_HIST
#define RT_TONEMAP_HIST 0
#endif
#define RT_TONEMAP_BLOCK 256
#ifndef RT_TONEMAP_HIST_MAX_BLOCKS
#define RT_TONEMAP_HIST_MAX_BLOCKS 512      /* 2 per CU, the fastest measured: beyond it the lanes go round the grid-stride loop */
#endif
#define RT_TONEMAP_MIN_Y 1.52587890625e-05f /* 2^-16: the low end of the metered range */

typedef ToneMapRequest::State ExposureState;

__global__ __launch_bounds__(RT_TONEMAP_BLOCK) void k_luminance_hist(const float *rgb, const int32_t *object_id, uint32_t n, uint32_t *hist)
{
#if RT_TONEMAP_HIST == 1
    __shared__ uint32_t h[RT_TONEMAP_BLOCK / 64][256];
    for (int w = 0; w < RT_TONEMAP_BLOCK / 64; w++) h[w][threadIdx.x] = 0;
    uint32_t *mine = h[threadIdx.x >> 6];
#else
    __shared__ uint32_t h[256];
    h[threadIdx.x] = 0;
    uint32_t *mine = h;
#endif
    __syncthreads();
    // n <= 2^30 and the stride <= 2^17: p0 + stride does not wrap.  The loop is the same for every lane of a wave (ballots).
    const uint32_t stride = gridDim.x * RT_TONEMAP_BLOCK;
    for (uint32_t p0 = blockIdx.x * RT_TONEMAP_BLOCK; p0 < n; p0 += stride) {
        const uint32_t p = p0 + threadIdx.x;
        bool metered = false;
        uint32_t bin = 0;
        if (p < n) {
            const float *px = rgb + (size_t)p * 3;
            const float Y = tonemap_luminance(px[0], px[1], px[2]);
            // step 2: id >= 0, Y finite, Y >= 2^-16 (a NaN fails both comparisons); then Y is positive and its bits order like it
            metered = (!object_id || object_id[p] >= 0) && Y >= RT_TONEMAP_MIN_Y && Y < INFINITY;
            const uint32_t b = (__float_as_uint(Y) >> 20) - 888u;
            bin = b < 255u ? b : 255u;
        }
#if RT_TONEMAP_HIST == 2
        const unsigned long long any = ballot64(metered);
        if (any) {
            const int leader = __builtin_ctzll(any);
            const uint32_t lbin = (uint32_t)__builtin_amdgcn_readlane((int)bin, leader);
            const unsigned long long same = ballot64(metered && bin == lbin);
            if ((int)(threadIdx.x & 63) == leader) atomicAdd(&mine[lbin], (uint32_t)__popcll(same));
            else if (metered && bin != lbin) atomicAdd(&mine[bin], 1u);
        }
#else
        if (metered) atomicAdd(&mine[bin], 1u);
#endif
    }
    __syncthreads();
#if RT_TONEMAP_HIST == 1
    uint32_t c = 0;
    for (int w = 0; w < RT_TONEMAP_BLOCK / 64; w++) c += h[w][threadIdx.x];
#else
    const uint32_t c = h[threadIdx.x];
#endif
    if (c) atomicAdd(&hist[threadIdx.x], c);
}

// what k_exposure_meter needs of the parameters (validated by the caller)
struct MeterArgs {
    double log2_key;
    float ev_bias, ev_min, ev_max, p_low, p_high, adapt_up, adapt_down;
};

__device__ __forceinline__ double meter_clamp(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }

// steps 3-5, one workgroup of 256 lanes, lane b owns bin b
__global__ __launch_bounds__(256) void k_exposure_meter(ExposureState *S, MeterArgs A)
{
    __shared__ uint32_t cum[256];
    __shared__ unsigned long long part[256];
    const uint32_t b = threadIdx.x;
    const uint32_t hb = S->hist[b];
    S->last[b] = hb;
    S->hist[b] = 0;                     // the working histogram of the next call
    cum[b] = hb;
    __syncthreads();
    for (uint32_t d = 1; d < 256; d <<= 1) {        // inclusive prefix counts (n <= 2^30: no overflow)
        const uint32_t v = b >= d ? cum[b - d] : 0u;
        __syncthreads();
        cum[b] += v;
        __syncthreads();
    }
    const uint32_t n = cum[255], cb = cum[b] - hb;
    if (n == 0) {                       // nothing metered: E stays; with no earlier frame E = clamp(ev_bias)
        if (b == 0) {
            S->n = 0;
            if (!S->holds) {
                const float E = (float)meter_clamp((double)A.ev_bias, (double)A.ev_min, (double)A.ev_max);
                S->E = E;
                S->scale = (float)exp2((double)E);
            }
        }
        return;
    }
    uint32_t lo = (uint32_t)floor((double)A.p_low * (double)n), hi = (uint32_t)ceil((double)A.p_high * (double)n);
    if (hi > n) hi = n;
    if (hi <= lo) hi = lo + 1;          // two percentiles one float apart on a huge frame: rounding could make them meet
    const uint32_t top = cb + hb < hi ? cb + hb : hi, bot = cb > lo ? cb : lo;
    part[b] = (unsigned long long)(top > bot ? top - bot : 0u) * (unsigned long long)(2u * b + 1u);
    __syncthreads();
    for (uint32_t d = 128; d > 0; d >>= 1) {
        if (b < d) part[b] += part[b + d];
        __syncthreads();
    }
    if (b == 0) {
        const double lbar = (double)part[0] / (16.0 * (double)(hi - lo)) - 16.0;
        const double Et = meter_clamp(A.log2_key + (double)A.ev_bias - lbar, (double)A.ev_min, (double)A.ev_max);
        double E = Et;
        if (S->holds) {
            const double Ep = (double)S->E;
            E = Ep + (double)(Et > Ep ? A.adapt_up : A.adapt_down) * (Et - Ep);
        }
        const float Ef = (float)E;
        S->lbar = lbar; S->E = Ef; S->scale = (float)exp2((double)Ef); S->n = n; S->holds = 1;
    }
}

// the kernel's argument: members, order and types are its layout
struct ToneMapArgs {
    const float *rgb; float *out_display; uint8_t *out_rgb8;
    const float *scale_ptr;             // the state's scale; NULL: `scale` (auto_exposure == 0)
    uint32_t n;
    float scale, white2, inv_gamma;
};

__device__ __forceinline__ float tonemap_aces(float x)
{
    const float v = (x * (2.51f * x + 0.03f)) / (x * (2.43f * x + 0.59f) + 0.14f);
    return v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v);         // a NaN stays NaN
}

// step 6
template <int OP>
__global__ __launch_bounds__(RT_TONEMAP_BLOCK) void k_tonemap(ToneMapArgs A)
{
    const uint32_t p = blockIdx.x * RT_TONEMAP_BLOCK + threadIdx.x;
    if (p >= A.n) return;
    const float scale = A.scale_ptr ? *A.scale_ptr : A.scale;
    const size_t i = (size_t)p * 3;
    float r = A.rgb[i] * scale, g = A.rgb[i + 1] * scale, b = A.rgb[i + 2] * scale;
    if (OP == RT_TONEMAP_REINHARD) {
        const float Y = tonemap_luminance(r, g, b);
        if (Y > 0.0f) {
            const float f = (1.0f + Y / A.white2) / (1.0f + Y);
            r *= f; g *= f; b *= f;
        }
    } else if (OP == RT_TONEMAP_ACES) {
        r = tonemap_aces(r); g = tonemap_aces(g); b = tonemap_aces(b);
    }
    if (A.out_display) { A.out_display[i] = r; A.out_display[i + 1] = g; A.out_display[i + 2] = b; }
    if (A.out_rgb8) {
        A.out_rgb8[i] = float_to_byte(powf(r, A.inv_gamma));
        A.out_rgb8[i + 1] = float_to_byte(powf(g, A.inv_gamma));
        A.out_rgb8[i + 2] = float_to_byte(powf(b, A.inv_gamma));
    }
}

void rtk_launch_tonemap(hipStream_t st, const ToneMapRequest &R)
{
    const uint32_t n = (uint32_t)((size_t)R.width * (size_t)R.height);      // <= 2^30 (the caller's check)
    const uint32_t blocks = (n + RT_TONEMAP_BLOCK - 1) / RT_TONEMAP_BLOCK;
    if (R.meter) {
        const uint32_t hist_blocks = blocks < RT_TONEMAP_HIST_MAX_BLOCKS ? blocks : RT_TONEMAP_HIST_MAX_BLOCKS;
        hipLaunchKernelGGL(k_luminance_hist, dim3(hist_blocks), dim3(RT_TONEMAP_BLOCK), 0, st, R.rgb_linear, R.object_id, n, R.state->hist);
        MeterArgs M = {R.log2_key, R.ev_bias, R.ev_min, R.ev_max, R.p_low, R.p_high, R.adapt_up, R.adapt_down};
        hipLaunchKernelGGL(k_exposure_meter, dim3(1), dim3(256), 0, st, R.state, M);
    }
    ToneMapArgs A = {};
    A.rgb = R.rgb_linear; A.out_display = R.out_display; A.out_rgb8 = R.out_rgb8;
    A.scale_ptr = R.meter ? &R.state->scale : nullptr;
    A.n = n; A.scale = R.scale; A.white2 = R.white2; A.inv_gamma = R.inv_gamma;
    switch (R.op) {
    case RT_TONEMAP_CLAMP:    hipLaunchKernelGGL(k_tonemap<RT_TONEMAP_CLAMP>, dim3(blocks), dim3(RT_TONEMAP_BLOCK), 0, st, A); break;
    case RT_TONEMAP_REINHARD: hipLaunchKernelGGL(k_tonemap<RT_TONEMAP_REINHARD>, dim3(blocks), dim3(RT_TONEMAP_BLOCK), 0, st, A); break;
    default:                  hipLaunchKernelGGL(k_tonemap<RT_TONEMAP_ACES>, dim3(blocks), dim3(RT_TONEMAP_BLOCK), 0, st, A); break;
    }
}
