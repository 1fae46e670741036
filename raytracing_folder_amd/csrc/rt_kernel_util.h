// rt_kernel_util.h -- the few helpers that more than one kernel translation unit (rt_kernels.hip through rt_trace.h, rt_trace.hip,
// rt_resolve.hip, rt_gather.hip, rt_denoise.hip, ...) uses.  Device code, except grid_for, which the launch wrappers of three units
// size their grids with.  Not a general utility header: a helper moves here when a second file needs it (what only the two
// tile-gather stages share is in rt_tile_gather.h).
#ifndef RT_KERNEL_UTIL_H
#define RT_KERNEL_UTIL_H

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>

// workgroups for `work` items at `block` per workgroup: at least one, at most max_blocks (the kernels stride over the rest)
static inline int grid_for(unsigned long long work, int block, int max_blocks)
{
    const unsigned long long b = (work + block - 1) / block;
    return (int)std::min<unsigned long long>(std::max<unsigned long long>(b, 1), (unsigned long long)max_blocks);
}

// the lanes where a condition holds: the builtin keeps the condition a lane mask (one s_and with exec); HIP's
// __ballot(int) round-trips it through a 0/1 register (v_cndmask + v_cmp_ne per call, on the VALU the gather is bound by)
__device__ __forceinline__ unsigned long long ballot64(bool pred) { return __builtin_amdgcn_ballot_w64(pred); }
// how many lanes of a mask lie below this one: v_mbcnt_lo + v_mbcnt_hi
__device__ __forceinline__ uint32_t lanes_below(unsigned long long m) { return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u)); }

// Reproducible mode (RT_RENDER_REPRODUCIBLE): a contribution that is not a sample's primary one goes into the secondary plane as
// a 32.32 fixed-point integer, rounded to nearest-even, saturated at +-2^31, NaN as 0.  Integer adds are associative, so the
// sum does not depend on the order the atomics arrive in; the plane is folded into sample_rgb once per pass (k_fold_fx).
#define RT_FX_ONE 4294967296.0f          /* 2^32: 32 fractional bits */
__device__ __forceinline__ unsigned long long fx_encode(float c)
{
    const float x = rintf(c * RT_FX_ONE);                 // exact scaling (a power of two), then round to an integer
    if (!(x == x)) return 0ull;
    if (x >= 9223372036854775807.0f) return 0x7FFFFFFFFFFFFFFFull;       // 2^63 as a float
    if (x <= -9223372036854775808.0f) return 0x8000000000000000ull;
    return (unsigned long long)(long long)x;
}
__device__ __forceinline__ void fx_add(unsigned long long *dst, float r, float g, float b)
{
    atomicAdd(dst, fx_encode(r)); atomicAdd(dst + 1, fx_encode(g)); atomicAdd(dst + 2, fx_encode(b));    // global_atomic_add_u64
}

// One channel of the Color24 pack (cyColor.h:245-246) as k_resolve and the denoiser's RGB8 output apply it after gamma:
// r * 255 truncated, clamped to [0, 255], NaN as 0.
__device__ __forceinline__ uint8_t float_to_byte(float r)
{
    const float s = r * 255;
    if (!(s == s)) return 0;
    if (s <= -2147483648.0f) return 0;
    if (s >= 2147483647.0f) return 255;
    const int v = (int)s;
    return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// step 1 of "exposure and tone mapping" (rt_mi355x.h), which "bloom" takes its luminance from:
// Y = ((0.2126 r) + (0.7152 g)) + (0.0722 b), every product and sum rounded to float on its own
__device__ __forceinline__ float tonemap_luminance(float r, float g, float b)
{
    return __fadd_rn(__fadd_rn(__fmul_rn(0.2126f, r), __fmul_rn(0.7152f, g)), __fmul_rn(0.0722f, b));
}

#endif
