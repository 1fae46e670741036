// rt_motion_blur.hip -- motion blur: the image-space stage between the denoise and bloom.  The definition the kernels follow step
// by step is in include/rt_mi355x.h ("motion blur"); the reference has no counterpart.  Three launches per frame:
//
//   k_mblur_tile_max        one wave per K x K tile: the lanes stride over the tile's pixels (12 bytes of the motion plane each), keep
//                           their best (m, pixel index) key, and six xor-shuffles reduce the wave.  (max m, then min index) is
//                           associative, so the result does not depend on how the pixels were dealt to the lanes
//   k_mblur_neighbour_max   one lane per tile: the largest m of the 3 x 3 tile-max values around it, first in row-major order
//   k_mblur_gather          one lane per pixel.  A workgroup covers a square of whole tiles (G x G of them, G = 16 / K, one tile from
//                           K = 9 on), so the neighbour-max vector and the early out are uniform over a wave wherever K allows: a
//                           static frame costs 12 bytes in and 12 out per pixel here, and a wave in flight takes the N taps together.
//                           A tap reads 28 bytes (motion, z, colour) of a pixel that the lanes beside it read as well; the taps
//                           go through the caches, nothing is staged in LDS
//
// No atomics, fixed orders; contraction is off for the whole library and the arithmetic pins it with __fmul_rn / __fadd_rn on top.
// sqrtf and the divisions are the correctly rounded ones (hipcc's default, -fhip-fp32-correctly-rounded-divide-sqrt).
#include <hip/hip_runtime.h>
#include <math.h>

#include "rt_kernel_util.h"
#include "rt_launch.h"

#define RT_MBLUR_BLOCK 256
#define RT_MBLUR_GROUP 16                   /* the side a gather workgroup's square reaches while it holds more than one tile        */
#define RT_MBLUR_FAR 1.0e30f                /* the z plane's "nothing hit" (BIGFLOAT); what every z that is not finite counts as */

// the kernels' argument: members, order and types are its layout
struct MblurArgs {
    int width, height, K, N;
    int tiles_x, tiles_y;
    int side, groups_x;                 // k_mblur_gather: the pixels along a workgroup's square, and the squares along x
    float h, g, depth_extent, Kf, KK;   // 0.5f * shutter, 2 / N, (float)K, (float)(K * K)
    const float *rgb, *motion, *z;
    float *out, *out_tiles;
    float *tile_max, *tile_nmax;        // [tiles_x * tiles_y * 2]
};

struct Vel { float x, y, m; };

__device__ __forceinline__ bool mblur_finite(float a) { return fabsf(a) < INFINITY; }         // false for a NaN
__device__ __forceinline__ float mblur_m(float vx, float vy) { return __fadd_rn(__fmul_rn(vx, vx), __fmul_rn(vy, vy)); }

// step 1: the velocity of the pixel (x, y), p = y * width + x
__device__ __forceinline__ Vel mblur_velocity(const float *motion, size_t p, int x, int y, float h)
{
    const float *mv = motion + 3 * p;
    const float fx = mv[0], fy = mv[1], ze = mv[2];
    const bool ok = ze > 0.0f && mblur_finite(fx) && mblur_finite(fy) && mblur_finite(ze);
    Vel v;
    v.x = ok ? __fmul_rn(h, __fsub_rn((float)x, fx)) : 0.0f;
    v.y = ok ? __fmul_rn(h, __fsub_rn((float)y, fy)) : 0.0f;
    v.m = mblur_m(v.x, v.y);
    return v;
}

// step 2
__global__ __launch_bounds__(RT_MBLUR_BLOCK) void k_mblur_tile_max(MblurArgs A)
{
    const int lane = (int)(threadIdx.x & 63u);
    const uint32_t tile = blockIdx.x * (RT_MBLUR_BLOCK / 64) + (threadIdx.x >> 6);
    if (tile >= (uint32_t)A.tiles_x * (uint32_t)A.tiles_y) return;     // the whole wave
    const int ty = (int)(tile / (uint32_t)A.tiles_x), tx = (int)(tile - (uint32_t)ty * (uint32_t)A.tiles_x);
    const int x0 = tx * A.K, y0 = ty * A.K;
    const int tw = min(A.K, A.width - x0), th = min(A.K, A.height - y0);
    float bm = -1.0f, bx = 0.0f, by = 0.0f;                     // no pixel yet: below every m
    uint32_t bi = 0xffffffffu;
    for (int k = lane; k < tw * th; k += 64) {                  // in rising pixel index: `>` keeps the lowest among equals
        const int ly = k / tw, lx = k - ly * tw;
        const size_t p = (size_t)(y0 + ly) * (size_t)A.width + (size_t)(x0 + lx);
        const Vel v = mblur_velocity(A.motion, p, x0 + lx, y0 + ly, A.h);
        if (v.m > bm) { bm = v.m; bx = v.x; by = v.y; bi = (uint32_t)p; }
    }
    for (int off = 32; off > 0; off >>= 1) {
        const float om = __shfl_xor(bm, off), ox = __shfl_xor(bx, off), oy = __shfl_xor(by, off);
        const uint32_t oi = (uint32_t)__shfl_xor((int)bi, off);
        if (om > bm || (om == bm && oi < bi)) { bm = om; bx = ox; by = oy; bi = oi; }
    }
    if (lane == 0) { A.tile_max[2 * (size_t)tile] = bx; A.tile_max[2 * (size_t)tile + 1] = by; }
}

// step 3
__global__ __launch_bounds__(RT_MBLUR_BLOCK) void k_mblur_neighbour_max(MblurArgs A)
{
    const uint32_t tile = blockIdx.x * RT_MBLUR_BLOCK + threadIdx.x;
    if (tile >= (uint32_t)A.tiles_x * (uint32_t)A.tiles_y) return;
    const int ty = (int)(tile / (uint32_t)A.tiles_x), tx = (int)(tile - (uint32_t)ty * (uint32_t)A.tiles_x);
    float bm = -1.0f, bx = 0.0f, by = 0.0f;
    for (int dy = -1; dy <= 1; dy++)
        for (int dx = -1; dx <= 1; dx++) {
            const int nx = tx + dx, ny = ty + dy;
            if (nx < 0 || ny < 0 || nx >= A.tiles_x || ny >= A.tiles_y) continue;
            const size_t t = (size_t)ny * (size_t)A.tiles_x + (size_t)nx;
            const float vx = A.tile_max[2 * t], vy = A.tile_max[2 * t + 1];
            const float m = mblur_m(vx, vy);
            if (m > bm) { bm = m; bx = vx; by = vy; }
        }
    A.tile_nmax[2 * (size_t)tile] = bx; A.tile_nmax[2 * (size_t)tile + 1] = by;
    if (A.out_tiles) { A.out_tiles[2 * (size_t)tile] = bx; A.out_tiles[2 * (size_t)tile + 1] = by; }
}

// steps 4 and 6: lenK, and the three weight functions
__device__ __forceinline__ float mblur_len(float m, float Kf) { return fminf(sqrtf(m), Kf); }
__device__ __forceinline__ float mblur_clamp01(float a) { return fminf(fmaxf(a, 0.0f), 1.0f); }
__device__ __forceinline__ float mblur_cone(float d, float l) { return mblur_clamp01(__fsub_rn(1.0f, d / l)); }
__device__ __forceinline__ float mblur_cyl(float d, float l)
{
    const float e0 = __fmul_rn(0.95f, l), e1 = __fmul_rn(1.05f, l);
    const float u = mblur_clamp01(__fsub_rn(d, e0) / __fsub_rn(e1, e0));
    return __fsub_rn(1.0f, __fmul_rn(__fmul_rn(u, u), __fsub_rn(3.0f, __fmul_rn(2.0f, u))));
}
__device__ __forceinline__ float mblur_near(float a, float b, float extent)
{
    const float e = __fmul_rn(extent, fmaxf(fminf(a, b), 1e-6f));
    return mblur_clamp01(__fsub_rn(1.0f, __fsub_rn(a, b) / e));
}
__device__ __forceinline__ float mblur_depth(float z) { return (mblur_finite(z) && z < RT_MBLUR_FAR) ? z : RT_MBLUR_FAR; }

// steps 5 and 6
__global__ __launch_bounds__(RT_MBLUR_BLOCK) void k_mblur_gather(MblurArgs A)
{
    const int gx = (int)(blockIdx.x % (uint32_t)A.groups_x), gy = (int)(blockIdx.x / (uint32_t)A.groups_x);
    for (int l = (int)threadIdx.x; l < A.side * A.side; l += RT_MBLUR_BLOCK) {
        const int ly = l / A.side, lx = l - ly * A.side;
        const int x = gx * A.side + lx, y = gy * A.side + ly;
        if (x >= A.width || y >= A.height) continue;
        const size_t p = (size_t)y * (size_t)A.width + (size_t)x;
        const size_t tile = (size_t)(y / A.K) * (size_t)A.tiles_x + (size_t)(x / A.K);
        const float nx = A.tile_nmax[2 * tile], ny = A.tile_nmax[2 * tile + 1];
        const float mn = mblur_m(nx, ny);
        const float cr = A.rgb[3 * p], cg = A.rgb[3 * p + 1], cb = A.rgb[3 * p + 2];
        float *o = A.out + 3 * p;
        if (mn < 0.25f || !(mblur_finite(cr) && mblur_finite(cg) && mblur_finite(cb))) { o[0] = cr; o[1] = cg; o[2] = cb; continue; }
        float cx = nx, cy = ny;                                 // clampK(vn)
        if (!(mn <= A.KK)) { const float f = A.Kf / sqrtf(mn); cx = __fmul_rn(nx, f); cy = __fmul_rn(ny, f); }
        const float L = mblur_len(mn, A.Kf);
        const Vel vp = mblur_velocity(A.motion, p, x, y, A.h);
        const float lp = fmaxf(mblur_len(vp.m, A.Kf), 0.5f);
        const float zp = mblur_depth(A.z[p]);
        const float wp = 1.0f / lp;
        float W = wp, sr = __fmul_rn(wp, cr), sg = __fmul_rn(wp, cg), sb = __fmul_rn(wp, cb);
        const int j = (0x78 >> (2 * ((y & 1) * 2 + (x & 1)))) & 3;     // {0, 2, 3, 1}
        const float jitter = 0.125f + 0.25f * (float)j;
        for (int i = 0; i < A.N; i++) {
            const float t = __fsub_rn(__fmul_rn((float)i + jitter, A.g), 1.0f);
            const float sxf = floorf(__fadd_rn(__fadd_rn((float)x, __fmul_rn(t, cx)), 0.5f));
            const float syf = floorf(__fadd_rn(__fadd_rn((float)y, __fmul_rn(t, cy)), 0.5f));
            if (!(sxf >= 0.0f && sxf < (float)A.width && syf >= 0.0f && syf < (float)A.height)) continue;     // outside: weight 0
            const int sx = (int)sxf, sy = (int)syf;
            const size_t s = (size_t)sy * (size_t)A.width + (size_t)sx;
            const float tr = A.rgb[3 * s], tg = A.rgb[3 * s + 1], tb = A.rgb[3 * s + 2];
            if (!(mblur_finite(tr) && mblur_finite(tg) && mblur_finite(tb))) continue;
            const Vel vs = mblur_velocity(A.motion, s, sx, sy, A.h);
            const float ls = fmaxf(mblur_len(vs.m, A.Kf), 0.5f);
            const float zs = mblur_depth(A.z[s]);
            const float d = __fmul_rn(fabsf(t), L);
            const float fore = __fmul_rn(mblur_near(zs, zp, A.depth_extent), mblur_cone(d, ls));
            const float back = __fmul_rn(mblur_near(zp, zs, A.depth_extent), mblur_cone(d, lp));
            const float both = __fmul_rn(2.0f, __fmul_rn(mblur_cyl(d, ls), mblur_cyl(d, lp)));
            const float w = __fadd_rn(__fadd_rn(fore, back), both);
            W = __fadd_rn(W, w);
            sr = __fadd_rn(sr, __fmul_rn(w, tr)); sg = __fadd_rn(sg, __fmul_rn(w, tg)); sb = __fadd_rn(sb, __fmul_rn(w, tb));
        }
        o[0] = sr / W; o[1] = sg / W; o[2] = sb / W;
    }
}

hipError_t rtk_launch_motion_blur(hipStream_t st, const MotionBlurRequest &R)
{
    MblurArgs A = {};
    A.width = R.width; A.height = R.height; A.K = R.K; A.N = R.N;
    A.tiles_x = R.tiles_x; A.tiles_y = R.tiles_y;
    const int G = RT_MBLUR_GROUP / R.K > 1 ? RT_MBLUR_GROUP / R.K : 1;
    A.side = G * R.K;                                           // at most 32: K <= 32, and G K <= 16 when G > 1
    A.groups_x = (R.width + A.side - 1) / A.side;
    const int groups_y = (R.height + A.side - 1) / A.side;
    A.h = R.half_shutter; A.g = R.two_over_n; A.depth_extent = R.depth_extent; A.Kf = (float)R.K; A.KK = (float)(R.K * R.K);
    A.rgb = R.rgb_linear; A.motion = R.motion; A.z = R.z; A.out = R.out; A.out_tiles = R.out_tiles;
    A.tile_max = R.tile_max; A.tile_nmax = R.tile_nmax;
    const size_t tiles = (size_t)R.tiles_x * (size_t)R.tiles_y;                        // <= 2^28 (2^30 pixels, K >= 2)
    const size_t per_block = RT_MBLUR_BLOCK / 64;
    hipLaunchKernelGGL(k_mblur_tile_max, dim3((uint32_t)((tiles + per_block - 1) / per_block)), dim3(RT_MBLUR_BLOCK), 0, st, A);
    hipLaunchKernelGGL(k_mblur_neighbour_max, dim3((uint32_t)((tiles + RT_MBLUR_BLOCK - 1) / RT_MBLUR_BLOCK)), dim3(RT_MBLUR_BLOCK), 0, st, A);
    hipLaunchKernelGGL(k_mblur_gather, dim3((uint32_t)((size_t)A.groups_x * (size_t)groups_y)), dim3(RT_MBLUR_BLOCK), 0, st, A);
    return hipGetLastError();
}
