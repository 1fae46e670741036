// rt_dof.hip -- depth of field: the image-space stage between the denoise / temporal accumulation and motion blur.  The definition the
// kernels follow step by step is in include/rt_mi355x.h ("depth of field"); the reference has no counterpart.  Three launches per frame,
// in the launch shape of rt_motion_blur.hip:
//
//   k_dof_coc             one wave per K x K tile: the lanes stride over the tile's pixels (4 bytes of z each), compute the signed
//                         circle of confusion c and the axial depth D once and store them as a float2 in the rt_dof's plane -- a tap
//                         of the gather then reads 20 bytes (c, D, colour) instead of taking a square root and two divisions again --
//                         and six xor-shuffles reduce the tile's largest r = min(|c|, K).  A float max is associative, so the result
//                         does not depend on how the pixels were dealt to the lanes
//   k_dof_neighbour_max   one lane per tile: the largest tile max of the 3 x 3 tiles around it, R
//   k_dof_gather          one lane per pixel.  A workgroup covers a square of whole tiles (G x G of them, G = 16 / K, one tile from
//                         K = 9 on), so R and the early out are uniform over a wave wherever K allows: a frame in focus costs 12
//                         bytes in and 12 out per pixel here, and a wave in flight takes the N taps together.  The tap table comes
//                         in the kernel argument (512 bytes, read by scalar loads: the tap index is uniform); the quarter turn per
//                         pixel is two selects.  The taps go through the caches, nothing is staged in LDS
//
// No atomics, fixed orders; contraction is off for the whole library and the arithmetic pins it with __fmul_rn / __fadd_rn on top.
// sqrtf and the divisions are the correctly rounded ones (hipcc's default, -fhip-fp32-correctly-rounded-divide-sqrt).
#include <hip/hip_runtime.h>
#include <math.h>

#include "rt_kernel_util.h"
#include "rt_launch.h"

#define RT_DOF_BLOCK 256
#define RT_DOF_GROUP 16                     /* the side a gather workgroup's square reaches while it holds more than one tile */
#define RT_DOF_FAR 1.0e30f                  /* the z plane's "nothing hit" (BIGFLOAT), and the D of every such pixel          */

// the kernels' argument: members, order and types are its layout
struct DofArgs {
    int width, height, K, N;
    int tiles_x, tiles_y;
    int side, groups_x;                 // k_dof_gather: the pixels along a workgroup's square, and the squares along x
    float A, fd, depth_extent, Kf, Nf;  // step 0's A and focus distance; (float)K, (float)N
    float bx, by, u, v, l;              // the camera quantities of step 1
    const float *rgb, *z;
    float *out, *out_coc, *out_tiles;
    float2 *coc;                        // [width * height]: (c, D)
    float *tile_max, *tile_nmax;        // [tiles_x * tiles_y]
    float2 taps[RT_DOF_MAX_TAPS];       // step 5's table, N of them
};

__device__ __forceinline__ bool dof_finite(float a) { return fabsf(a) < INFINITY; }           // false for a NaN
__device__ __forceinline__ float dof_clamp01(float a) { return fminf(fmaxf(a, 0.0f), 1.0f); }

// step 1: (c, D) of the pixel (x, y) with depth z
__device__ __forceinline__ float2 dof_coc(const DofArgs &A, int x, int y, float z)
{
    if (!(dof_finite(z) && z > 0.0f && z < RT_DOF_FAR)) return make_float2(A.A, RT_DOF_FAR);
    const float sx = __fadd_rn(A.bx, __fmul_rn(__fadd_rn((float)x, 0.5f), A.u));
    const float sy = __fadd_rn(A.by, __fmul_rn(__fadd_rn((float)y, 0.5f), A.v));
    const float n2 = __fadd_rn(__fadd_rn(__fmul_rn(sx, sx), __fmul_rn(sy, sy)), __fmul_rn(A.l, A.l));
    const float cs = A.l / sqrtf(n2);
    const float D = fmaxf(__fmul_rn(z, cs), 1e-6f);
    return make_float2(__fmul_rn(A.A, __fsub_rn(1.0f, A.fd / D)), D);
}

// steps 1 and 2
__global__ __launch_bounds__(RT_DOF_BLOCK) void k_dof_coc(DofArgs A)
{
    const int lane = (int)(threadIdx.x & 63u);
    const uint32_t tile = blockIdx.x * (RT_DOF_BLOCK / 64) + (threadIdx.x >> 6);
    if (tile >= (uint32_t)A.tiles_x * (uint32_t)A.tiles_y) return;     // the whole wave
    const int ty = (int)(tile / (uint32_t)A.tiles_x), tx = (int)(tile - (uint32_t)ty * (uint32_t)A.tiles_x);
    const int x0 = tx * A.K, y0 = ty * A.K;
    const int tw = min(A.K, A.width - x0), th = min(A.K, A.height - y0);
    float best = 0.0f;                                          // every r is at least 0
    for (int k = lane; k < tw * th; k += 64) {
        const int ly = k / tw, lx = k - ly * tw;
        const size_t p = (size_t)(y0 + ly) * (size_t)A.width + (size_t)(x0 + lx);
        const float2 cd = dof_coc(A, x0 + lx, y0 + ly, A.z[p]);
        A.coc[p] = cd;
        if (A.out_coc) A.out_coc[p] = cd.x;
        best = fmaxf(best, fminf(fabsf(cd.x), A.Kf));
    }
    for (int off = 32; off > 0; off >>= 1) best = fmaxf(best, __shfl_xor(best, off));
    if (lane == 0) A.tile_max[tile] = best;
}

// step 3
__global__ __launch_bounds__(RT_DOF_BLOCK) void k_dof_neighbour_max(DofArgs A)
{
    const uint32_t tile = blockIdx.x * RT_DOF_BLOCK + threadIdx.x;
    if (tile >= (uint32_t)A.tiles_x * (uint32_t)A.tiles_y) return;
    const int ty = (int)(tile / (uint32_t)A.tiles_x), tx = (int)(tile - (uint32_t)ty * (uint32_t)A.tiles_x);
    float best = 0.0f;
    for (int dy = -1; dy <= 1; dy++)
        for (int dx = -1; dx <= 1; dx++) {
            const int nx = tx + dx, ny = ty + dy;
            if (nx < 0 || ny < 0 || nx >= A.tiles_x || ny >= A.tiles_y) continue;
            best = fmaxf(best, A.tile_max[(size_t)ny * (size_t)A.tiles_x + (size_t)nx]);
        }
    A.tile_nmax[tile] = best;
    if (A.out_tiles) A.out_tiles[tile] = best;
}

// steps 4 and 5
__global__ __launch_bounds__(RT_DOF_BLOCK) void k_dof_gather(DofArgs A)
{
    const int gx = (int)(blockIdx.x % (uint32_t)A.groups_x), gy = (int)(blockIdx.x / (uint32_t)A.groups_x);
    for (int l = (int)threadIdx.x; l < A.side * A.side; l += RT_DOF_BLOCK) {
        const int ly = l / A.side, lx = l - ly * A.side;
        const int x = gx * A.side + lx, y = gy * A.side + ly;
        if (x >= A.width || y >= A.height) continue;
        const size_t p = (size_t)y * (size_t)A.width + (size_t)x;
        const float R = A.tile_nmax[(size_t)(y / A.K) * (size_t)A.tiles_x + (size_t)(x / A.K)];
        const float cr = A.rgb[3 * p], cg = A.rgb[3 * p + 1], cb = A.rgb[3 * p + 2];
        float *o = A.out + 3 * p;
        if (R < 0.5f || !(dof_finite(cr) && dof_finite(cg) && dof_finite(cb))) { o[0] = cr; o[1] = cg; o[2] = cb; continue; }
        const float2 cdp = A.coc[p];
        const float rp = fminf(fabsf(cdp.x), A.Kf), Dp = cdp.y;
        const float q = fmaxf(rp, 0.5f);
        const float wp = 1.0f / __fmul_rn(q, q);
        float W = wp, sr = __fmul_rn(wp, cr), sg = __fmul_rn(wp, cg), sb = __fmul_rn(wp, cb);
        const float area = __fmul_rn(R, R) / A.Nf;
        const int j = (0x78 >> (2 * ((y & 1) * 2 + (x & 1)))) & 3;     // {0, 2, 3, 1}
        const float fx = (float)x, fy = (float)y;
        bool any = false;
        for (int i = 0; i < A.N; i++) {
            const float2 t = A.taps[i];                         // uniform: a scalar load
            const float ax = (j & 1) ? t.y : t.x, ay = (j & 1) ? t.x : t.y;       // the quarter turns: swaps and negations
            const float ox = (j == 1 || j == 2) ? -ax : ax, oy = (j >= 2) ? -ay : ay;
            const float sxf = floorf(__fadd_rn(__fadd_rn(fx, __fmul_rn(R, ox)), 0.5f));
            const float syf = floorf(__fadd_rn(__fadd_rn(fy, __fmul_rn(R, oy)), 0.5f));
            if (!(sxf >= 0.0f && sxf < (float)A.width && syf >= 0.0f && syf < (float)A.height)) continue;     // outside: weight 0
            const int sx = (int)sxf, sy = (int)syf;
            if (sx == x && sy == y) continue;                   // p itself: the centre term has it
            const size_t s = (size_t)sy * (size_t)A.width + (size_t)sx;
            const float tr = A.rgb[3 * s], tg = A.rgb[3 * s + 1], tb = A.rgb[3 * s + 2];
            if (!(dof_finite(tr) && dof_finite(tg) && dof_finite(tb))) continue;
            const float2 cds = A.coc[s];
            const float rs = fminf(fabsf(cds.x), A.Kf), Ds = cds.y;
            const float dx = __fsub_rn(sxf, fx), dy = __fsub_rn(syf, fy);
            const float d = sqrtf(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)));
            const float e = __fmul_rn(A.depth_extent, fmaxf(fminf(Ds, Dp), 1e-6f));
            const float behind = dof_clamp01(__fsub_rn(Ds, Dp) / e);
            const float re = fmaxf(__fadd_rn(rs, __fmul_rn(behind, __fsub_rn(fminf(rs, rp), rs))), 0.5f);
            const float cov = dof_clamp01(__fadd_rn(__fsub_rn(re, d), 0.5f));
            if (!(cov > 0.0f)) continue;                        // weight 0: adds nothing to any sum
            any = true;
            const float w = __fmul_rn(area, cov) / __fmul_rn(re, re);
            W = __fadd_rn(W, w);
            sr = __fadd_rn(sr, __fmul_rn(w, tr)); sg = __fadd_rn(sg, __fmul_rn(w, tg)); sb = __fadd_rn(sb, __fmul_rn(w, tb));
        }
        if (any) { o[0] = sr / W; o[1] = sg / W; o[2] = sb / W; }
        else { o[0] = cr; o[1] = cg; o[2] = cb; }
    }
}

hipError_t rtk_launch_dof(hipStream_t st, const DofRequest &R)
{
    DofArgs A = {};
    A.width = R.width; A.height = R.height; A.K = R.K; A.N = R.N;
    A.tiles_x = R.tiles_x; A.tiles_y = R.tiles_y;
    const int G = RT_DOF_GROUP / R.K > 1 ? RT_DOF_GROUP / R.K : 1;
    A.side = G * R.K;                                           // at most 32: K <= 32, and G K <= 16 when G > 1
    A.groups_x = (R.width + A.side - 1) / A.side;
    const int groups_y = (R.height + A.side - 1) / A.side;
    A.A = R.A; A.fd = R.focus; A.depth_extent = R.depth_extent; A.Kf = (float)R.K; A.Nf = (float)R.N;
    A.bx = R.bx; A.by = R.by; A.u = R.u; A.v = R.v; A.l = R.l;
    A.rgb = R.rgb_linear; A.z = R.z; A.out = R.out; A.out_coc = R.out_coc; A.out_tiles = R.out_tiles;
    A.coc = R.coc; A.tile_max = R.tile_max; A.tile_nmax = R.tile_nmax;
    for (int i = 0; i < R.N && i < RT_DOF_MAX_TAPS; i++) A.taps[i] = make_float2(R.taps[2 * i], R.taps[2 * i + 1]);
    const size_t tiles = (size_t)R.tiles_x * (size_t)R.tiles_y;                        // <= 2^28 (2^30 pixels, K >= 2)
    const size_t per_block = RT_DOF_BLOCK / 64;
    hipLaunchKernelGGL(k_dof_coc, dim3((uint32_t)((tiles + per_block - 1) / per_block)), dim3(RT_DOF_BLOCK), 0, st, A);
    hipLaunchKernelGGL(k_dof_neighbour_max, dim3((uint32_t)((tiles + RT_DOF_BLOCK - 1) / RT_DOF_BLOCK)), dim3(RT_DOF_BLOCK), 0, st, A);
    hipLaunchKernelGGL(k_dof_gather, dim3((uint32_t)((size_t)A.groups_x * (size_t)groups_y)), dim3(RT_DOF_BLOCK), 0, st, A);
    return hipGetLastError();
}
