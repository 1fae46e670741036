// rt_tile_gather.h -- the skeleton rt_motion_blur.hip and rt_dof.hip fill in: K x K tiles (K in 2..32), a wave per tile that reduces
// it, a lane per tile over the 3 x 3 tiles around it, and a gather whose workgroups cover squares of whole tiles, so that what a pixel
// takes from its tile is uniform over a wave wherever K allows.  The walks take one callable, and the grid by value: that keeps the
// kernels' code what the loops written in place gave.  stage_* and RT_STAGE_FAR are here because only these stages use them.
// No atomics, fixed orders; contraction is off for the whole library and the arithmetic pins it with __fmul_rn / __fadd_rn on top.
// sqrtf and the divisions are the correctly rounded ones (hipcc's default, -fhip-fp32-correctly-rounded-divide-sqrt).
#ifndef RT_TILE_GATHER_H
#define RT_TILE_GATHER_H

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#define RT_TILE_BLOCK 256
#define RT_TILE_GROUP 16                    /* the side a gather workgroup's square reaches while it holds more than one tile */
#define RT_STAGE_FAR 1.0e30f                /* the z plane's "nothing hit" (BIGFLOAT); what every depth that is not finite counts as */

// the head of a stage's kernel argument
struct TileGrid {
    int width, height, K;
    int tiles_x, tiles_y;               // ceil(width / K), ceil(height / K)
    int side, groups_x;                 // the gather: the pixels along a workgroup's square, and the squares along x
};

static inline TileGrid tile_grid(int width, int height, int K, int tiles_x, int tiles_y)
{
    TileGrid g = {width, height, K, tiles_x, tiles_y, 0, 0};
    const int G = RT_TILE_GROUP / K > 1 ? RT_TILE_GROUP / K : 1;
    g.side = G * K;                                             // at most 32: K <= 32, and G K <= 16 when G > 1
    g.groups_x = (width + g.side - 1) / g.side;
    return g;
}

// on `st`: the three kernels of a stage, each with the argument A (whose grid is g)
template <class Args>
static inline hipError_t tile_gather_launch(hipStream_t st, const TileGrid &g, void (*per_tile)(Args), void (*neighbours)(Args), void (*gather)(Args), const Args &A)
{
    const size_t tiles = (size_t)g.tiles_x * (size_t)g.tiles_y;                        // <= 2^28 (2^30 pixels, K >= 2)
    const size_t per_block = RT_TILE_BLOCK / 64, groups_y = (size_t)((g.height + g.side - 1) / g.side);
    hipLaunchKernelGGL(per_tile, dim3((uint32_t)((tiles + per_block - 1) / per_block)), dim3(RT_TILE_BLOCK), 0, st, A);
    hipLaunchKernelGGL(neighbours, dim3((uint32_t)((tiles + RT_TILE_BLOCK - 1) / RT_TILE_BLOCK)), dim3(RT_TILE_BLOCK), 0, st, A);
    hipLaunchKernelGGL(gather, dim3((uint32_t)((size_t)g.groups_x * groups_y)), dim3(RT_TILE_BLOCK), 0, st, A);
    return hipGetLastError();
}

__device__ __forceinline__ bool stage_finite(float a) { return fabsf(a) < INFINITY; }         // false for a NaN
__device__ __forceinline__ float stage_clamp01(float a) { return fminf(fmaxf(a, 0.0f), 1.0f); }
// which quarter of its pattern the pixel (x, y) takes: {0, 2, 3, 1} over a 2 x 2 block of pixels
__device__ __forceinline__ int stage_pixel_quarter(int x, int y) { return (0x78 >> (2 * ((y & 1) * 2 + (x & 1)))) & 3; }

// One wave per tile: f(p, x, y) for this lane's pixels of the wave's tile, p = y * width + x, in rising pixel index -- a reduction
// that keeps the first of equals relies on that.  Leaves the wave's tile in `tile`; false for a whole wave that has none.
template <class F>
__device__ __forceinline__ bool tile_wave_pixels(const TileGrid g, uint32_t &tile, F f)
{
    const int lane = (int)(threadIdx.x & 63u);
    tile = blockIdx.x * (RT_TILE_BLOCK / 64) + (threadIdx.x >> 6);
    if (tile >= (uint32_t)g.tiles_x * (uint32_t)g.tiles_y) return false;
    const int ty = (int)(tile / (uint32_t)g.tiles_x), tx = (int)(tile - (uint32_t)ty * (uint32_t)g.tiles_x);
    const int x0 = tx * g.K, y0 = ty * g.K;
    const int tw = min(g.K, g.width - x0), th = min(g.K, g.height - y0);
    for (int k = lane; k < tw * th; k += 64) {
        const int ly = k / tw, lx = k - ly * tw;
        f((size_t)(y0 + ly) * (size_t)g.width + (size_t)(x0 + lx), x0 + lx, y0 + ly);
    }
    return true;
}

// One lane per tile: f(t) for the tiles t of the 3 x 3 around the lane's that lie inside the grid, in row-major order.  Leaves
// the lane's tile in `tile`; false for a lane that has none.
template <class F>
__device__ __forceinline__ bool tile_neighbours(const TileGrid g, uint32_t &tile, F f)
{
    tile = blockIdx.x * RT_TILE_BLOCK + threadIdx.x;
    if (tile >= (uint32_t)g.tiles_x * (uint32_t)g.tiles_y) return false;
    const int ty = (int)(tile / (uint32_t)g.tiles_x), tx = (int)(tile - (uint32_t)ty * (uint32_t)g.tiles_x);
    for (int dy = -1; dy <= 1; dy++)
        for (int dx = -1; dx <= 1; dx++) {
            const int nx = tx + dx, ny = ty + dy;
            if (nx < 0 || ny < 0 || nx >= g.tiles_x || ny >= g.tiles_y) continue;
            f((size_t)ny * (size_t)g.tiles_x + (size_t)nx);
        }
    return true;
}

// One workgroup per square of whole tiles: f(p, x, y, tile) for this lane's pixels of the square that lie inside the image
template <class F>
__device__ __forceinline__ void tile_gather_pixels(const TileGrid g, F f)
{
    const int gx = (int)(blockIdx.x % (uint32_t)g.groups_x), gy = (int)(blockIdx.x / (uint32_t)g.groups_x);
    for (int l = (int)threadIdx.x; l < g.side * g.side; l += RT_TILE_BLOCK) {
        const int ly = l / g.side, lx = l - ly * g.side;
        const int x = gx * g.side + lx, y = gy * g.side + ly;
        if (x >= g.width || y >= g.height) continue;
        f((size_t)y * (size_t)g.width + (size_t)x, x, y, (size_t)(y / g.K) * (size_t)g.tiles_x + (size_t)(x / g.K));
    }
}

// A tap at the floored coordinates (sxf, syf): whether it lies inside the image (outside: weight 0) and, if so, its pixel and index
struct TileTap { bool inside; int sx, sy; size_t s; };
__device__ __forceinline__ TileTap tile_tap(const TileGrid g, float sxf, float syf)
{
    TileTap t = {sxf >= 0.0f && sxf < (float)g.width && syf >= 0.0f && syf < (float)g.height, 0, 0, 0};
    if (t.inside) { t.sx = (int)sxf; t.sy = (int)syf; t.s = (size_t)t.sy * (size_t)g.width + (size_t)t.sx; }
    return t;
}

#endif
