// rt_motion_blur.hip -- motion blur: the image-space stage between the denoise and bloom.  The definition the kernels follow step
// by step is in include/rt_mi355x.h ("motion blur"); the reference has no counterpart.  A tile-gather stage: the tiles, the three
// walks and the launch are rt_tile_gather.h's.  Its own:
//
//   k_mblur_tile_max        per pixel 12 bytes of the motion plane; the lanes keep their best (m, pixel index) key.  (max m, then
//                           min index) is associative, so the result does not depend on how the pixels were dealt to the lanes
//   k_mblur_neighbour_max   the largest m of the 3 x 3 tile-max values, the first of equals
//   k_mblur_gather          a static frame costs 12 bytes in and 12 out per pixel here, and a wave in flight takes the N taps
//                           together.  A tap reads 28 bytes (motion, z, colour) of a pixel that the lanes beside it read as well
#include "rt_launch.h"
#include "rt_tile_gather.h"

// the kernels' argument: the grid, (float)K and (float)(K * K), then the request as the host made it; members, order and types are its layout
struct MblurArgs { TileGrid grid; float Kf, KK; MotionBlurRequest R; };

struct Vel { float x, y, m; };

__device__ __forceinline__ float mblur_m(float vx, float vy) { return __fadd_rn(__fmul_rn(vx, vx), __fmul_rn(vy, vy)); }

// step 1: the velocity of the pixel (x, y), p = y * width + x
__device__ __forceinline__ Vel mblur_velocity(const float *motion, size_t p, int x, int y, float h)
{
    const float *mv = motion + 3 * p;
    const float fx = mv[0], fy = mv[1], ze = mv[2];
    const bool ok = ze > 0.0f && stage_finite(fx) && stage_finite(fy) && stage_finite(ze);
    Vel v;
    v.x = ok ? __fmul_rn(h, __fsub_rn((float)x, fx)) : 0.0f;
    v.y = ok ? __fmul_rn(h, __fsub_rn((float)y, fy)) : 0.0f;
    v.m = mblur_m(v.x, v.y);
    return v;
}

// step 2
__global__ __launch_bounds__(RT_TILE_BLOCK) void k_mblur_tile_max(MblurArgs A)
{
    float bm = -1.0f, bx = 0.0f, by = 0.0f;                     // no pixel yet: below every m
    uint32_t bi = 0xffffffffu, tile;
    if (!tile_wave_pixels(A.grid, tile, [&](size_t p, int x, int y) {                  // in rising p: `>` keeps the lowest among equals
            const Vel v = mblur_velocity(A.R.motion, p, x, y, A.R.half_shutter);
            if (v.m > bm) { bm = v.m; bx = v.x; by = v.y; bi = (uint32_t)p; }
        })) return;                                             // the whole wave
    for (int off = 32; off > 0; off >>= 1) {
        const float om = __shfl_xor(bm, off), ox = __shfl_xor(bx, off), oy = __shfl_xor(by, off);
        const uint32_t oi = (uint32_t)__shfl_xor((int)bi, off);
        if (om > bm || (om == bm && oi < bi)) { bm = om; bx = ox; by = oy; bi = oi; }
    }
    if ((threadIdx.x & 63u) == 0) { A.R.tile_max[2 * (size_t)tile] = bx; A.R.tile_max[2 * (size_t)tile + 1] = by; }
}

// step 3
__global__ __launch_bounds__(RT_TILE_BLOCK) void k_mblur_neighbour_max(MblurArgs A)
{
    float bm = -1.0f, bx = 0.0f, by = 0.0f;
    uint32_t tile;
    if (!tile_neighbours(A.grid, tile, [&](size_t t) {
            const float vx = A.R.tile_max[2 * t], vy = A.R.tile_max[2 * t + 1];
            const float m = mblur_m(vx, vy);
            const bool up = m > bm;                             // the first of equals stays.  Selects on purpose: written as an
            bm = up ? m : bm; bx = up ? vx : bx; by = up ? vy : by;        // `if` the kernel comes out with a branch per neighbour
        })) return;
    A.R.tile_nmax[2 * (size_t)tile] = bx; A.R.tile_nmax[2 * (size_t)tile + 1] = by;
    if (A.R.out_tiles) { A.R.out_tiles[2 * (size_t)tile] = bx; A.R.out_tiles[2 * (size_t)tile + 1] = by; }
}

// steps 4 and 6: lenK, and the three weight functions
__device__ __forceinline__ float mblur_len(float m, float Kf) { return fminf(sqrtf(m), Kf); }
__device__ __forceinline__ float mblur_cone(float d, float l) { return stage_clamp01(__fsub_rn(1.0f, d / l)); }
__device__ __forceinline__ float mblur_cyl(float d, float l)
{
    const float e0 = __fmul_rn(0.95f, l), e1 = __fmul_rn(1.05f, l);
    const float u = stage_clamp01(__fsub_rn(d, e0) / __fsub_rn(e1, e0));
    return __fsub_rn(1.0f, __fmul_rn(__fmul_rn(u, u), __fsub_rn(3.0f, __fmul_rn(2.0f, u))));
}
__device__ __forceinline__ float mblur_near(float a, float b, float extent)
{
    const float e = __fmul_rn(extent, fmaxf(fminf(a, b), 1e-6f));
    return stage_clamp01(__fsub_rn(1.0f, __fsub_rn(a, b) / e));
}
__device__ __forceinline__ float mblur_depth(float z) { return (stage_finite(z) && z < RT_STAGE_FAR) ? z : RT_STAGE_FAR; }

// steps 5 and 6
__global__ __launch_bounds__(RT_TILE_BLOCK) void k_mblur_gather(MblurArgs A)
{
    tile_gather_pixels(A.grid, [&](size_t p, int x, int y, size_t tile) {
        const float nx = A.R.tile_nmax[2 * tile], ny = A.R.tile_nmax[2 * tile + 1];
        const float mn = mblur_m(nx, ny);
        const float cr = A.R.rgb_linear[3 * p], cg = A.R.rgb_linear[3 * p + 1], cb = A.R.rgb_linear[3 * p + 2];
        float *o = A.R.out + 3 * p;
        if (mn < 0.25f || !(stage_finite(cr) && stage_finite(cg) && stage_finite(cb))) { o[0] = cr; o[1] = cg; o[2] = cb; return; }
        float cx = nx, cy = ny;                                 // clampK(vn)
        if (!(mn <= A.KK)) { const float f = A.Kf / sqrtf(mn); cx = __fmul_rn(nx, f); cy = __fmul_rn(ny, f); }
        const float L = mblur_len(mn, A.Kf);
        const Vel vp = mblur_velocity(A.R.motion, p, x, y, A.R.half_shutter);
        const float lp = fmaxf(mblur_len(vp.m, A.Kf), 0.5f);
        const float zp = mblur_depth(A.R.z[p]);
        const float wp = 1.0f / lp;
        float W = wp, sr = __fmul_rn(wp, cr), sg = __fmul_rn(wp, cg), sb = __fmul_rn(wp, cb);
        const float jitter = 0.125f + 0.25f * (float)stage_pixel_quarter(x, y);
        for (int i = 0; i < A.R.N; i++) {
            const float t = __fsub_rn(__fmul_rn((float)i + jitter, A.R.two_over_n), 1.0f);
            const TileTap tap = tile_tap(A.grid, floorf(__fadd_rn(__fadd_rn((float)x, __fmul_rn(t, cx)), 0.5f)),
                                         floorf(__fadd_rn(__fadd_rn((float)y, __fmul_rn(t, cy)), 0.5f)));
            if (!tap.inside) continue;
            const size_t s = tap.s;
            const float tr = A.R.rgb_linear[3 * s], tg = A.R.rgb_linear[3 * s + 1], tb = A.R.rgb_linear[3 * s + 2];
            if (!(stage_finite(tr) && stage_finite(tg) && stage_finite(tb))) continue;
            const Vel vs = mblur_velocity(A.R.motion, s, tap.sx, tap.sy, A.R.half_shutter);
            const float ls = fmaxf(mblur_len(vs.m, A.Kf), 0.5f);
            const float zs = mblur_depth(A.R.z[s]);
            const float d = __fmul_rn(fabsf(t), L);
            const float fore = __fmul_rn(mblur_near(zs, zp, A.R.depth_extent), mblur_cone(d, ls));
            const float back = __fmul_rn(mblur_near(zp, zs, A.R.depth_extent), mblur_cone(d, lp));
            const float both = __fmul_rn(2.0f, __fmul_rn(mblur_cyl(d, ls), mblur_cyl(d, lp)));
            const float w = __fadd_rn(__fadd_rn(fore, back), both);
            W = __fadd_rn(W, w);
            sr = __fadd_rn(sr, __fmul_rn(w, tr)); sg = __fadd_rn(sg, __fmul_rn(w, tg)); sb = __fadd_rn(sb, __fmul_rn(w, tb));
        }
        o[0] = sr / W; o[1] = sg / W; o[2] = sb / W;
    });
}

hipError_t rtk_launch_motion_blur(hipStream_t st, const MotionBlurRequest &R)
{
    const MblurArgs A = {tile_grid(R.width, R.height, R.K, R.tiles_x, R.tiles_y), (float)R.K, (float)(R.K * R.K), R};
    return tile_gather_launch(st, A.grid, k_mblur_tile_max, k_mblur_neighbour_max, k_mblur_gather, A);
}
