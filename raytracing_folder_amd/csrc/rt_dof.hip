// rt_dof.hip -- depth of field: the image-space stage between the denoise / temporal accumulation and motion blur.  The definition the
// kernels follow step by step is in include/rt_mi355x.h ("depth of field"); the reference has no counterpart.  A tile-gather stage:
// the tiles, the three walks and the launch are rt_tile_gather.h's.  Its own:
//
//   k_dof_coc             per pixel 4 bytes of z; the lanes compute the signed circle of confusion c and the axial depth D once and
//                         store them as a float2 in the rt_dof's plane -- a tap of the gather then reads 20 bytes (c, D, colour)
//                         instead of taking a square root and two divisions again -- and reduce the tile's largest r = min(|c|, K).
//                         A float max is associative, so the result does not depend on how the pixels were dealt to the lanes
//   k_dof_neighbour_max   the largest tile max of the 3 x 3 tiles, R
//   k_dof_gather          a frame in focus costs 12 bytes in and 12 out per pixel here, and a wave in flight takes the N taps
//                         together.  The tap table comes in the kernel argument (512 bytes, read by scalar loads: the tap index is
//                         uniform); the quarter turn per pixel is two selects
#include "rt_launch.h"
#include "rt_tile_gather.h"

// the kernels' argument: the grid, (float)K and (float)N, the request as the host made it (its taps: a host pointer, not read here) and
// step 5's table, N of them; members, order and types are its layout
struct DofArgs { TileGrid grid; float Kf, Nf; DofRequest R; float2 taps[RT_DOF_MAX_TAPS]; };

// step 1: (c, D) of the pixel (x, y) with depth z
__device__ __forceinline__ float2 dof_coc(const DofArgs &A, int x, int y, float z)
{
    if (!(stage_finite(z) && z > 0.0f && z < RT_STAGE_FAR)) return make_float2(A.R.A, RT_STAGE_FAR);
    const float sx = __fadd_rn(A.R.bx, __fmul_rn(__fadd_rn((float)x, 0.5f), A.R.u));
    const float sy = __fadd_rn(A.R.by, __fmul_rn(__fadd_rn((float)y, 0.5f), A.R.v));
    const float n2 = __fadd_rn(__fadd_rn(__fmul_rn(sx, sx), __fmul_rn(sy, sy)), __fmul_rn(A.R.l, A.R.l));
    const float cs = A.R.l / sqrtf(n2);
    const float D = fmaxf(__fmul_rn(z, cs), 1e-6f);
    return make_float2(__fmul_rn(A.R.A, __fsub_rn(1.0f, A.R.focus / D)), D);
}

// steps 1 and 2
__global__ __launch_bounds__(RT_TILE_BLOCK) void k_dof_coc(DofArgs A)
{
    float best = 0.0f;                                          // every r is at least 0
    uint32_t tile;
    if (!tile_wave_pixels(A.grid, tile, [&](size_t p, int x, int y) {
            const float2 cd = dof_coc(A, x, y, A.R.z[p]);
            A.R.coc[p] = cd;
            if (A.R.out_coc) A.R.out_coc[p] = cd.x;
            best = fmaxf(best, fminf(fabsf(cd.x), A.Kf));
        })) return;                                             // the whole wave
    for (int off = 32; off > 0; off >>= 1) best = fmaxf(best, __shfl_xor(best, off));
    if ((threadIdx.x & 63u) == 0) A.R.tile_max[tile] = best;
}

// step 3
__global__ __launch_bounds__(RT_TILE_BLOCK) void k_dof_neighbour_max(DofArgs A)
{
    float best = 0.0f;
    uint32_t tile;
    if (!tile_neighbours(A.grid, tile, [&](size_t t) { best = fmaxf(best, A.R.tile_max[t]); })) return;
    A.R.tile_nmax[tile] = best;
    if (A.R.out_tiles) A.R.out_tiles[tile] = best;
}

// steps 4 and 5
__global__ __launch_bounds__(RT_TILE_BLOCK) void k_dof_gather(DofArgs A)
{
    tile_gather_pixels(A.grid, [&](size_t p, int x, int y, size_t tile) {
        const float R = A.R.tile_nmax[tile];
        const float cr = A.R.rgb_linear[3 * p], cg = A.R.rgb_linear[3 * p + 1], cb = A.R.rgb_linear[3 * p + 2];
        float *o = A.R.out + 3 * p;
        if (R < 0.5f || !(stage_finite(cr) && stage_finite(cg) && stage_finite(cb))) { o[0] = cr; o[1] = cg; o[2] = cb; return; }
        const float2 cdp = A.R.coc[p];
        const float rp = fminf(fabsf(cdp.x), A.Kf), Dp = cdp.y;
        const float q = fmaxf(rp, 0.5f);
        const float wp = 1.0f / __fmul_rn(q, q);
        float W = wp, sr = __fmul_rn(wp, cr), sg = __fmul_rn(wp, cg), sb = __fmul_rn(wp, cb);
        const float area = __fmul_rn(R, R) / A.Nf;
        const int j = stage_pixel_quarter(x, y);
        const float fx = (float)x, fy = (float)y;
        bool any = false;
        for (int i = 0; i < A.R.N; i++) {
            const float2 t = A.taps[i];                         // uniform: a scalar load
            const float ax = (j & 1) ? t.y : t.x, ay = (j & 1) ? t.x : t.y;       // the quarter turns: swaps and negations
            const float ox = (j == 1 || j == 2) ? -ax : ax, oy = (j >= 2) ? -ay : ay;
            const float sxf = floorf(__fadd_rn(__fadd_rn(fx, __fmul_rn(R, ox)), 0.5f));
            const float syf = floorf(__fadd_rn(__fadd_rn(fy, __fmul_rn(R, oy)), 0.5f));
            const TileTap tap = tile_tap(A.grid, sxf, syf);
            if (!tap.inside || (tap.sx == x && tap.sy == y)) continue;      // outside, or p itself: the centre term has it
            const size_t s = tap.s;
            const float tr = A.R.rgb_linear[3 * s], tg = A.R.rgb_linear[3 * s + 1], tb = A.R.rgb_linear[3 * s + 2];
            if (!(stage_finite(tr) && stage_finite(tg) && stage_finite(tb))) continue;
            const float2 cds = A.R.coc[s];
            const float rs = fminf(fabsf(cds.x), A.Kf), Ds = cds.y;
            const float dx = __fsub_rn(sxf, fx), dy = __fsub_rn(syf, fy);
            const float d = sqrtf(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)));
            const float e = __fmul_rn(A.R.depth_extent, fmaxf(fminf(Ds, Dp), 1e-6f));
            const float behind = stage_clamp01(__fsub_rn(Ds, Dp) / e);
            const float re = fmaxf(__fadd_rn(rs, __fmul_rn(behind, __fsub_rn(fminf(rs, rp), rs))), 0.5f);
            const float cov = stage_clamp01(__fadd_rn(__fsub_rn(re, d), 0.5f));
            if (!(cov > 0.0f)) continue;                        // weight 0: adds nothing to any sum
            any = true;
            const float w = __fmul_rn(area, cov) / __fmul_rn(re, re);
            W = __fadd_rn(W, w);
            sr = __fadd_rn(sr, __fmul_rn(w, tr)); sg = __fadd_rn(sg, __fmul_rn(w, tg)); sb = __fadd_rn(sb, __fmul_rn(w, tb));
        }
        if (any) { o[0] = sr / W; o[1] = sg / W; o[2] = sb / W; }
        else { o[0] = cr; o[1] = cg; o[2] = cb; }
    });
}

hipError_t rtk_launch_dof(hipStream_t st, const DofRequest &R)
{
    DofArgs A = {tile_grid(R.width, R.height, R.K, R.tiles_x, R.tiles_y), (float)R.K, (float)R.N, R, {}};
    for (int i = 0; i < R.N && i < RT_DOF_MAX_TAPS; i++) A.taps[i] = make_float2(R.taps[2 * i], R.taps[2 * i + 1]);
    return tile_gather_launch(st, A.grid, k_dof_coc, k_dof_neighbour_max, k_dof_gather, A);
}
