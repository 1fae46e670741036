// rt_denoise.hip -- the image-space denoiser: an edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) on
// albedo-demodulated linear colour, guided by the first-hit planes (normal, z, object id).  The definition the kernels follow
// term by term is in include/rt_mi355x.h ("denoising"); the reference has no counterpart.
//
//   k_denoise_prepare   one lane per pixel: validity, demodulation, and the two 16-byte records every tap then reads --
//                       colour {d.r, d.g, d.b, z} into the first ping-pong buffer and the constant guide {n.x, n.y, n.z, id}
//   k_atrous<LAST>      one launch per level, one lane per pixel, 32 x 8 pixels per workgroup (the render's tile): 25 taps at
//                       step 2^level from the previous level's complete output; the LAST level remodulates and writes the
//                       caller's planes instead of a ping-pong buffer
//
// A pixel that takes no part -- invalid, or with a colour that is not finite before or after demodulation -- carries id -1 in
// its guide and its RAW colour in the colour buffers: every level copies it, the last one writes it back bit for bit, and no
// other pixel's tap accepts it (the ids differ).  Without the caller's id plane every participating pixel has id 0.
// No atomics, no LDS, fixed tap order: identical inputs give identical bytes.
//
// Variance-guided (rt_mi355x.h, "variance-guided denoising"): k_denoise_prepare_var and k_atrous_var<LAST> are the same two
// kernels with the demodulated variance of the mean u = variance / a^2 in a float4 ping-pong pair of its own ({u.r, u.g, u.b,
// unused}; the colour record's fourth lane is z).  A level's colour term is the squared colour difference per channel over
// k_sigma^2 times the 3 x 3 prefiltered variance of the CENTRE pixel (nine loads at unit step, once per lane) instead of
// sigma_color's, and the level writes u' = sum(w^2 u_q) / sum(w)^2 beside the colour.  A pixel that takes no part carries its
// RAW variance, like its raw colour.  They are kernels of their own, not instantiations of one template with the fixed-sigma
// ones: sharing the body moved the register allocation of k_atrous<LAST>, and those stay as they were.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "rt_kernel_util.h"
#include "rt_launch.h"

#define RT_DENOISE_TILE_W 32
#define RT_DENOISE_TILE_H 8
#define RT_DENOISE_NO_HIT 1.0e30f        /* the z plane's "nothing hit" (BIGFLOAT) */
#define RT_DENOISE_MIN_ALBEDO 1.0e-3f    /* below it a channel is not demodulated: mirrors and black surfaces have kd = 0 */

struct DenoiseGeom { int width, height, tiles_x; };

// the pixel of this lane: workgroup b is tile (b % tiles_x, b / tiles_x), a wave holds two rows of 32 pixels
__device__ __forceinline__ bool denoise_pixel(const DenoiseGeom &G, int &x, int &y)
{
    const int tx = (int)(blockIdx.x % (unsigned)G.tiles_x), ty = (int)(blockIdx.x / (unsigned)G.tiles_x);
    x = tx * RT_DENOISE_TILE_W + (int)(threadIdx.x % RT_DENOISE_TILE_W);
    y = ty * RT_DENOISE_TILE_H + (int)(threadIdx.x / RT_DENOISE_TILE_W);
    return x < G.width && y < G.height;
}

__device__ __forceinline__ float denoise_albedo(float a) { return a > RT_DENOISE_MIN_ALBEDO ? a : 1.0f; }
// x - x is 0 for a finite x and NaN otherwise
__device__ __forceinline__ bool finite3(float a, float b, float c) { return (a - a) + (b - b) + (c - c) == 0.0f; }

__global__ __launch_bounds__(RT_DENOISE_TILE_W * RT_DENOISE_TILE_H) void k_denoise_prepare(DenoiseGeom G, const float *rgb, const float *normal, const float *albedo,
                                                                                           const float *z, const int32_t *object_id, float4 *color, float4 *guide)
{
    int x, y;
    if (!denoise_pixel(G, x, y)) return;
    const size_t p = (size_t)y * G.width + x;
    const float r = rgb[3 * p], g = rgb[3 * p + 1], b = rgb[3 * p + 2], zp = z[p];
    const float dr = r / denoise_albedo(albedo[3 * p]), dg = g / denoise_albedo(albedo[3 * p + 1]), db = b / denoise_albedo(albedo[3 * p + 2]);
    const bool valid = object_id ? object_id[p] >= 0 : zp < RT_DENOISE_NO_HIT;
    const bool takes_part = valid && finite3(dr, dg, db);
    const int id = takes_part ? (object_id ? object_id[p] : 0) : -1;
    color[p] = takes_part ? make_float4(dr, dg, db, zp) : make_float4(r, g, b, zp);
    guide[p] = make_float4(normal[3 * p], normal[3 * p + 1], normal[3 * p + 2], __int_as_float(id));
}

// a component of the variance plane that is negative or not finite counts as 0
__device__ __forceinline__ float denoise_variance(float v) { return v > 0.0f && v < INFINITY ? v : 0.0f; }

// k_denoise_prepare, and the demodulated variance {u.r, u.g, u.b, 0} into the first buffer of the variance pair
__global__ __launch_bounds__(RT_DENOISE_TILE_W * RT_DENOISE_TILE_H) void k_denoise_prepare_var(DenoiseGeom G, const float *rgb, const float *normal, const float *albedo,
                                                                                               const float *z, const int32_t *object_id, float4 *color, float4 *guide,
                                                                                               const float *variance, float4 *var)
{
    int x, y;
    if (!denoise_pixel(G, x, y)) return;
    const size_t p = (size_t)y * G.width + x;
    const float r = rgb[3 * p], g = rgb[3 * p + 1], b = rgb[3 * p + 2], zp = z[p];
    const float ar = denoise_albedo(albedo[3 * p]), ag = denoise_albedo(albedo[3 * p + 1]), ab = denoise_albedo(albedo[3 * p + 2]);
    const float dr = r / ar, dg = g / ag, db = b / ab;
    const bool valid = object_id ? object_id[p] >= 0 : zp < RT_DENOISE_NO_HIT;
    const bool takes_part = valid && finite3(dr, dg, db);
    const int id = takes_part ? (object_id ? object_id[p] : 0) : -1;
    const float vr = variance[3 * p], vg = variance[3 * p + 1], vb = variance[3 * p + 2];
    color[p] = takes_part ? make_float4(dr, dg, db, zp) : make_float4(r, g, b, zp);
    guide[p] = make_float4(normal[3 * p], normal[3 * p + 1], normal[3 * p + 2], __int_as_float(id));
    var[p] = takes_part ? make_float4(denoise_variance(vr) / (ar * ar), denoise_variance(vg) / (ag * ag), denoise_variance(vb) / (ab * ab), 0.0f)
                        : make_float4(vr, vg, vb, 0.0f);
}

struct AtrousArgs {
    DenoiseGeom G;
    int step;
    float inv_color2, inv_normal2, sigma_depth;     // 1 / (sigma_color * 2^-level)^2, 1 / sigma_normal^2
    const float4 *src, *guide;
    float4 *dst;                                    // the other ping-pong buffer (not LAST)
    const float *albedo; float *out_linear; uint8_t *out_rgb8; float inv_gamma;     // LAST
};

template <bool LAST>
__global__ __launch_bounds__(RT_DENOISE_TILE_W * RT_DENOISE_TILE_H) void k_atrous(AtrousArgs A)
{
    int x, y;
    if (!denoise_pixel(A.G, x, y)) return;
    const size_t p = (size_t)y * A.G.width + x;
    const float4 cp = A.src[p], gp = A.guide[p];
    const int idp = __float_as_int(gp.w);
    // a colour that stopped being finite on the way (an overflowing average) passes through like a pixel that takes no part
    const bool filter = idp >= 0 && finite3(cp.x, cp.y, cp.z);
    float r = cp.x, g = cp.y, b = cp.z;
    if (filter) {
        const float h[5] = {1.0f / 16, 1.0f / 4, 3.0f / 8, 1.0f / 4, 1.0f / 16};
        float sr = 0, sg = 0, sb = 0, sw = 0;
#pragma unroll
        for (int dy = -2; dy <= 2; dy++) {
            const int qy = y + dy * A.step;
            if (qy < 0 || qy >= A.G.height) continue;
#pragma unroll
            for (int dx = -2; dx <= 2; dx++) {
                const int qx = x + dx * A.step;
                if (qx < 0 || qx >= A.G.width) continue;
                if (dx == 0 && dy == 0) {                   // the centre tap: t = 0 by definition
                    const float w = h[2] * h[2];
                    sr += w * cp.x; sg += w * cp.y; sb += w * cp.z; sw += w;
                    continue;
                }
                const size_t q = (size_t)qy * A.G.width + qx;
                const float4 gq = A.guide[q], cq = A.src[q];
                if (__float_as_int(gq.w) != idp) continue;  // another object, or a pixel that takes no part (id -1)
                const float cr = cq.x - cp.x, cg = cq.y - cp.y, cb = cq.z - cp.z;
                const float nx = gq.x - gp.x, ny = gq.y - gp.y, nz = gq.z - gp.z;
                const float zr = (cq.w - cp.w) / (A.sigma_depth * fmaxf(cq.w, cp.w));
                const float t = (cr * cr + cg * cg + cb * cb) * A.inv_color2 + (nx * nx + ny * ny + nz * nz) * A.inv_normal2 + zr * zr;
                // t is a sum of squares: NaN or +inf exactly when the weight or the tap's colour is not finite, or the weight is 0
                if (!(t < INFINITY)) continue;
                const float w = h[dx + 2] * h[dy + 2] * expf(-t);
                sr += w * cq.x; sg += w * cq.y; sb += w * cq.z; sw += w;
            }
        }
        r = sr / sw; g = sg / sw; b = sb / sw;              // sw >= 9/64: the centre tap
    }
    if constexpr (LAST) {
        if (idp >= 0) {                                     // remodulate; a pixel that took no part holds its raw colour
            r *= denoise_albedo(A.albedo[3 * p]); g *= denoise_albedo(A.albedo[3 * p + 1]); b *= denoise_albedo(A.albedo[3 * p + 2]);
        }
        A.out_linear[3 * p] = r; A.out_linear[3 * p + 1] = g; A.out_linear[3 * p + 2] = b;
        if (A.out_rgb8) {
            A.out_rgb8[3 * p] = float_to_byte(powf(r, A.inv_gamma));
            A.out_rgb8[3 * p + 1] = float_to_byte(powf(g, A.inv_gamma));
            A.out_rgb8[3 * p + 2] = float_to_byte(powf(b, A.inv_gamma));
        }
    } else {
        A.dst[p] = make_float4(r, g, b, cp.w);
    }
}

// k_atrous_var: the variance pair as src / dst; k_sigma^2; the caller's variance output (LAST, may be NULL)
struct AtrousVarArgs { const float4 *vsrc; float4 *vdst; float k_sigma2; float *out_variance; };
#define RT_DENOISE_VAR_FLOOR 1.0e-10f    /* guards 0 / 0 in the variance-guided colour term; not a tuning knob */

template <bool LAST>
__global__ __launch_bounds__(RT_DENOISE_TILE_W * RT_DENOISE_TILE_H) void k_atrous_var(AtrousArgs A, AtrousVarArgs V)
{
    int x, y;
    if (!denoise_pixel(A.G, x, y)) return;
    const size_t p = (size_t)y * A.G.width + x;
    const float4 cp = A.src[p], gp = A.guide[p], up = V.vsrc[p];
    const int idp = __float_as_int(gp.w);
    const bool filter = idp >= 0 && finite3(cp.x, cp.y, cp.z);
    float r = cp.x, g = cp.y, b = cp.z, ur = up.x, ug = up.y, ub = up.z;
    if (filter) {
        // the 3 x 3 prefilter at UNIT step, whatever the level: {1/4, 1/2, 1/4} each way; a neighbour outside the image or of another
        // id (a pixel that takes no part has id -1) is skipped, the centre is always taken
        const float g3[3] = {0.25f, 0.5f, 0.25f};
        float pr = 0, pg = 0, pb = 0, pw = 0;
#pragma unroll
        for (int dy = -1; dy <= 1; dy++) {
            const int qy = y + dy;
            if (qy < 0 || qy >= A.G.height) continue;
#pragma unroll
            for (int dx = -1; dx <= 1; dx++) {
                const int qx = x + dx;
                if (qx < 0 || qx >= A.G.width) continue;
                const float w = g3[dx + 1] * g3[dy + 1];
                if (dx == 0 && dy == 0) { pr += w * up.x; pg += w * up.y; pb += w * up.z; pw += w; continue; }
                const size_t q = (size_t)qy * A.G.width + qx;
                if (__float_as_int(A.guide[q].w) != idp) continue;
                const float4 uq = V.vsrc[q];
                pr += w * uq.x; pg += w * uq.y; pb += w * uq.z; pw += w;
            }
        }
        // 1 / (k_sigma^2 * prefiltered variance + floor) per channel: the centre's tolerance, the same for all 24 taps
        const float ir = 1.0f / (V.k_sigma2 * (pr / pw) + RT_DENOISE_VAR_FLOOR);
        const float ig = 1.0f / (V.k_sigma2 * (pg / pw) + RT_DENOISE_VAR_FLOOR);
        const float ib = 1.0f / (V.k_sigma2 * (pb / pw) + RT_DENOISE_VAR_FLOOR);
        const float h[5] = {1.0f / 16, 1.0f / 4, 3.0f / 8, 1.0f / 4, 1.0f / 16};
        float sr = 0, sg = 0, sb = 0, sw = 0, vr = 0, vg = 0, vb = 0;      // v: sum of w^2 u_q
#pragma unroll
        for (int dy = -2; dy <= 2; dy++) {
            const int qy = y + dy * A.step;
            if (qy < 0 || qy >= A.G.height) continue;
#pragma unroll
            for (int dx = -2; dx <= 2; dx++) {
                const int qx = x + dx * A.step;
                if (qx < 0 || qx >= A.G.width) continue;
                if (dx == 0 && dy == 0) {                   // the centre tap: t = 0 by definition
                    const float w = h[2] * h[2];
                    sr += w * cp.x; sg += w * cp.y; sb += w * cp.z; sw += w;
                    vr += w * w * up.x; vg += w * w * up.y; vb += w * w * up.z;
                    continue;
                }
                const size_t q = (size_t)qy * A.G.width + qx;
                const float4 gq = A.guide[q], cq = A.src[q];
                if (__float_as_int(gq.w) != idp) continue;
                const float cr = cq.x - cp.x, cg = cq.y - cp.y, cb = cq.z - cp.z;
                const float nx = gq.x - gp.x, ny = gq.y - gp.y, nz = gq.z - gp.z;
                const float zr = (cq.w - cp.w) / (A.sigma_depth * fmaxf(cq.w, cp.w));
                const float t = (cr * cr * ir + cg * cg * ig + cb * cb * ib) + (nx * nx + ny * ny + nz * nz) * A.inv_normal2 + zr * zr;
                if (!(t < INFINITY)) continue;
                const float w = h[dx + 2] * h[dy + 2] * expf(-t);
                const float4 uq = V.vsrc[q];
                const float w2 = w * w;
                sr += w * cq.x; sg += w * cq.y; sb += w * cq.z; sw += w;
                vr += w2 * uq.x; vg += w2 * uq.y; vb += w2 * uq.z;
            }
        }
        const float sw2 = sw * sw;
        r = sr / sw; g = sg / sw; b = sb / sw;              // sw >= 9/64: the centre tap
        ur = vr / sw2; ug = vg / sw2; ub = vb / sw2;
    }
    if constexpr (LAST) {
        if (idp >= 0) {                                     // remodulate; a pixel that took no part holds its raw colour and variance
            const float ar = denoise_albedo(A.albedo[3 * p]), ag = denoise_albedo(A.albedo[3 * p + 1]), ab = denoise_albedo(A.albedo[3 * p + 2]);
            r *= ar; g *= ag; b *= ab;
            ur *= ar * ar; ug *= ag * ag; ub *= ab * ab;
        }
        A.out_linear[3 * p] = r; A.out_linear[3 * p + 1] = g; A.out_linear[3 * p + 2] = b;
        if (V.out_variance) { V.out_variance[3 * p] = ur; V.out_variance[3 * p + 1] = ug; V.out_variance[3 * p + 2] = ub; }
        if (A.out_rgb8) {
            A.out_rgb8[3 * p] = float_to_byte(powf(r, A.inv_gamma));
            A.out_rgb8[3 * p + 1] = float_to_byte(powf(g, A.inv_gamma));
            A.out_rgb8[3 * p + 2] = float_to_byte(powf(b, A.inv_gamma));
        }
    } else {
        A.dst[p] = make_float4(r, g, b, cp.w);
        V.vdst[p] = make_float4(ur, ug, ub, 0.0f);
    }
}

void rtk_launch_denoise_frame(hipStream_t st, const DenoiseRequest &R)
{
    DenoiseGeom G;
    G.width = R.width; G.height = R.height; G.tiles_x = (R.width + RT_DENOISE_TILE_W - 1) / RT_DENOISE_TILE_W;
    const long long tiles = (long long)G.tiles_x * ((R.height + RT_DENOISE_TILE_H - 1) / RT_DENOISE_TILE_H);
    const dim3 grid((unsigned)tiles), block(RT_DENOISE_TILE_W * RT_DENOISE_TILE_H);
    const bool var = R.variance != nullptr;
    if (var) hipLaunchKernelGGL(k_denoise_prepare_var, grid, block, 0, st, G, R.rgb_linear, R.normal, R.albedo, R.z, R.object_id, R.color[0], R.guide, R.variance, R.var[0]);
    else hipLaunchKernelGGL(k_denoise_prepare, grid, block, 0, st, G, R.rgb_linear, R.normal, R.albedo, R.z, R.object_id, R.color[0], R.guide);
    for (int level = 0; level < R.levels; level++) {
        AtrousArgs A = {};
        A.G = G; A.step = 1 << level;
        const double sc = (double)R.sigma_color / (double)(1 << level);
        // capped at FLT_MAX: a tiny sigma must leave 0 * (1 / sigma^2) = 0 for equal colours, not 0 * inf
        A.inv_color2 = (float)std::min(1.0 / (sc * sc), 3.0e38);
        A.inv_normal2 = (float)std::min(1.0 / ((double)R.sigma_normal * (double)R.sigma_normal), 3.0e38);
        A.sigma_depth = R.sigma_depth;
        A.src = R.color[level & 1]; A.guide = R.guide; A.dst = R.color[(level + 1) & 1];
        A.albedo = R.albedo; A.out_linear = R.out_linear; A.out_rgb8 = R.out_rgb8; A.inv_gamma = R.inv_gamma;
        if (var) {
            AtrousVarArgs V;
            V.vsrc = R.var[level & 1]; V.vdst = R.var[(level + 1) & 1];
            V.k_sigma2 = (float)((double)R.k_sigma * (double)R.k_sigma); V.out_variance = R.out_variance;
            if (level == R.levels - 1) hipLaunchKernelGGL(k_atrous_var<true>, grid, block, 0, st, A, V);
            else hipLaunchKernelGGL(k_atrous_var<false>, grid, block, 0, st, A, V);
        }
        else if (level == R.levels - 1) hipLaunchKernelGGL(k_atrous<true>, grid, block, 0, st, A);
        else hipLaunchKernelGGL(k_atrous<false>, grid, block, 0, st, A);
    }
}
