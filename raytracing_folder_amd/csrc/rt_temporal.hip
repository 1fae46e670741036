// rt_temporal.hip -- temporal accumulation with camera reprojection: the frame-to-frame stage in front of the denoiser.  The
// definition the kernel follows step by step is in include/rt_mi355x.h ("temporal accumulation"); the reference has no
// counterpart.  Like the denoiser it is an image-space operation on image-sized planes and knows nothing of scenes: the scene is
// taken to be static between two frames, only the camera moves -- unless the caller hands in a motion plane (k_motion,
// rt_motion.hip), which then says where each pixel was instead of the two cameras.
//
//   k_temporal   one lane per pixel, 32 x 8 pixels per workgroup (the render's tile, as k_atrous): validity and demodulation of
//                the lane's own pixel, its world point from z and the current camera, that point's position in the STORED
//                camera's image, four bilinear taps into the previous history set, the blend, the caller's planes and the
//                lane's three records of the next history set.  k_temporal<true> reads that position and the expected depth
//                from the motion plane instead (rt_mi355x.h, "motion vectors"); everything else is the same code.
//
// The history is two ping-pong sets of three float4 planes (96 bytes a pixel in all): colour {d.r, d.g, d.b, z}, variance
// {u.r, u.g, u.b, N} and guide {n.x, n.y, n.z, id}.  A lane gathers from arbitrary pixels of the previous set while every lane
// writes its own pixel of the other one, hence two sets and no ordering between lanes.  A pixel that takes no part (invalid, or
// a colour that is not finite) stores N = 0 and id -1: no later tap accepts it.  Every pixel of a set is written by every frame,
// so in a set "id >= 0" and "N > 0" say the same, and a tap is judged by its guide record (id, normal) first, then by its
// colour record (z: the depth test); the variance record is loaded only for a tap that was accepted.  After a reset (or in the
// first frame) no tap is read at all, which is why nothing has to clear the allocation.
// k_temporal: no atomics, no LDS, fixed tap order: an identical sequence of calls gives identical bytes.
//
//   k_temporal_clip   the same pixel code with step 4b of "history rectification" between the taps and the blend: the reprojected
//                history colour is clamped into mu +- k_clip sigma of the CURRENT frame's (2r+1)^2 neighbourhood, and a pixel whose
//                history was clamped keeps at most clip_history of its length.  The neighbourhood is read from LDS: before anything
//                else the workgroup stages the (32+2r) x (8+2r) halo of its tile as one float4 {d.r, d.g, d.b, id} per pixel
//                (id -1: the pixel does not count -- outside the image, invalid, or a colour that is not finite; 0 for every
//                counting pixel when there is no id plane), row-major, halo_w = 32+2r float4 to a row, 38 x 14 x 16 B = 8512 B at
//                r = 3 (the array is sized for that).  Every lane of the workgroup stages and reaches the one barrier; the early
//                exits (outside the image, pass-through) come after it.  A lane with a history then walks its window row-major, top
//                row first, twice (sum and count; then the squared deviations from the mean) with one 16-byte LDS read a pixel.
//                The walk has no branch: a pixel of another id adds +0 through a select, which leaves the sums unchanged.  (With
//                `if (id differs) continue` the compiler split every read into a ds_read_b32 of the id, a wait, a branch and a
//                ds_read_b96 of the colour.)  As it stands `make asm` shows ds_read_b128 only: the 32 lanes of a tile row read 32
//                consecutive float4.  The inner loops are unrolled by 4, not by the compiler's 8, which keeps the kernel at 62
//                VGPRs and 8 waves a SIMD (74 and 6 otherwise).
//                Still no atomics and a fixed order: identical calls give identical bytes.  The halo is read from the caller's
//                rgb_linear, so out_linear must NOT be rgb_linear here (a neighbouring workgroup may already have written it):
//                the launch boundary's caller hands in a plane of its own in that case (rt_post.cpp).
#include <hip/hip_runtime.h>

#include "rt_kernel_util.h"
#include "rt_launch.h"
#include "rt_reproject.h"

#define RT_TEMPORAL_TILE_W 32
#define RT_TEMPORAL_TILE_H 8
#define RT_TEMPORAL_NO_HIT 1.0e30f       /* the z plane's "nothing hit" (BIGFLOAT) */
#define RT_TEMPORAL_MIN_ALBEDO 1.0e-3f   /* the denoiser's: below it a channel is not demodulated */
#define RT_TEMPORAL_MIN_WEIGHT 0.01f     /* accepted bilinear weight below which the pixel has no history */

// the kernel's argument: members, order and types are its layout
struct TemporalArgs {
    int width, height, tiles_x;
    int has_history;                    // 0: the first frame after create / reset -- `prev` is not read
    DevCamera cur, old;                 // this frame's camera and the one of the frame the history holds (camera_setup's quantities)
    float alpha, max_history, sigma_normal2, sigma_depth, inv_gamma;
    const float *rgb, *normal, *albedo, *z; const int32_t *object_id; const float *variance;
    float *out_linear, *out_variance, *out_history; uint8_t *out_rgb8;
    const float4 *prev; float4 *next;   // a set: colour[n], variance[n], guide[n], n = width * height
    const float *motion;                // k_temporal<true> only: (fx, fy, z_exp) per pixel
};

// k_temporal_clip's second argument (rt_mi355x.h, "history rectification")
struct TemporalClipArgs {
    int radius, min_count;
    float k_clip, clip_history;
    float *out_clipped;                 // optional: 0 no history, 1 kept, 2 clipped
};
#define RT_TEMPORAL_CLIP_MAX_RADIUS 3
#define RT_TEMPORAL_CLIP_TILE_MAX ((RT_TEMPORAL_TILE_W + 2 * RT_TEMPORAL_CLIP_MAX_RADIUS) * (RT_TEMPORAL_TILE_H + 2 * RT_TEMPORAL_CLIP_MAX_RADIUS))

__device__ __forceinline__ float temporal_albedo(float a) { return a > RT_TEMPORAL_MIN_ALBEDO ? a : 1.0f; }
// a component of the variance plane that is negative or not finite counts as 0
__device__ __forceinline__ float temporal_variance(float v) { return v > 0.0f && v < INFINITY ? v : 0.0f; }
// x - x is 0 for a finite x and NaN otherwise
__device__ __forceinline__ bool temporal_finite3(float a, float b, float c) { return (a - a) + (b - b) + (c - c) == 0.0f; }

// step 4b's staging: the workgroup's halo tile of the current frame, one float4 {d, id-or-minus-one} per pixel.  Every lane of the
// workgroup calls it, and it ends in the kernel's only barrier.
__device__ __forceinline__ void temporal_stage_halo(const TemporalArgs &A, int radius, int tx, int ty, float4 *tile)
{
    const int halo_w = RT_TEMPORAL_TILE_W + 2 * radius, halo_n = halo_w * (RT_TEMPORAL_TILE_H + 2 * radius);
    const int x_lo = tx * RT_TEMPORAL_TILE_W - radius, y_lo = ty * RT_TEMPORAL_TILE_H - radius;
    for (int i = (int)threadIdx.x; i < halo_n; i += RT_TEMPORAL_TILE_W * RT_TEMPORAL_TILE_H) {
        const int qx = x_lo + i % halo_w, qy = y_lo + i / halo_w;
        float4 e = make_float4(0.0f, 0.0f, 0.0f, __int_as_float(-1));
        if (qx >= 0 && qx < A.width && qy >= 0 && qy < A.height) {
            const size_t q = (size_t)qy * A.width + qx;
            const float dr = A.rgb[3 * q] / temporal_albedo(A.albedo[3 * q]), dg = A.rgb[3 * q + 1] / temporal_albedo(A.albedo[3 * q + 1]),
                        db = A.rgb[3 * q + 2] / temporal_albedo(A.albedo[3 * q + 2]);
            const int idq = A.object_id ? A.object_id[q] : (A.z[q] < RT_TEMPORAL_NO_HIT ? 0 : -1);
            if (idq >= 0 && temporal_finite3(dr, dg, db)) e = make_float4(dr, dg, db, __int_as_float(idq));
        }
        tile[i] = e;
    }
    __syncthreads();
}

// MOTION: steps 2-3 are replaced by the lane's own pixel of the motion plane.  CLIP: step 4b ("history rectification"); K and
// tile are used by that instance alone
template <bool MOTION, bool CLIP>
__device__ __forceinline__ void temporal_pixel(const TemporalArgs A, const TemporalClipArgs K, float4 *tile)
{
    const int tx = (int)(blockIdx.x % (unsigned)A.tiles_x), ty = (int)(blockIdx.x / (unsigned)A.tiles_x);
    const int x = tx * RT_TEMPORAL_TILE_W + (int)(threadIdx.x % RT_TEMPORAL_TILE_W);
    const int y = ty * RT_TEMPORAL_TILE_H + (int)(threadIdx.x / RT_TEMPORAL_TILE_W);
    if (CLIP) temporal_stage_halo(A, K.radius, tx, ty, tile);      // every lane: the early exits come after the barrier
    if (x >= A.width || y >= A.height) return;
    const size_t n = (size_t)A.width * (size_t)A.height;
    const size_t p = (size_t)y * A.width + x;
    float4 *next_color = A.next, *next_var = A.next + n, *next_guide = A.next + 2 * n;

    // 1. validity and demodulation: the lane reads its own pixel of every input plane before it writes anything
    const float r = A.rgb[3 * p], g = A.rgb[3 * p + 1], b = A.rgb[3 * p + 2], zp = A.z[p];
    const float ar = temporal_albedo(A.albedo[3 * p]), ag = temporal_albedo(A.albedo[3 * p + 1]), ab = temporal_albedo(A.albedo[3 * p + 2]);
    const float nx = A.normal[3 * p], ny = A.normal[3 * p + 1], nz = A.normal[3 * p + 2];
    const float vr = A.variance ? A.variance[3 * p] : 0.0f, vg = A.variance ? A.variance[3 * p + 1] : 0.0f, vb = A.variance ? A.variance[3 * p + 2] : 0.0f;
    const int idp = A.object_id ? A.object_id[p] : 0;
    const float dr = r / ar, dg = g / ag, db = b / ab;
    const bool valid = A.object_id ? idp >= 0 : zp < RT_TEMPORAL_NO_HIT;
    if (!(valid && temporal_finite3(dr, dg, db))) {         // passes through bit for bit, stores N = 0 and id -1
        next_color[p] = make_float4(r, g, b, zp);
        next_var[p] = make_float4(vr, vg, vb, 0.0f);
        next_guide[p] = make_float4(nx, ny, nz, __int_as_float(-1));
        A.out_linear[3 * p] = r; A.out_linear[3 * p + 1] = g; A.out_linear[3 * p + 2] = b;
        if (A.out_variance) { A.out_variance[3 * p] = vr; A.out_variance[3 * p + 1] = vg; A.out_variance[3 * p + 2] = vb; }
        if (A.out_history) A.out_history[p] = 0.0f;
        if (CLIP) { if (K.out_clipped) K.out_clipped[p] = 0.0f; }
        if (A.out_rgb8) {
            A.out_rgb8[3 * p] = float_to_byte(powf(r, A.inv_gamma));
            A.out_rgb8[3 * p + 1] = float_to_byte(powf(g, A.inv_gamma));
            A.out_rgb8[3 * p + 2] = float_to_byte(powf(b, A.inv_gamma));
        }
        return;
    }
    const float ur = temporal_variance(vr) / (ar * ar), ug = temporal_variance(vg) / (ag * ag), ub = temporal_variance(vb) / (ab * ab);

    float hr = 0, hg = 0, hb = 0, hur = 0, hug = 0, hub = 0, hn = 0, W = 0;     // sums over the accepted taps
    float n0 = 0;                       // the first accepted tap's length: the lengths are summed as differences to it
    if (A.has_history) {
        // 2.-3. the pixel's world point and its position in the stored camera's image (rt_reproject.h) -- or, with a motion
        // plane, what k_motion left for this pixel: z_exp <= 0 or a value that is not finite means "no previous position"
        Reprojected R;
        bool found;
        if (MOTION) {
            R.fx = A.motion[3 * p]; R.fy = A.motion[3 * p + 1]; R.zexp = A.motion[3 * p + 2];
            found = R.zexp > 0.0f && temporal_finite3(R.fx, R.fy, R.zexp);
        } else {
            found = reproject_pixel<false>(A.cur, A.old, x, y, zp, nullptr, R);
        }
        if (found) {
            const float fx = R.fx, fy = R.fy, zexp = R.zexp;
            // outside (-1, width) x (-1, height) every tap lies outside the image or weighs 0; this also keeps the conversion
            // to int away from huge and NaN positions
            if (fx > -1.0f && fx < (float)A.width && fy > -1.0f && fy < (float)A.height) {
                const float x0f = floorf(fx), y0f = floorf(fy);
                const int x0 = (int)x0f, y0 = (int)y0f;
                const float wx1 = fx - x0f, wy1 = fy - y0f, wx0 = 1.0f - wx1, wy0 = 1.0f - wy1;
                const float4 *prev_color = A.prev, *prev_var = A.prev + n, *prev_guide = A.prev + 2 * n;
                // 4. the taps, in the order (0,0), (1,0), (0,1), (1,1)
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const int qxk = x0 + (k & 1), qyk = y0 + (k >> 1);
                    if (qxk < 0 || qxk >= A.width || qyk < 0 || qyk >= A.height) continue;
                    const size_t q = (size_t)qyk * A.width + qxk;
                    const float4 gq = prev_guide[q];
                    const int idq = __float_as_int(gq.w);
                    if (A.object_id ? idq != idp : idq < 0) continue;      // another object, or a pixel that stored N = 0 (id -1)
                    const float ax = gq.x - nx, ay = gq.y - ny, az = gq.z - nz;
                    if (!(ax * ax + ay * ay + az * az <= A.sigma_normal2)) continue;
                    const float4 cq = prev_color[q];
                    if (!(fabsf(cq.w - zexp) <= A.sigma_depth * fmaxf(cq.w, zexp))) continue;
                    const float4 uq = prev_var[q];
                    const float w = ((k & 1) ? wx1 : wx0) * ((k >> 1) ? wy1 : wy0);
                    hr += w * cq.x; hg += w * cq.y; hb += w * cq.z;
                    hur += w * uq.x; hug += w * uq.y; hub += w * uq.z;
                    if (W == 0.0f) n0 = uq.w;               // (a first tap of weight 0 hands the role on: hn is still 0)
                    hn += w * (uq.w - n0); W += w;
                }
            }
        }
    }

    // 5. the blend
    float N = 1.0f, or_ = dr, og = dg, ob = db, our = ur, oug = ug, oub = ub;
    if (CLIP) {
        // 4b. the history colour into the box of the current frame's window: the window pixels that count are those of p's id
        // (the staged id is -1 for a pixel that does not count, p's own always matches), row-major, mean first
        float state = 0.0f;
        if (W >= RT_TEMPORAL_MIN_WEIGHT) {
            state = 1.0f;
            const int halo_w = RT_TEMPORAL_TILE_W + 2 * K.radius, side = 2 * K.radius + 1;
            const float4 *win = tile + (int)(threadIdx.x / RT_TEMPORAL_TILE_W) * halo_w + (int)(threadIdx.x % RT_TEMPORAL_TILE_W);
            float sr = 0, sg = 0, sb = 0; int m = 0;
            for (int j = 0; j < side; j++)
#pragma unroll 4
                for (int i = 0; i < side; i++) {
                    const float4 e = win[j * halo_w + i];          // one 16-byte read, no branch: a pixel that does not
                    const bool c = __float_as_int(e.w) == idp;      // count adds +0 (its staged colour is finite), which
                    sr += c ? e.x : 0.0f; sg += c ? e.y : 0.0f; sb += c ? e.z : 0.0f; m += c ? 1 : 0;   // leaves the sums as they are
                }
            if (m >= K.min_count) {
                const float fm = (float)m, mr = sr / fm, mg = sg / fm, mb = sb / fm;
                float qr = 0, qg = 0, qb = 0;
                for (int j = 0; j < side; j++)
#pragma unroll 4
                    for (int i = 0; i < side; i++) {
                        const float4 e = win[j * halo_w + i];
                        const bool c = __float_as_int(e.w) == idp;
                        const float xr = e.x - mr, xg = e.y - mg, xb = e.z - mb;
                        qr += c ? xr * xr : 0.0f; qg += c ? xg * xg : 0.0f; qb += c ? xb * xb : 0.0f;
                    }
                const float er = K.k_clip * sqrtf(qr / fm), eg = K.k_clip * sqrtf(qg / fm), eb = K.k_clip * sqrtf(qb / fm);
                // d_h = sum / W as the blend forms it; afterwards the sums hold the clamped d_h times W = 1
                const float ur_ = hr / W, ug_ = hg / W, ub_ = hb / W;
                const float cr = fminf(fmaxf(ur_, mr - er), mr + er), cg = fminf(fmaxf(ug_, mg - eg), mg + eg), cb = fminf(fmaxf(ub_, mb - eb), mb + eb);
                if (cr != ur_ || cg != ug_ || cb != ub_) {
                    state = 2.0f;
                    // the clamped colour stands for the taps' sum: hX / W below must give it back exactly, so the sums of
                    // colour, variance and length are renormalised to W = 1 (x / 1 is x)
                    hr = cr; hg = cg; hb = cb;
                    hur = hur / W; hug = hug / W; hub = hub / W;
                    n0 = fminf(n0 + hn / W, K.clip_history); hn = 0.0f;
                    W = 1.0f;
                }
            }
        }
        if (K.out_clipped) K.out_clipped[p] = state;
    }
    if (W >= RT_TEMPORAL_MIN_WEIGHT) {
        N = fminf((n0 + hn / W) + 1.0f, A.max_history);      // taps of equal length give exactly that length + 1
        const float beta = fmaxf(A.alpha, 1.0f / N), keep = 1.0f - beta;
        or_ = keep * (hr / W) + beta * dr; og = keep * (hg / W) + beta * dg; ob = keep * (hb / W) + beta * db;
        our = keep * keep * (hur / W) + beta * beta * ur; oug = keep * keep * (hug / W) + beta * beta * ug; oub = keep * keep * (hub / W) + beta * beta * ub;
    }
    next_color[p] = make_float4(or_, og, ob, zp);
    next_var[p] = make_float4(our, oug, oub, N);
    next_guide[p] = make_float4(nx, ny, nz, __int_as_float(idp));

    // 6. the caller's planes, remodulated
    const float lr = or_ * ar, lg = og * ag, lb = ob * ab;
    A.out_linear[3 * p] = lr; A.out_linear[3 * p + 1] = lg; A.out_linear[3 * p + 2] = lb;
    if (A.out_variance) { A.out_variance[3 * p] = our * (ar * ar); A.out_variance[3 * p + 1] = oug * (ag * ag); A.out_variance[3 * p + 2] = oub * (ab * ab); }
    if (A.out_history) A.out_history[p] = N;
    if (A.out_rgb8) {
        A.out_rgb8[3 * p] = float_to_byte(powf(lr, A.inv_gamma));
        A.out_rgb8[3 * p + 1] = float_to_byte(powf(lg, A.inv_gamma));
        A.out_rgb8[3 * p + 2] = float_to_byte(powf(lb, A.inv_gamma));
    }
}

template <bool MOTION>
__global__ __launch_bounds__(RT_TEMPORAL_TILE_W * RT_TEMPORAL_TILE_H) void k_temporal(TemporalArgs A)
{
    temporal_pixel<MOTION, false>(A, TemporalClipArgs{}, nullptr);
}

template <bool MOTION>
__global__ __launch_bounds__(RT_TEMPORAL_TILE_W * RT_TEMPORAL_TILE_H) void k_temporal_clip(TemporalArgs A, TemporalClipArgs K)
{
    __shared__ float4 tile[RT_TEMPORAL_CLIP_TILE_MAX];
    temporal_pixel<MOTION, true>(A, K, tile);
}

static TemporalArgs temporal_args(const TemporalRequest &R)
{
    TemporalArgs A = {};
    A.width = R.width; A.height = R.height; A.tiles_x = (R.width + RT_TEMPORAL_TILE_W - 1) / RT_TEMPORAL_TILE_W;
    A.has_history = R.has_history ? 1 : 0;
    A.cur = R.cur; A.old = R.old;
    A.alpha = R.alpha; A.max_history = (float)R.max_history;
    A.sigma_normal2 = (float)((double)R.sigma_normal * (double)R.sigma_normal);
    A.sigma_depth = R.sigma_depth; A.inv_gamma = R.inv_gamma;
    A.rgb = R.rgb_linear; A.normal = R.normal; A.albedo = R.albedo; A.z = R.z; A.object_id = R.object_id; A.variance = R.variance;
    A.out_linear = R.out_linear; A.out_variance = R.out_variance; A.out_history = R.out_history; A.out_rgb8 = R.out_rgb8;
    A.prev = R.prev; A.next = R.next;
    A.motion = R.motion;
    return A;
}

void rtk_launch_temporal(hipStream_t st, const TemporalRequest &R)
{
    const TemporalArgs A = temporal_args(R);
    const long long tiles = (long long)A.tiles_x * ((R.height + RT_TEMPORAL_TILE_H - 1) / RT_TEMPORAL_TILE_H);
    if (R.motion) hipLaunchKernelGGL(k_temporal<true>, dim3((unsigned)tiles), dim3(RT_TEMPORAL_TILE_W * RT_TEMPORAL_TILE_H), 0, st, A);
    else hipLaunchKernelGGL(k_temporal<false>, dim3((unsigned)tiles), dim3(RT_TEMPORAL_TILE_W * RT_TEMPORAL_TILE_H), 0, st, A);
}

void rtk_launch_temporal_clip(hipStream_t st, const TemporalClipRequest &R)
{
    const TemporalArgs A = temporal_args(R.frame);
    TemporalClipArgs K = {};
    K.radius = R.radius; K.min_count = R.min_count; K.k_clip = R.k_clip; K.clip_history = (float)R.clip_history;
    K.out_clipped = R.out_clipped;
    const long long tiles = (long long)A.tiles_x * ((R.frame.height + RT_TEMPORAL_TILE_H - 1) / RT_TEMPORAL_TILE_H);
    if (R.frame.motion) hipLaunchKernelGGL(k_temporal_clip<true>, dim3((unsigned)tiles), dim3(RT_TEMPORAL_TILE_W * RT_TEMPORAL_TILE_H), 0, st, A, K);
    else hipLaunchKernelGGL(k_temporal_clip<false>, dim3((unsigned)tiles), dim3(RT_TEMPORAL_TILE_W * RT_TEMPORAL_TILE_H), 0, st, A, K);
}
