// rt_resolve.hip -- the kernels of the render path that never see a ray (gfx950 / CDNA4, wave64), with their launches:
//
//   k_resolve       K6  per-pixel average / variance gate / gamma / Color24 pack (rtk_launch_resolve)
//   k_fold_fx           reproducible mode: the secondary plane folded into sample_rgb (rtk_launch_fold_fx)
//   k_unpack_tiles, k_unpack_planes  an all-gathered frame un-interleaved into image planes (rtk_launch_unpack_*)
//
// Includes rt_trace.h for what k_resolve takes from it (pixel_of, the background map's texture lookup) and, through it,
// rt_launch.h and rt_kernel_util.h; nothing of the shading layer (rt_shade.h).
#include <hip/hip_runtime.h>
#include <math.h>
#include <assert.h>
#include <algorithm>
#include "rt_trace.h"

// ------------------------------------------------------------------------------------------------
// K6: per pixel, the tail of RenderPixel (FIN/main.cpp:273-338): hits-only average
// (averageColor :191-199), VariantOverThreshold (:164-189) gate for the second batch, gamma
// (powf(c, 1.0/gamma) :318-320), Color24 pack (cyColor.h:245-246), z of the last hit sample,
// sample-count byte (:312-315), background for all-miss pixels (:326-337).
//   phase 0: after the first batch (samples 0..min-1): either finalise or list the pixel
//   phase 1: after the second batch: finalise listed pixels with all samples
// ------------------------------------------------------------------------------------------------
// (ResolveArgs: rt_launch.h; float_to_byte: rt_kernel_util.h)

#ifndef RT_RESOLVE_TILE
#define RT_RESOLVE_TILE 8            // samples per pixel staged through LDS at a time
#endif
// LIN: also the linear plane (ResolveArgs::rgb_linear), or 24-byte packed records; the default instantiation is the kernel
// as it was
// VAR: also the variance plane (ResolveArgs::variance): the two double sums of its definition ride in the averaging pass
template <bool LIN = false, bool VAR = false>
__global__ __launch_bounds__(256) void k_resolve(DevWork W, ResolveArgs A)
{
    // A pixel's samples are contiguous (max_sample slots of 12 B), so a thread walking its own pixel reads 12 B
    // at a 768-B stride from its neighbours: measured 6.6x the useful bytes from HBM.  In phase 0 the 64 pixels of
    // a wave are consecutive, so the wave stages RT_RESOLVE_TILE samples of each of them through LDS with
    // coalesced reads (one 96-B run per pixel) and every lane then reads its own pixel's samples from LDS
    // (row stride 25 words: conflict-free).  The sums are taken in sample order, as before.
    __shared__ float s_tile[4][64 * (3 * RT_RESOLVE_TILE + 1)];
    float *tile = s_tile[threadIdx.x >> 6];
    const int lane = threadIdx.x & 63;
    const uint32_t npix = A.phase == 1 ? W.counts[CNT_PIXLIST] : A.npix;
    const uint32_t npix_round = (npix + 63u) & ~63u;            // whole waves take part in the staging
    if (blockIdx.x == 0 && threadIdx.x == 0 && W.stats) {
        // the queues of this pass are final by now (same stream): remember how full they got, so that the host
        // can size them from what a scene really produces instead of the 2^bounce worst case
        uint32_t pr = 0;
        for (int l = 1; l < CNT_PHOTONQ; l++) pr = max(pr, W.counts[l]);
        atomicMax(&W.stats[ST_AT(ST_PEAK_RAYS)], (unsigned long long)pr);
        // both query queues are sized from this one figure (the caustic queue gets the photon queue's capacity)
        atomicMax(&W.stats[ST_AT(ST_PEAK_QUERIES)], (unsigned long long)max(W.counts[CNT_PHOTONQ], W.counts[CNT_CAUSTICQ]));
    }
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < npix_round; i += gridDim.x * blockDim.x) {
        const uint32_t i0 = i - (uint32_t)lane;                  // first pixel of this wave
        const bool staged = A.phase == 0 && i0 + 64u <= npix;    // wave-uniform
        const bool in_range = i < npix;
        const uint32_t ql = in_range ? (A.phase == 1 ? W.pixel_list[i] : i) : 0u;
        int x = 0, y = 0;
        const bool valid = in_range && pixel_of(A.tiles, A.cam, A.q0 + ql, x, y);
        // packed mode: slots of a ragged tile that lie outside the image are part of the exchanged buffer -> zero
        if (A.packed && in_range && !valid && A.phase == 0) {
            if constexpr (LIN) {
                uint2 *rec = A.packed + 3 * ((size_t)A.q0 + ql);
                rec[0] = make_uint2(0u, 0u); rec[1] = make_uint2(0u, 0u); rec[2] = make_uint2(0u, 0u);
            } else {
                A.packed[(size_t)A.q0 + ql] = make_uint2(0u, 0u);
            }
        }
        if (!staged && !valid) continue;
        const size_t index = (size_t)y * A.cam.width + x;
        const float *rgb = W.sample_rgb + 3 * (size_t)ql * A.max_sample;
        const uint8_t *hitf = W.sample_hit + (size_t)ql * A.max_sample;
        const float *zs = W.sample_z + (size_t)ql * A.max_sample;
        const int ns = A.phase == 1 ? A.max_sample : A.min_sample;
        // the hit flags of the pixel's samples (bytes 0 / 1), 64 samples at a time: with rows of a multiple of 16 bytes they are read as
        // 16-byte words and packed into a 64-bit mask (four loads instead of one byte load per sample and pass)
        const bool packed_hits = (A.max_sample & 15) == 0;
        const int nblk = (ns + 63) >> 6;
        auto block_mask = [&](int b) -> unsigned long long {                  // samples [64 b, 64 b + 64) of this pixel, clipped to ns
            const int base = 64 * b, cnt = min(64, ns - base);
            unsigned long long m = 0;
            if (packed_hits) {
                const uint4 *h4 = (const uint4 *)(hitf + base);
                for (int t = 0; 16 * t < cnt; t++) {
                    const uint4 w = h4[t];
                    const uint32_t b16 = (((w.x & 0x01010101u) * 0x01020408u) >> 24) | ((((w.y & 0x01010101u) * 0x01020408u) >> 24) << 4) |
                                         ((((w.z & 0x01010101u) * 0x01020408u) >> 24) << 8) | ((((w.w & 0x01010101u) * 0x01020408u) >> 24) << 12);
                    m |= (unsigned long long)(b16 & 0xFFFFu) << (16 * t);
                }
            } else {
                for (int j = 0; j < cnt; j++) if (hitf[base + j]) m |= 1ull << j;
            }
            if (cnt < 64) m &= (1ull << cnt) - 1ull;
            return m;
        };
        int n = 0, last = -1;
        for (int b = 0; b < nblk; b++) { const unsigned long long m = block_mask(b); n += __popcll(m); if (m) last = 64 * b + 63 - __clzll((long long)m); }
        float hitz = 0;
        if (last >= 0) hitz = zs[last];
        // visit(r, g, b) for the hit samples in order, from LDS tiles (staged) or straight from memory
        auto for_hit_samples = [&](auto &&visit) {
            const float *wave_rgb = W.sample_rgb + 3 * (size_t)i0 * A.max_sample;
            for (int b = 0; b < nblk; b++) {
                const unsigned long long hm = block_mask(b);
                const int base = 64 * b, cnt = min(64, ns - base);
                if (staged) {
                    for (int t0 = 0; t0 < cnt; t0 += RT_RESOLVE_TILE) {
                        const int tn = min(RT_RESOLVE_TILE, cnt - t0);             // samples in this tile
                        const int run = 3 * tn;                                     // floats per pixel
                        __builtin_amdgcn_wave_barrier();
                        for (int k = lane; k < 64 * run; k += 64) {
                            const int pix = k / run, off = k - pix * run;
                            tile[pix * (3 * RT_RESOLVE_TILE + 1) + off] = wave_rgb[(size_t)pix * 3 * A.max_sample + 3 * (base + t0) + off];
                        }
                        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                        __builtin_amdgcn_wave_barrier();
                        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                        const float *mine = tile + lane * (3 * RT_RESOLVE_TILE + 1);
                        for (int j = 0; j < tn; j++) if ((hm >> (t0 + j)) & 1ull) visit(mine[3 * j], mine[3 * j + 1], mine[3 * j + 2]);
                    }
                } else {
                    for (int j = 0; j < cnt; j++) if ((hm >> j) & 1ull) visit(rgb[3 * (base + j)], rgb[3 * (base + j) + 1], rgb[3 * (base + j) + 2]);
                }
            }
        };
        bool over = false;
        if (A.phase == 0 && A.min_sample != A.max_sample && (staged || n > 0)) {
            // VariantOverThreshold over the hit colours of the first batch
            const float ninverse = (float)(1.0 / (n > 0 ? n : 1));
            float sum[3] = {0, 0, 0}, sq[3] = {0, 0, 0};
            for_hit_samples([&](float r, float g, float b) {
                const float t3[3] = {r, g, b};
                for (int c = 0; c < 3; c++) {
                    sum[c] += t3[c];
                    sq[c] = (float)((double)sq[c] + (double)t3[c] * (double)t3[c]);       // pow(float,int) -> double
                }
            });
            for (int c = 0; c < 3; c++) {
                const float avg = ninverse * sum[c];
                const float var = (float)((double)(sq[c] * ninverse) + (double)avg * (double)avg - (double)(2 * avg * ninverse * sum[c]));
                if (var > A.threshold) over = true;
            }
            over = over && n > 0 && valid;
            if (over) W.pixel_list[atomicAdd(&W.counts[CNT_PIXLIST], 1u)] = ql;
        }
        float c0 = 0, c1 = 0, c2 = 0;
        double s1[3] = {0, 0, 0}, s2[3] = {0, 0, 0};                // VAR: sum and sum of squares in sample order (float products are exact in double)
        if (staged || n > 0) {
            const float inv = 1 / (float)(n > 0 ? n : 1);
            for_hit_samples([&](float r, float g, float b) {
                c0 += r * inv; c1 += g * inv; c2 += b * inv;
                if constexpr (VAR) {
                    s1[0] += (double)r; s1[1] += (double)g; s1[2] += (double)b;
                    s2[0] += (double)r * (double)r; s2[1] += (double)g * (double)g; s2[2] += (double)b * (double)b;
                }
            });
        }
        if (!valid || over) continue;
        if constexpr (VAR) {
            // variance of the mean, max(0, s2 - s1^2 / n) / (n (n - 1)); 0 for fewer than two hit samples
            float *v = A.variance + 3 * (A.packed ? (size_t)A.q0 + ql : index);
            for (int c = 0; c < 3; c++)
                v[c] = n >= 2 ? (float)(fmax(0.0, s2[c] - s1[c] * s1[c] / (double)n) / ((double)n * (double)(n - 1))) : 0.0f;
        }
        float g[3];
        uint8_t cnt_byte = 0;
        float zval = BIGFLOAT;
        if (n > 0) {
            g[0] = powf(c0, A.inv_gamma); g[1] = powf(c1, A.inv_gamma); g[2] = powf(c2, A.inv_gamma);
            cnt_byte = (n <= A.min_sample) ? 0 : 255;
            zval = hitz;
        } else {
            // background.Sample(Point3(x/W, y/H, 0)), FIN/main.cpp:326-328
            const V3 bgc = textured_color(A.S, ld3(A.bg), A.S.bg_map, mk((float)x / A.cam.width, (float)y / A.cam.height, 0));
            g[0] = powf(bgc.x, A.inv_gamma); g[1] = powf(bgc.y, A.inv_gamma); g[2] = powf(bgc.z, A.inv_gamma);
            if constexpr (LIN) { c0 = bgc.x; c1 = bgc.y; c2 = bgc.z; }        // the linear plane holds the linear background
        }
        const uint32_t r8 = float_to_byte(g[0]), g8 = float_to_byte(g[1]), b8 = float_to_byte(g[2]);
        if (A.packed) {
            const uint32_t zb = __float_as_uint(zval);
            const uint2 v = make_uint2(r8 | (g8 << 8) | (b8 << 16) | (zb << 24), (zb >> 8) | ((uint32_t)cnt_byte << 24));
            if constexpr (LIN) {
                // three 8-byte stores: the record of a wave is one contiguous 1536-byte run
                uint2 *rec = A.packed + 3 * ((size_t)A.q0 + ql);
                rec[0] = v;
                rec[1] = make_uint2(__float_as_uint(c0), __float_as_uint(c1));
                rec[2] = make_uint2(__float_as_uint(c2), 0u);
            } else {
                A.packed[(size_t)A.q0 + ql] = v;
            }
        } else {
            A.count[index] = cnt_byte;
            A.z[index] = zval;
            A.rgb8[3 * index] = (uint8_t)r8; A.rgb8[3 * index + 1] = (uint8_t)g8; A.rgb8[3 * index + 2] = (uint8_t)b8;
            if constexpr (LIN) { A.rgb_linear[3 * index] = c0; A.rgb_linear[3 * index + 1] = c1; A.rgb_linear[3 * index + 2] = c2; }
        }
    }
}

// Reproducible mode, once per pass: sample_rgb (the primary contributions) += the secondary plane, and the plane back to zero.
// Slots the pass did not touch hold zero in the plane and are left alone.
__global__ __launch_bounds__(256) void k_fold_fx(float *sample_rgb, unsigned long long *fx, size_t n)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const long long q = (long long)fx[i];
        if (q == 0) continue;
        sample_rgb[i] += (float)((double)q * (1.0 / 4294967296.0));
        fx[i] = 0ull;
    }
}

void rtk_launch_fold_fx(hipStream_t st, float *sample_rgb, unsigned long long *fx, size_t samples)
{
    const size_t n = 3 * samples;
    const int grid = (int)std::min<size_t>((n + 255) / 256, 256 * 8);
    hipLaunchKernelGGL(k_fold_fx, dim3(grid > 0 ? grid : 1), dim3(256), 0, st, sample_rgb, fx, n);
}

// Un-interleave an all-gathered frame: rank r contributed its tiles r, r+R, r+2R, ... as `per_rank` packed tiles of
// tile_w*tile_h 8-byte pixel records (see ResolveArgs::packed); one thread per image pixel reads its record (8-byte
// loads, contiguous along a tile row) and writes the three planes of the RenderImage.  LIN: 24-byte records (three 8-byte
// loads) and the linear plane as a fourth.
template <bool LIN = false>
__global__ __launch_bounds__(256) void k_unpack_tiles(const uint2 *gathered, int world, int per_rank, int width, int height,
                                                      int tile_w, int tile_h, int tiles_x, uint8_t *rgb8, float *z, uint8_t *count,
                                                      float *rgb_linear = nullptr)
{
    const size_t n = (size_t)width * height;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int y = (int)(i / (size_t)width), x = (int)(i - (size_t)y * width);
        const int tx = x / tile_w, ty = y / tile_h;
        const int t = ty * tiles_x + tx;
        const int r = t % world, k = t / world;
        const size_t q = ((size_t)r * per_rank + k) * (size_t)(tile_w * tile_h) + (size_t)(y - ty * tile_h) * tile_w + (x - tx * tile_w);
        const uint2 v = gathered[LIN ? 3 * q : q];
        rgb8[3 * i] = (uint8_t)(v.x & 255u); rgb8[3 * i + 1] = (uint8_t)((v.x >> 8) & 255u); rgb8[3 * i + 2] = (uint8_t)((v.x >> 16) & 255u);
        z[i] = __uint_as_float((v.x >> 24) | (v.y << 8));
        count[i] = (uint8_t)(v.y >> 24);
        if constexpr (LIN) {
            const uint2 a = gathered[3 * q + 1], b = gathered[3 * q + 2];
            rgb_linear[3 * i] = __uint_as_float(a.x); rgb_linear[3 * i + 1] = __uint_as_float(a.y); rgb_linear[3 * i + 2] = __uint_as_float(b.x);
        }
    }
}

void rtk_launch_unpack_tiles(hipStream_t st, const UnpackRequest &R)
{
    const int tiles_x = (R.width + R.tile_w - 1) / R.tile_w;
    const size_t n = (size_t)R.width * R.height;
    const int grid = (int)std::min<size_t>((n + 255) / 256, 4096);
    if (R.rgb_linear)
        hipLaunchKernelGGL(k_unpack_tiles<true>, dim3(grid > 0 ? grid : 1), dim3(256), 0, st, (const uint2 *)R.gathered, R.world, R.per_rank, R.width,
                           R.height, R.tile_w, R.tile_h, tiles_x, R.rgb8, R.z, R.count, R.rgb_linear);
    else
        hipLaunchKernelGGL(k_unpack_tiles<false>, dim3(grid > 0 ? grid : 1), dim3(256), 0, st, (const uint2 *)R.gathered, R.world, R.per_rank, R.width,
                           R.height, R.tile_w, R.tile_h, tiles_x, R.rgb8, R.z, R.count, nullptr);
}

// Un-interleave an all-gathered frame in the packed planes format (rt_mi355x.h, "packed planes"): k_unpack_tiles' walk over
// the image, with the records AND every plane section of the mask moved in the same pass -- up to 68 bytes read and 68 written
// per pixel, nothing computed: HBM streaming.  A pixel's slot q (tile k of its rank, row-major inside the tile) is the same in
// every section, so one index serves all of them; a section the request has no destination for costs one uniform branch.
//   V4: one thread per FOUR pixels of an image row.  With width and tile_w multiples of 4 the four lie in one tile row, so
//       they are 4 consecutive slots: 96 (32) bytes of records, 48 of each 12-byte plane, 16 of alpha and of the ids, all
//       16-byte aligned at both ends -- dwordx4 loads and stores only, lanes side by side (a wave moves 6 KB of a 24-byte
//       record run, 3 KB of a 12-byte plane per instruction triple).  rgb8 and count leave as 3 + 1 packed dwords.
//   otherwise (any geometry, any 4-byte-aligned planes): one thread per pixel, 8-byte record loads like k_unpack_tiles and
//       dword loads for the sections.
// LIN: 24-byte records and the linear plane.
template <bool V4, bool LIN>
__global__ __launch_bounds__(256) void k_unpack_planes(UnpackPlanesRequest R, int tiles_x)
{
    constexpr int PX = V4 ? 4 : 1, RW = LIN ? 6 : 2;                // pixels per thread; 32-bit words per record
    const int tile_px = R.tile_w * R.tile_h;
    const size_t n = (size_t)R.width * R.height / PX;
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < n; g += (size_t)gridDim.x * blockDim.x) {
        const size_t i = g * PX;                                     // the thread's first pixel
        const int y = (int)(i / (size_t)R.width), x = (int)(i - (size_t)y * R.width);
        const int tx = x / R.tile_w, ty = y / R.tile_h;
        const int t = ty * tiles_x + tx;
        const int r = t % R.world, k = t / R.world;
        const size_t q = (size_t)k * tile_px + (size_t)(y - ty * R.tile_h) * R.tile_w + (x - tx * R.tile_w);
        const uint8_t *base = (const uint8_t *)R.gathered + (size_t)r * R.rank_bytes;
        if constexpr (V4) {
            uint32_t w[4 * RW];
            const uint4 *rec = (const uint4 *)(base + (size_t)(4 * RW) * q);
#pragma unroll
            for (int j = 0; j < RW; j++) { const uint4 v = rec[j]; w[4 * j] = v.x; w[4 * j + 1] = v.y; w[4 * j + 2] = v.z; w[4 * j + 3] = v.w; }
            const uint32_t c0 = w[0] & 0xFFFFFFu, c1 = w[RW] & 0xFFFFFFu, c2 = w[2 * RW] & 0xFFFFFFu, c3 = w[3 * RW] & 0xFFFFFFu;
            uint32_t *rgb = (uint32_t *)(R.rgb8 + 3 * i);
            rgb[0] = c0 | (c1 << 24); rgb[1] = (c1 >> 8) | (c2 << 16); rgb[2] = (c2 >> 16) | (c3 << 8);
            *(uint4 *)(R.z + i) = make_uint4((w[0] >> 24) | (w[1] << 8), (w[RW] >> 24) | (w[RW + 1] << 8),
                                             (w[2 * RW] >> 24) | (w[2 * RW + 1] << 8), (w[3 * RW] >> 24) | (w[3 * RW + 1] << 8));
            *(uint32_t *)(R.count + i) = (w[1] >> 24) | ((w[RW + 1] >> 24) << 8) | ((w[2 * RW + 1] >> 24) << 16) | ((w[3 * RW + 1] >> 24) << 24);
            if constexpr (LIN) {
                uint4 *lin = (uint4 *)(R.rgb_linear + 3 * i);
                lin[0] = make_uint4(w[2], w[3], w[4], w[8]);
                lin[1] = make_uint4(w[9], w[10], w[14], w[15]);
                lin[2] = make_uint4(w[16], w[20], w[21], w[22]);
            }
            auto move48 = [&](uint64_t off, float *dst) {            // four slots of a 12-byte plane
                const uint4 *src = (const uint4 *)(base + off + 12 * q);
                const uint4 a = src[0], b = src[1], c = src[2];
                uint4 *d = (uint4 *)(dst + 3 * i);
                d[0] = a; d[1] = b; d[2] = c;
            };
            if (R.normal) move48(R.off_normal, R.normal);
            if (R.albedo) move48(R.off_albedo, R.albedo);
            if (R.alpha) *(uint4 *)(R.alpha + i) = *(const uint4 *)(base + R.off_alpha + 4 * q);
            if (R.object_id) *(uint4 *)(R.object_id + i) = *(const uint4 *)(base + R.off_object_id + 4 * q);
            if (R.variance) move48(R.off_variance, R.variance);
        } else {
            const uint2 *rec = (const uint2 *)(base + (size_t)(4 * RW) * q);
            const uint2 v = rec[0];
            R.rgb8[3 * i] = (uint8_t)(v.x & 255u); R.rgb8[3 * i + 1] = (uint8_t)((v.x >> 8) & 255u); R.rgb8[3 * i + 2] = (uint8_t)((v.x >> 16) & 255u);
            R.z[i] = __uint_as_float((v.x >> 24) | (v.y << 8));
            R.count[i] = (uint8_t)(v.y >> 24);
            if constexpr (LIN) {
                const uint2 a = rec[1], b = rec[2];
                R.rgb_linear[3 * i] = __uint_as_float(a.x); R.rgb_linear[3 * i + 1] = __uint_as_float(a.y); R.rgb_linear[3 * i + 2] = __uint_as_float(b.x);
            }
            auto move12 = [&](uint64_t off, float *dst) {
                const uint32_t *src = (const uint32_t *)(base + off + 12 * q);
                const uint32_t a = src[0], b = src[1], c = src[2];
                uint32_t *d = (uint32_t *)(dst + 3 * i);
                d[0] = a; d[1] = b; d[2] = c;
            };
            if (R.normal) move12(R.off_normal, R.normal);
            if (R.albedo) move12(R.off_albedo, R.albedo);
            if (R.alpha) *(uint32_t *)(R.alpha + i) = *(const uint32_t *)(base + R.off_alpha + 4 * q);
            if (R.object_id) *(uint32_t *)(R.object_id + i) = *(const uint32_t *)(base + R.off_object_id + 4 * q);
            if (R.variance) move12(R.off_variance, R.variance);
        }
    }
}

void rtk_launch_unpack_planes(hipStream_t st, const UnpackPlanesRequest &R)
{
    const int tiles_x = (R.width + R.tile_w - 1) / R.tile_w;
    // the 4-pixel instantiation needs every 4-pixel group inside one tile row and every access 16-byte aligned: the section
    // offsets and rank_bytes are multiples of 16 once tile_w is a multiple of 4, the planes are the caller's
    auto aligned16 = [](const void *p) { return ((uintptr_t)p & 15u) == 0; };
    const bool v4 = R.width % 4 == 0 && R.tile_w % 4 == 0 && R.rank_bytes % 16 == 0 && aligned16(R.gathered) && aligned16(R.rgb8) && aligned16(R.z) &&
                    aligned16(R.count) && aligned16(R.rgb_linear) && aligned16(R.normal) && aligned16(R.albedo) && aligned16(R.alpha) &&
                    aligned16(R.object_id) && aligned16(R.variance);
    const size_t n = (size_t)R.width * R.height / (v4 ? 4 : 1);
    // a streaming copy: enough workgroups to fill 256 CUs eight deep, a grid stride beyond that
    const dim3 grid((unsigned)std::max<size_t>(1, std::min<size_t>((n + 255) / 256, 2048))), block(256);
    if (v4) {
        if (R.rgb_linear) hipLaunchKernelGGL((k_unpack_planes<true, true>), grid, block, 0, st, R, tiles_x);
        else hipLaunchKernelGGL((k_unpack_planes<true, false>), grid, block, 0, st, R, tiles_x);
    } else {
        if (R.rgb_linear) hipLaunchKernelGGL((k_unpack_planes<false, true>), grid, block, 0, st, R, tiles_x);
        else hipLaunchKernelGGL((k_unpack_planes<false, false>), grid, block, 0, st, R, tiles_x);
    }
}

void rtk_launch_resolve(hipStream_t st, const DevWork &W, const ResolveArgs &R, int max_blocks, bool linear)
{
    assert(!linear || R.rgb_linear || R.packed);     // the LIN instantiation writes the linear plane, or 24-byte records into `packed`
    ResolveArgs A = R;
    tiles_prepare(A.tiles);
    const int grid = grid_for(A.npix, 256, max_blocks);
    if (A.variance) {
        if (linear) hipLaunchKernelGGL((k_resolve<true, true>), dim3(grid), dim3(256), 0, st, W, A);
        else hipLaunchKernelGGL((k_resolve<false, true>), dim3(grid), dim3(256), 0, st, W, A);
    }
    else if (linear) hipLaunchKernelGGL(k_resolve<true>, dim3(grid), dim3(256), 0, st, W, A);
    else hipLaunchKernelGGL(k_resolve<false>, dim3(grid), dim3(256), 0, st, W, A);
}
