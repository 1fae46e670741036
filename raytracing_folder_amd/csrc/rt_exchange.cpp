// rt_exchange.cpp -- the multi-GPU tile exchange of the C ABI in include/rt_mi355x.h: the packed layouts and their two size
// queries, the packed render entry points (a rank's tiles straight into its all-gather contribution; they reach the renderer only
// through render_tiles, rt_render.cpp) and the unpack entry points (the gathered contributions back into image planes).
// rt_host.h is what the host files share.
#include <cstring>

#include "rt_host.h"

namespace {
// A width x height image cut into tile_w x tile_h tiles (ragged edges count), dealt round-robin.
struct TileGrid {
    int64_t total;
    TileGrid(int32_t width, int32_t height, int32_t tile_w, int32_t tile_h)
        : total((((int64_t)width + tile_w - 1) / tile_w) * (((int64_t)height + tile_h - 1) / tile_h)) {}
    // the tiles first, first + stride, ...: from 0 the largest share of `stride` ranks
    int64_t share(int32_t stride, int32_t first = 0) const { return first >= total ? 0 : (total - first + stride - 1) / stride; }
};
}   // namespace
// what both size queries require of an image and its tile range
static bool tile_range_ok(int32_t width, int32_t height, const rt_tile_range *t)
{
    return t && width > 0 && height > 0 && t->tile_w > 0 && t->tile_h > 0 && t->stride > 0 && t->first >= 0;
}

// ---- packed records: 8 bytes per tile pixel of the call's own tiles (24 with the linear plane) ----
extern "C" rt_status rt_tiles_packed_size(int32_t width, int32_t height, const rt_tile_range *t, uint64_t *bytes, int32_t *n_tiles)
{
    if (!tile_range_ok(width, height, t)) return fail(RT_ERR_ARG, "rt_tiles_packed_size: bad argument");
    const int64_t n = TileGrid(width, height, t->tile_w, t->tile_h).share(t->stride, t->first);
    if (bytes) *bytes = (uint64_t)n * (uint64_t)t->tile_w * (uint64_t)t->tile_h * 8ull;
    if (n_tiles) *n_tiles = (int32_t)n;
    return RT_OK;
}

// ---- packed planes (rt_mi355x.h, "packed planes") ----
static const uint32_t RT_PLANE_ALL = RT_PLANE_LINEAR | RT_PLANE_NORMAL | RT_PLANE_ALBEDO | RT_PLANE_ALPHA | RT_PLANE_OBJECT_ID | RT_PLANE_VARIANCE;
// the sections behind the records, in buffer order: mask bit and plane
static const struct { uint32_t bit; Plane plane; } PACKED_SECTIONS[5] = {
    {RT_PLANE_NORMAL, PL_NORMAL}, {RT_PLANE_ALBEDO, PL_ALBEDO}, {RT_PLANE_ALPHA, PL_ALPHA}, {RT_PLANE_OBJECT_ID, PL_ID}, {RT_PLANE_VARIANCE, PL_VARIANCE}};

// one contribution of `per_rank` tiles of tile_px pixels: its bytes and the offsets of the six sections (UINT64_MAX: absent)
static uint64_t packed_planes_layout(uint64_t per_rank, uint64_t tile_px, uint32_t mask, uint64_t off[6])
{
    const uint64_t Q = per_rank * tile_px;
    uint64_t at = Q * ((mask & RT_PLANE_LINEAR) ? 24u : 8u);
    off[0] = 0;
    for (int i = 0; i < 5; i++) {
        const bool on = (mask & PACKED_SECTIONS[i].bit) != 0;
        off[1 + i] = on ? at : UINT64_MAX;
        if (on) at += Q * PLANE_BYTES[PACKED_SECTIONS[i].plane];
    }
    return (at + 15u) & ~(uint64_t)15u;
}

extern "C" rt_status rt_tiles_packed_planes_size(int32_t width, int32_t height, const rt_tile_range *t, uint32_t mask,
                                                 uint64_t *bytes, int32_t *n_tiles, uint64_t section_offsets[6])
{
    if (!bytes || !tile_range_ok(width, height, t)) return fail(RT_ERR_ARG, "rt_tiles_packed_planes_size: bad argument");
    if (mask & ~RT_PLANE_ALL) return fail(RT_ERR_ARG, "rt_tiles_packed_planes_size: unknown plane bits 0x%x", mask & ~RT_PLANE_ALL);
    const int64_t per_rank = TileGrid(width, height, t->tile_w, t->tile_h).share(t->stride);
    uint64_t off[6];
    *bytes = packed_planes_layout((uint64_t)per_rank, (uint64_t)t->tile_w * (uint64_t)t->tile_h, mask, off);
    if (n_tiles) *n_tiles = (int32_t)per_rank;
    if (section_offsets) memcpy(section_offsets, off, sizeof off);
    return RT_OK;
}

// ---- the packed render entry points ----
// What every packed entry point (the two below and the packed-planes one) checks first, and the request it ends with: 8-byte
// records into packed_dev, or 24-byte ones with the linear plane (linear).  How much of the buffer a call needs, and whether the
// rest of it is zeroed, differs between them and stays with each.
static rt_status check_packed(const char *name, const rt_scene *s, const void *packed_dev)
{
    if (!s) return fail(RT_ERR_ARG, "%s: scene is NULL", name);
    if (!packed_dev) return fail(RT_ERR_ARG, "%s: the packed buffer is required", name);
    return RT_OK;
}
static RenderRequest packed_request(void *hip_stream, int sync, rt_stats *stats_out, void *packed_dev, bool linear)
{
    RenderRequest req;
    req.stream = (hipStream_t)hip_stream; req.sync = sync != 0; req.stats_out = stats_out;
    req.packed = packed_dev; req.rec_bytes = linear ? 24 : 8;
    return req;
}

// both packed entry points: the buffer holds the records of the call's own tiles
static rt_status render_packed(const char *name, rt_scene *s, const rt_camera *cam, const rt_params *p, const rt_tile_range *tiles,
                               int device, void *hip_stream, void *packed_dev, uint64_t packed_bytes, int sync, rt_stats *stats_out,
                               bool linear)
{
    rt_status st = check_packed(name, s, packed_dev);
    if (st) return st;
    if ((st = validate_render(s, cam, p, tiles))) return st;
    uint64_t need = 0;
    if ((st = rt_tiles_packed_size(cam->width, cam->height, tiles, &need, nullptr))) return st;
    if (linear) need *= 3;
    if (packed_bytes < need) return fail(RT_ERR_ARG, "%s: buffer of %llu bytes, this call's tiles need %llu", name,
                                         (unsigned long long)packed_bytes, (unsigned long long)need);
    return render_tiles(s, cam, p, tiles, device, packed_request(hip_stream, sync, stats_out, packed_dev, linear));
}

extern "C" rt_status rt_render_tiles_packed_device(rt_scene *s, const rt_camera *cam, const rt_params *p, const rt_tile_range *tiles,
                                                   int device, void *hip_stream, void *packed_dev, uint64_t packed_bytes,
                                                   int sync, rt_stats *stats_out)
{
    return render_packed("rt_render_tiles_packed_device", s, cam, p, tiles, device, hip_stream, packed_dev, packed_bytes, sync, stats_out, false);
}

extern "C" rt_status rt_render_tiles_packed_linear_device(rt_scene *s, const rt_camera *cam, const rt_params *p, const rt_tile_range *tiles,
                                                          int device, void *hip_stream, void *packed_dev, uint64_t packed_bytes,
                                                          int sync, rt_stats *stats_out)
{
    return render_packed("rt_render_tiles_packed_linear_device", s, cam, p, tiles, device, hip_stream, packed_dev, packed_bytes, sync,
                         stats_out, true);
}

extern "C" rt_status rt_render_tiles_packed_outputs_device(rt_scene *s, const rt_camera *cam, const rt_params *p, const rt_tile_range *tiles,
                                                           int device, void *hip_stream, void *packed_dev, uint64_t packed_bytes, uint32_t mask,
                                                           int sync, rt_stats *stats_out)
{
    const char *name = "rt_render_tiles_packed_outputs_device";
    rt_status st = check_packed(name, s, packed_dev);
    if (st) return st;
    if (mask & ~RT_PLANE_ALL) return fail(RT_ERR_ARG, "%s: unknown plane bits 0x%x", name, mask & ~RT_PLANE_ALL);
    if ((st = validate_render(s, cam, p, tiles))) return st;
    uint64_t need = 0, off[6];
    if ((st = rt_tiles_packed_planes_size(cam->width, cam->height, tiles, mask, &need, nullptr, off))) return st;
    if (packed_bytes < need) return fail(RT_ERR_ARG, "%s: buffer of %llu bytes, a contribution with these planes needs %llu", name,
                                         (unsigned long long)packed_bytes, (unsigned long long)need);
    RenderRequest req = packed_request(hip_stream, sync, stats_out, packed_dev, (mask & RT_PLANE_LINEAR) != 0);
    req.packed_bytes = need;
    for (int i = 0; i < 5; i++)
        if (mask & PACKED_SECTIONS[i].bit) req.walk.p[PACKED_SECTIONS[i].plane] = (uint8_t *)packed_dev + off[1 + i];
    return render_tiles(s, cam, p, tiles, device, req);
}

// ---- the unpack entry points ----
// every unpack entry point: `world` contributions of tiles_per_rank tiles each must hold the image's tiles, dealt round-robin
static rt_status check_unpack_geometry(const char *name, int32_t world, int32_t tiles_per_rank, int32_t width, int32_t height,
                                       int32_t tile_w, int32_t tile_h)
{
    if (world <= 0 || width <= 0 || height <= 0 || tile_w <= 0 || tile_h <= 0) return fail(RT_ERR_ARG, "%s: bad geometry", name);
    const TileGrid g(width, height, tile_w, tile_h);
    if ((int64_t)tiles_per_rank * world < g.total || tiles_per_rank < g.share(world))
        return fail(RT_ERR_ARG, "%s: %d tiles per rank x %d ranks cannot hold %lld tiles", name, tiles_per_rank, world, (long long)g.total);
    return RT_OK;
}

extern "C" rt_status rt_tiles_unpack_outputs_device(int device, void *hip_stream, const void *gathered_dev, int32_t world, int32_t tiles_per_rank,
                                                    int32_t width, int32_t height, int32_t tile_w, int32_t tile_h, uint32_t mask,
                                                    const rt_outputs *device_planes, float *variance_dev)
{
    const char *name = "rt_tiles_unpack_outputs_device";
    if (!gathered_dev) return fail(RT_ERR_ARG, "%s: NULL buffer", name);
    if ((uintptr_t)gathered_dev & 15u) return fail(RT_ERR_ARG, "%s: the gathered buffer must be 16-byte aligned", name);
    if (mask & ~RT_PLANE_ALL) return fail(RT_ERR_ARG, "%s: unknown plane bits 0x%x", name, mask & ~RT_PLANE_ALL);
    rt_status st = check_outputs(name, device_planes);
    if (st) return st;
    const Planes dst(*device_planes, variance_dev);
    if ((mask & RT_PLANE_LINEAR) && !dst.p[PL_LINEAR]) return fail(RT_ERR_ARG, "%s: the linear plane is in the mask and has no destination", name);
    for (int i = 0; i < 5; i++)
        if ((mask & PACKED_SECTIONS[i].bit) && !dst.p[PACKED_SECTIONS[i].plane])
            return fail(RT_ERR_ARG, "%s: plane bit 0x%x is in the mask and has no destination", name, PACKED_SECTIONS[i].bit);
    if ((st = check_unpack_geometry(name, world, tiles_per_rank, width, height, tile_w, tile_h))) return st;
    if (!device_is_gfx950(device)) return fail(RT_ERR_NO_DEVICE, "%s: device %d is not gfx950 (no CPU path)", name, device);
    HIP_TRY(hipSetDevice(device));
    uint64_t off[6];
    UnpackPlanesRequest u = {};
    u.rank_bytes = packed_planes_layout((uint64_t)tiles_per_rank, (uint64_t)tile_w * (uint64_t)tile_h, mask, off);
    u.gathered = gathered_dev; u.world = world; u.per_rank = tiles_per_rank; u.width = width; u.height = height; u.tile_w = tile_w; u.tile_h = tile_h;
    u.rgb8 = dst.at<uint8_t>(PL_RGB8); u.z = dst.at<float>(PL_Z); u.count = dst.at<uint8_t>(PL_COUNT);
    // a destination outside the mask is not the kernel's business: it sees NULL there
    if (mask & RT_PLANE_LINEAR) u.rgb_linear = dst.at<float>(PL_LINEAR);
    if (mask & RT_PLANE_NORMAL) { u.normal = dst.at<float>(PL_NORMAL); u.off_normal = off[1]; }
    if (mask & RT_PLANE_ALBEDO) { u.albedo = dst.at<float>(PL_ALBEDO); u.off_albedo = off[2]; }
    if (mask & RT_PLANE_ALPHA) { u.alpha = dst.at<float>(PL_ALPHA); u.off_alpha = off[3]; }
    if (mask & RT_PLANE_OBJECT_ID) { u.object_id = dst.at<int32_t>(PL_ID); u.off_object_id = off[4]; }
    if (mask & RT_PLANE_VARIANCE) { u.variance = dst.at<float>(PL_VARIANCE); u.off_variance = off[5]; }
    rtk_launch_unpack_planes((hipStream_t)hip_stream, u);
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

// both record-only unpack entry points: rgb_linear_dev == NULL reads 8-byte records, otherwise 24-byte ones
static rt_status tiles_unpack(const char *name, int device, void *hip_stream, const void *gathered_dev, int32_t world, int32_t tiles_per_rank,
                              int32_t width, int32_t height, int32_t tile_w, int32_t tile_h,
                              uint8_t *rgb8_dev, float *z_dev, uint8_t *count_dev, float *rgb_linear_dev)
{
    if (!gathered_dev || !rgb8_dev || !z_dev || !count_dev) return fail(RT_ERR_ARG, "%s: NULL buffer", name);
    if (rt_status st = check_unpack_geometry(name, world, tiles_per_rank, width, height, tile_w, tile_h)) return st;
    if (!device_is_gfx950(device)) return fail(RT_ERR_NO_DEVICE, "%s: device %d is not gfx950 (no CPU path)", name, device);
    HIP_TRY(hipSetDevice(device));
    UnpackRequest u = {};
    u.gathered = gathered_dev; u.world = world; u.per_rank = tiles_per_rank; u.width = width; u.height = height; u.tile_w = tile_w; u.tile_h = tile_h;
    u.rgb8 = rgb8_dev; u.z = z_dev; u.count = count_dev; u.rgb_linear = rgb_linear_dev;
    rtk_launch_unpack_tiles((hipStream_t)hip_stream, u);
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

extern "C" rt_status rt_tiles_unpack_device(int device, void *hip_stream, const void *gathered_dev, int32_t world, int32_t tiles_per_rank,
                                            int32_t width, int32_t height, int32_t tile_w, int32_t tile_h,
                                            uint8_t *rgb8_dev, float *z_dev, uint8_t *count_dev)
{
    return tiles_unpack("rt_tiles_unpack_device", device, hip_stream, gathered_dev, world, tiles_per_rank, width, height, tile_w, tile_h,
                        rgb8_dev, z_dev, count_dev, nullptr);
}

extern "C" rt_status rt_tiles_unpack_linear_device(int device, void *hip_stream, const void *gathered_dev, int32_t world, int32_t tiles_per_rank,
                                                   int32_t width, int32_t height, int32_t tile_w, int32_t tile_h,
                                                   uint8_t *rgb8_dev, float *z_dev, uint8_t *count_dev, float *rgb_linear_dev)
{
    if (!rgb_linear_dev) return fail(RT_ERR_ARG, "rt_tiles_unpack_linear_device: the linear plane is required");
    return tiles_unpack("rt_tiles_unpack_linear_device", device, hip_stream, gathered_dev, world, tiles_per_rank, width, height, tile_w, tile_h,
                        rgb8_dev, z_dev, count_dev, rgb_linear_dev);
}
