// rt_launch.h -- the boundary between the host orchestration (rt_lower.cpp, rt_mesh_update.cpp, rt_photons.cpp, rt_render.cpp, rt_exchange.cpp, rt_jobs.cpp, rt_post.cpp) and the kernels (rt_kernels.hip, rt_trace.hip, rt_resolve.hip, rt_gather.hip,
// rt_photon_build.hip, rt_denoise.hip, rt_temporal.hip, rt_motion.hip, rt_motion_mesh.hip, rt_tonemap.hip, rt_bloom.hip, rt_motion_blur.hip, rt_dof.hip, rt_refit.hip): every rtk_* function, the requests they take and the
// records they exchange.  All of these files include it, so a declaration and its definition cannot drift apart.  ResolveArgs, PhotonArgs and UnpackPlanesRequest are passed to kernels
// as they stand here (members, order and types are the kernels' argument layout), MotionBlurRequest and DofRequest as a member of
// their kernels' argument; everything else is host-side only.
#ifndef RT_LAUNCH_H
#define RT_LAUNCH_H

#include <hip/hip_runtime.h>
#include "rt_dev.h"

// ---- requests ---------------------------------------------------------------------------------------------------------
// One tracing pass over a chunk's samples (run_pipeline in rt_render.cpp; k_wavefront / k_primary and what follows them):
//   mode 0: pixels q0..q0+npix of the call's tile walk, samples j0..j0+ns of each
//   mode 1: the pixels of the working set's pixel list, samples j0..j0+ns   (second batch)
//   mode 2: rays[] supplied by the caller, one sample each, q0 = index of the first   (rt_shade_rays)
struct RenderPass {
    DevCamera cam; DevTiles tiles;      // tiles as the call has them: the wrappers run tiles_prepare on their copy
    uint32_t q0, npix;
    int j0, ns, max_sample, mode;
    const float *rays;                  // mode 2, else NULL
    unsigned long long *fx;             // the secondary plane of a reproducible render (RT_RENDER_REPRODUCIBLE); NULL selects the default instantiations
};

// One k_gather launch: the queries of `q` (their number on the device in *count, at most q.cap are answered) against `pm`.
struct GatherRequest {
    DevPhotonMap pm;
    DevPhotonQueue q; const uint32_t *count;
    int k; float radius;
    uint32_t *next_batch;               // the launch's RT_GATHER_CTRS work counters, RT_CTR_STRIDE apart, zero at launch
    float *cell_rk2;                    // per density-grid cell: the k-th squared distance of the last query answered there; may be NULL
    // either the outputs of a render: w * irr * max(0, N.(-dir)) added into the query's sample slot (into fx instead, when set) ...
    float *sample_rgb; unsigned long long *stats, *fx;
    // ... or, when out_irr is set, irr[3] and dir[3] per query (rt_estimate_irradiance)
    float *out_irr, *out_dir;
};

// K6, the tail of RenderPixel per pixel of a chunk:
//   phase 0: after the first batch (samples 0..min-1): either finalise or list the pixel
//   phase 1: after the second batch: finalise listed pixels with all samples
struct ResolveArgs {
    DevCamera cam; DevTiles tiles;
    uint32_t q0, npix;
    int min_sample, max_sample;
    float threshold; float inv_gamma;
    int phase;
    float bg[3];
    DevScene S;                 // for the background map
    uint8_t *rgb8; float *z; uint8_t *count;
    // packed output (multi-GPU tile exchange): pixel q of this call's tile walk (tile-major, row-major inside
    // the tile) is ONE 8-byte record {r, g, b, z as 4 little-endian bytes, count} at packed + 8*q -- the very
    // buffer a rank contributes to the all-gather, written here coalesced instead of being re-packed afterwards
    uint2 *packed;
    int direct_mode;            // rt_shade_rays: no image, leave samples as they are
    // linear plane (k_resolve<true> only): the pre-gamma float RGB of the pixel, row-major like rgb8; in packed mode the
    // record grows to 24 bytes instead -- {the 8-byte record, linear r, g, b as f32, 4 zero bytes} at packed + 24*q
    float *rgb_linear;
    // variance plane (the VAR instantiations only): the variance of the mean per channel over the samples the colour is averaged
    // over (rt_mi355x.h, "the variance plane"), float[3] per pixel, row-major like rgb8 -- or, when `packed` is set (a strided
    // job), indexed like the packed records by the call's tile walk: 12 bytes at variance + 3 * (q0 + q)
    float *variance;
};

// the photon pass: attempts first_attempt .. first_attempt + n_attempts of the counter RNG's sequence
struct PhotonArgs {
    unsigned long long first_attempt; uint32_t n_attempts;
    uint32_t seed; int max_bounce;
    float *out;            // [n_attempts][RT_PHOTON_SLOTS][9]: pos, dir, power
    uint32_t *count;       // [n_attempts]: photons stored | diffuse hits counted << 16
    int mode;              // 0: photon map (PhotonTracing), 1: caustic map (CausticTracing)
};

// what k_trace writes per ray (rt_trace_rays)
struct TraceOut { uint8_t *hit; float *z, *p, *N; int32_t *node; uint8_t *front; };

// an all-gathered frame to un-interleave: rank r of `world` contributed its tiles r, r+world, ... as per_rank packed tiles
// (8-byte records, 24-byte ones when rgb_linear is set) -> the planes of a width x height image
struct UnpackRequest {
    const void *gathered; int world, per_rank, width, height, tile_w, tile_h;
    uint8_t *rgb8; float *z; uint8_t *count; float *rgb_linear;
};

// an all-gathered frame in the packed planes format (rt_mi355x.h, "packed planes") to un-interleave: rank r's contribution at
// gathered + r * rank_bytes; in it the records (24-byte ones when rgb_linear is set, else 8-byte ones) at 0 and the section of
// each plane whose destination is set at its offset (bytes, from the contribution's start).  Destinations that are NULL are not
// in the mask: nothing is read or written for them.
struct UnpackPlanesRequest {
    const void *gathered; uint64_t rank_bytes;
    int world, per_rank, width, height, tile_w, tile_h;
    uint8_t *rgb8; float *z; uint8_t *count; float *rgb_linear;
    float *normal, *albedo, *alpha; int32_t *object_id; float *variance;
    uint64_t off_normal, off_albedo, off_alpha, off_object_id, off_variance;
};

// One denoise of a width x height frame (rt_denoise.hip; the definition: rt_mi355x.h, "denoising").  The planes are the caller's
// device pointers (object_id and out_rgb8 may be NULL; out_linear may be rgb_linear), the sigmas are validated by the caller.
// color[0], color[1] and guide are the per-device scratch, width * height float4 each (RT_DENOISE_SCRATCH_PER_PIXEL bytes a pixel).
// Variance-guided (rt_mi355x.h, "variance-guided denoising"): `variance` is set, var[0] and var[1] are two more float4 buffers of
// the scratch (the demodulated variance's ping-pong pair: RT_DENOISE_SCRATCH_PER_PIXEL_VAR bytes a pixel in all), out_variance
// may be NULL or `variance`; sigma_color is not used then.
#define RT_DENOISE_SCRATCH_PER_PIXEL 48
#define RT_DENOISE_SCRATCH_PER_PIXEL_VAR 80
struct DenoiseRequest {
    int width, height, levels;
    float sigma_color, sigma_normal, sigma_depth, inv_gamma;
    const float *rgb_linear, *normal, *albedo, *z; const int32_t *object_id;
    float *out_linear; uint8_t *out_rgb8;
    float4 *color[2], *guide;
    const float *variance; float *out_variance; float k_sigma;
    float4 *var[2];
};

// One temporal accumulation of a width x height frame (rt_temporal.hip; the definition: rt_mi355x.h, "temporal accumulation").
// The planes are the caller's device pointers (object_id, variance, out_variance, out_history and out_rgb8 may be NULL;
// out_linear may be rgb_linear and out_variance may be variance), the parameters are validated by the caller.  `cur` and `old`
// are camera_setup's quantities of this frame's camera and of the one the history holds; has_history is false for the first
// frame after a create or a reset, and `prev` is then not read.  prev / next: the two sets of a history, each three planes of
// width * height float4 (colour, variance, guide: RT_TEMPORAL_HISTORY_PER_PIXEL bytes a pixel for both sets together).
// motion: NULL, or the device plane of a MotionRequest -- k_temporal<true> then takes each pixel's previous position and expected
// depth from it and `cur` / `old` are not used by the kernel.
#define RT_TEMPORAL_HISTORY_PER_PIXEL 96
struct TemporalRequest {
    int width, height; bool has_history;
    DevCamera cur, old;
    float alpha; int max_history; float sigma_normal, sigma_depth, inv_gamma;
    const float *rgb_linear, *normal, *albedo, *z; const int32_t *object_id; const float *variance;
    float *out_linear, *out_variance, *out_history; uint8_t *out_rgb8;
    const float4 *prev; float4 *next;
    const float *motion;
};

// One temporal accumulation with history rectification (rt_temporal.hip, k_temporal_clip; the definition: rt_mi355x.h, "history
// rectification"): `frame` is the plain accumulation's request, with one restriction -- out_linear must not overlap rgb_linear,
// because the workgroups read their neighbours' pixels of rgb_linear (the caller substitutes a plane of its own and copies).
// radius 1..3, min_count >= 1, k_clip > 0 and clip_history 1..65535 are validated by the caller; out_clipped: NULL, or the
// caller's device plane of width * height floats (0 no history, 1 kept, 2 clipped).
struct TemporalClipRequest {
    TemporalRequest frame;
    int radius, min_count; float k_clip; int clip_history;
    float *out_clipped;
};

// One motion plane of a width x height frame (rt_motion.hip; the definition: rt_mi355x.h, "motion vectors").  z, object_id and
// motion are the caller's device planes.  `cur` and `old` are camera_setup's quantities of this frame's camera and the previous
// frame's.  table: one DevNodeMotion per node on the device, this frame's world -> the previous frame's, P_prev = R P + t as three
// 16-byte rows {R_k0, R_k1, R_k2, t_k} (48 bytes a node, three dwordx4 loads); composed on the host in double.
struct DevNodeMotion { float4 row[3]; };
struct MotionRequest {
    int width, height, n_nodes;
    DevCamera cur, old;
    const float *z; const int32_t *object_id;
    const DevNodeMotion *table;
    float *motion;
};

// One motion plane of a scene whose meshes may have deformed (rt_motion_mesh.hip; the definition: rt_mi355x.h, "motion vectors for
// deforming meshes").  `rigid` is the MotionRequest of the same frame: a pixel whose node has no entry in `mesh_nodes` is k_motion's.
// mesh_nodes: one record per node on the device -- object < 0: rigid; otherwise the node's object in the lowered scene S (whose
// chain takes the ray into the mesh's coordinates), its mesh, that mesh's previous positions (nv x 3 floats, indexed like v) and
// its slots' indices (six uint32 per triangle slot, the first three into v).  from: one DevNodeMotion per node, the PREVIOUS
// chain's object-to-world map, composed on the host in double.  p13: the scene's triangle test is tri_hit_p13, else tri_hit_fin.
// spill: NULL, or RT_SPILL_BLOCKS * RT_BLOCK threads' RT_BVH_SPILL entries (required when S.max_bvh_depth > RT_BVH_STACK).
struct DevMotionMeshNode { int32_t object, mesh; const float *v_prev; const uint32_t *slot_idx; };
struct MotionMeshRequest {
    MotionRequest rigid;
    DevScene S;
    const DevMotionMeshNode *mesh_nodes;        // [rigid.n_nodes]
    const DevNodeMotion *from;                  // [rigid.n_nodes]
    float depth_tol; bool p13;
    uint32_t *spill;
};

// One tone-mapped width x height frame (rt_tonemap.hip; the definition: rt_mi355x.h, "exposure and tone mapping").  The planes are
// the caller's device pointers (object_id and one of out_display / out_rgb8 may be NULL; out_display may be rgb_linear), the
// parameters are validated by the caller.  meter: k_luminance_hist and k_exposure_meter run on `state` first and k_tonemap takes
// the scale they leave there; otherwise only k_tonemap runs, with `scale`, and `state` is not touched.  State is an rt_exposure's
// block on the device: the working histogram (zero between calls), the last metered frame's, and what the meter left.
struct ToneMapRequest {
    struct State { uint32_t hist[256], last[256]; double lbar; float E, scale; uint32_t n, holds; };
    int width, height, op; bool meter;
    State *state;
    double log2_key; float ev_bias, ev_min, ev_max, p_low, p_high, adapt_up, adapt_down;
    float scale, white2, inv_gamma;
    const float *rgb_linear; const int32_t *object_id; float *out_display; uint8_t *out_rgb8;
};

// One bloomed width x height frame (rt_bloom.hip; the definition: rt_mi355x.h, "bloom").  The planes are the caller's device
// pointers (one of out / out_bloom may be NULL; out may be rgb_linear), the parameters are validated by the caller.  state: NULL,
// or an rt_exposure's block -- k_bloom_prefilter takes its scale when it holds a metered frame, else `scale`; it is only read.
// pyramid: the rt_bloom's scratch, the levels one behind the other, 3 floats a texel (bloom_plan's offsets).
#define RT_BLOOM_MAX_LEVELS 32
struct BloomPlan {
    int levels;                         // L of step 3
    int tail;                           // k_bloom_tail starts at this level and runs levels tail .. L-1 in LDS; -1: no tail launch
    int w[RT_BLOOM_MAX_LEVELS], h[RT_BLOOM_MAX_LEVELS];
    size_t off[RT_BLOOM_MAX_LEVELS + 1];        // in texels; off[levels] = the texels of the whole pyramid
};
struct BloomRequest {
    int width, height;
    float threshold, knee_k, intensity, spread, one_minus_spread, scale;   // knee_k = knee * threshold; scale = 2^exposure_ev
    const ToneMapRequest::State *state;
    const float *rgb_linear; float *out, *out_bloom;
    float *pyramid;
    BloomPlan plan;
};

// What the requests of the two tile-gather stages (rt_tile_gather.h) start with: the frame, the tile size K and the taps N, the
// tiles for this call's K, and the object's tile-max and neighbour-max planes (tiles_x * tiles_y entries each).
struct TileGatherHead {
    int width, height, K, N;
    int tiles_x, tiles_y;               // ceil(width / K), ceil(height / K)
    float *tile_max, *tile_nmax;
};

// One motion-blurred width x height frame (rt_motion_blur.hip; the definition: rt_mi355x.h, "motion blur").  The planes are the
// caller's device pointers (out_tiles may be NULL), the parameters are validated by the caller.  tile_max and tile_nmax: the
// rt_motion_blur's scratch, one float2 per tile each.
struct MotionBlurRequest : TileGatherHead {
    float half_shutter;                 // h = 0.5f * shutter
    float two_over_n;                   // g = 2 / N
    float depth_extent;
    const float *rgb_linear, *motion, *z;
    float *out, *out_tiles;
};

// One defocused width x height frame (rt_dof.hip; the definition: rt_mi355x.h, "depth of field").  The planes are the caller's device
// pointers (out_coc and out_tiles may be NULL), the parameters are validated by the caller.  A and focus are step 0's A and focus
// distance; bx, by, u, v, l the camera quantities of step 1 (camera_setup's).  taps: step 5's table on the HOST, 2 N floats -- it
// travels in the kernel argument.  coc: the rt_dof's (c, D) plane, one float2 per pixel; tile_max and tile_nmax: its two tile
// planes, one float per tile each.
#define RT_DOF_MAX_TAPS 64
struct DofRequest : TileGatherHead {
    float A, focus, depth_extent;
    float bx, by, u, v, l;
    const float *taps;
    const float *rgb_linear, *z;
    float *out, *out_coc, *out_tiles;
    float2 *coc;
};

// One in-place update of a mesh on a device (rt_refit.hip; the definition: rt_mi355x.h, "mesh vertex updates").  Everything is the
// mesh's own device memory (DevMeshBufs in rt_host.h): v / vn the new vertices and normals, slot_idx six uint32 per triangle slot
// (the face's three indices into v, then its three into vn), level_nodes the node indices by depth, the deepest level first, and
// level_off (on the HOST, n_levels + 1 entries) where each level starts in it.  n_levels == 0: the mesh is one leaf, only
// k_mesh_retri runs.  after_retri: NULL, or an event recorded between k_mesh_retri and the first refit launch.
struct MeshRefitRequest {
    const float *v, *vn;
    const uint32_t *slot_idx; uint32_t n_slots;
    DevTri *tris; float *nrm;
    DevBvhNode *nodes;
    const uint32_t *level_nodes; const uint32_t *level_off; int n_levels;
    hipEvent_t after_retri;
};

// One mesh's smooth normals computed again on a device (rt_mesh_normals.hip; the definition: rt_mi355x.h, "smooth normals").  v
// and f are the mesh's positions and face indices on the device, nadj_off (n_normals + 1 entries) and nadj_corner (three per
// face) the corners of every normal with the corners of a row ascending; vn (n_normals x 3 floats) holds the stored values and
// receives every normal that is not to keep its own.
struct MeshNormalsRequest {
    const float *v; const uint32_t *f;
    const uint32_t *nadj_off, *nadj_corner; uint32_t n_normals;
    float *vn;
};

// One mesh posed on a device (rt_mesh_pose.hip; the definitions: rt_mi355x.h, "mesh skinning" and "morph targets").  base: nv x 3
// floats.  A MORPH pose: base and deltas (n_targets x nv x 3 floats) are the set as the store checked it; active: n_active
// (0 .. 256) pairs of (uint32 target, float weight), 8 bytes each, ascending by target, every target below the set's n_targets,
// every weight non-zero.  A BONE pose: n_active is 0, deltas and active may be NULL, base is the skin's rest positions.
// n_bones == 0 (only with deltas): no skin, and bone_index, weight and bones are not read; else bone_index (nv x 4 uint16, 8-byte
// aligned) and weight (nv x 4 floats, 16-byte aligned) are the skin as the store checked it -- every index below n_bones -- bones
// the pose, n_bones (1 .. 1024) x 12 floats, 16-byte aligned, and the skin is applied to the morphed position.  out (nv x 3
// floats, not base) receives every position.
struct MeshPoseRequest {
    const float *base; const float *deltas;
    const void *active; uint32_t n_active;
    const uint16_t *bone_index; const float *weight;
    const float *bones; uint32_t n_bones;
    uint32_t nv; float *out;
};

// One measurement of a mesh's tree on a device (rt_refit.hip, k_bvh_cost; the definition: rt_mi355x.h, "mesh tree quality"): the
// n_nodes (> 0, at most 2^28) records at `nodes`, one double per block of 256 terms to partials[0 .. ceil(4 n_nodes / 256)).
// partials has room for one double more: under RT_COST_FOLD_DEVICE k_bvh_cost_fold leaves the sum of the others there.
#ifndef RT_COST_FOLD_DEVICE
#define RT_COST_FOLD_DEVICE 0           /* 1: fold the block sums on the device (the variant that was measured and not kept) */
#endif
struct BvhCostRequest {
    const DevBvhNode *nodes; uint32_t n_nodes;
    double *partials;
};

// One build of a mesh's tree on a device (rt_bvh_build.hip; the definition: rt_mi355x.h, "device tree build").  v, f, fn (and vt, ft
// where the mesh has texture vertices, else NULL with tex) are the mesh on the device, n_faces > 0 of them.  The scratch is the
// caller's (rtk_mesh_build_scratch says how much): two key arrays and the sort's temporary storage, the binary nodes with their
// parents and visit counters, the records' binary nodes and held entries.  nodes has room for n_faces records -- a record stands
// for a binary node with more than four keys beneath it, of which there are fewer than n_faces.  result (device, RT_LBVH_RESULT_WORDS
// words): [0] the record count, [1] the levels, [2] stack_need, [3] 1 when the collapse stopped at RT_LBVH_MAX_LEVELS or at the
// capacity (never for a tree of the definition), [4 + d] where depth d starts (n_levels + 1 entries).  after_*: events recorded
// behind the phases (sort, boxes, collapse); the slots follow the collapse.  A mesh of at most four faces has no hierarchy, boxes
// or collapse launch and a result of zeros.
#define RT_LBVH_MAX_LEVELS 64
#define RT_LBVH_RESULT_WORDS (4 + RT_LBVH_MAX_LEVELS + 1)
struct LbvhBin;
struct MeshBuildScratch {
    float *cbox;                            // [blocks + 1][6]: the workgroups' centroid boxes, then the mesh's
    unsigned long long *keys[2]; void *sort_tmp; size_t sort_tmp_bytes;
    LbvhBin *bin; uint32_t *parent, *visit; // n_faces - 1 each
    uint32_t *rec_bin; int32_t *rec_held;   // n_faces each
};
struct MeshBuildRequest {
    const float *v; const uint32_t *f, *fn; const float *vt; const uint32_t *ft; uint32_t n_faces;
    MeshBuildScratch scratch;
    DevBvhNode *nodes; uint32_t *result;
    uint32_t *slot_face, *slot_idx; float *tex;
    hipEvent_t after_sort, after_boxes, after_collapse;
};

// ---- rt_kernels.hip: the kernels that shade -----------------------------------------------------------------------------
// The ray queue of tree level l >= 1 is W.rq[l & 1] with its count in W.counts[l]: a launch that works on level l reads
// that one and appends the rays it spawns to level l + 1.

// whether k_wavefront (the whole ray tree in one persistent launch) serves this scene and model; else the per-level kernels do
bool rtk_wavefront_usable(const DevScene &S, const rt_params &P);
// The primary samples of a pass, shaded: k_wavefront where usable (whole subtrees on LDS stacks; what does not fit goes to the
// level-1 queue), else k_primary with every secondary ray on the level-1 queue.  Grid of at most max_blocks workgroups.
void rtk_launch_primary(hipStream_t st, const DevScene &S, const DevWork &W, const rt_params &P, const RenderPass &pass, int max_blocks);
// The rays a k_wavefront pass could not keep on its LDS stacks (level 1), traced by a second pass of the same kernel with the
// queue as its source; what does not fit THIS time goes on to level 2 and the per-level launches.  Returns false, having done
// nothing, when the model has no wavefront kernel (the caller then starts the level launches at level 1).
bool rtk_launch_wavefront_queue(hipStream_t st, const DevScene &S, const DevWork &W, const rt_params &P, const RenderPass &pass);
// one level of the ray tree: k_bounce over the queue of `level` (P3 has no secondary rays: no launch)
void rtk_launch_bounce(hipStream_t st, const DevScene &S, const DevWork &W, const rt_params &P, int level, int max_blocks, unsigned long long *fx);
// The feature planes of one chunk (pass.cam, tiles, q0, npix), after its last k_resolve on the same stream: the second-batch
// flags from the chunk's pixel list, then k_features.  `second` is the working set's flag buffer ([npix] bytes, exists only when
// features are on); by_walk: the planes are indexed by the call's tile walk (a strided job's staging buffers) instead of by
// image pixel.
void rtk_launch_features(hipStream_t st, const DevScene &S, const DevWork &W, const rt_params &P, const RenderPass &pass,
                         uint8_t *second, const DevFeatures &out, bool by_walk);

// ---- rt_trace.hip: the kernels that only trace ----------------------------------------------------------------------
// closest hits of n caller-supplied rays (6 floats each) with the intersection code of `model`
void rtk_launch_trace(hipStream_t st, const DevScene &S, int model, const float *rays, long long n, const TraceOut &out);
// k_photon_trace, one thread per attempt
void rtk_launch_photon_trace(hipStream_t st, const DevScene &S, const PhotonArgs &A);

// ---- rt_resolve.hip: resolve, fold and unpack (no rays) -------------------------------------------------------------
// Reproducible mode, once per pass: sample_rgb (the primary contributions) += the secondary plane, and the plane back to zero.
void rtk_launch_fold_fx(hipStream_t st, float *sample_rgb, unsigned long long *fx, size_t samples);
// k_resolve over A.npix pixels, at most max_blocks workgroups (tiles_prepare is run on a copy of A.tiles).  linear: the LIN
// instantiation -- the linear plane A.rgb_linear, or 24-byte records when A.packed is set.  A.variance selects the VAR one.
void rtk_launch_resolve(hipStream_t st, const DevWork &W, const ResolveArgs &A, int max_blocks, bool linear);
void rtk_launch_unpack_tiles(hipStream_t st, const UnpackRequest &R);
// k_unpack_planes: one pass over the image that moves the records and every section of R (the 4-pixel instantiation when the
// geometry keeps every access 16-byte aligned, else one pixel per thread)
void rtk_launch_unpack_planes(hipStream_t st, const UnpackPlanesRequest &R);

// ---- rt_gather.hip: the photon gather ------------------------------------------------------------------------------------
// k_gather as a persistent grid of `blocks` workgroups
void rtk_launch_gather(hipStream_t st, const GatherRequest &R, int blocks);

// ---- rt_denoise.hip: the image-space denoiser ----------------------------------------------------------------------------
// k_denoise_prepare, then k_atrous once per level (the last one remodulates and writes the caller's planes), all on `st`
void rtk_launch_denoise_frame(hipStream_t st, const DenoiseRequest &R);

// ---- rt_temporal.hip: temporal accumulation with camera reprojection ---------------------------------------------------
// k_temporal over the frame on `st`: reads the set `prev` (when has_history), writes the set `next` and the caller's planes
void rtk_launch_temporal(hipStream_t st, const TemporalRequest &R);
// k_temporal_clip over the frame on `st`: the same, with step 4b between the taps and the blend (8512 bytes of LDS a workgroup)
void rtk_launch_temporal_clip(hipStream_t st, const TemporalClipRequest &R);

// ---- rt_motion.hip: motion vectors in image space ------------------------------------------------------------------------
// k_motion over the frame on `st`: reads z, object_id and the node table, writes the motion plane
void rtk_launch_motion(hipStream_t st, const MotionRequest &R);

// ---- rt_motion_mesh.hip: motion vectors for deforming meshes ---------------------------------------------------------------
// k_motion_mesh over the frame on `st`, at most RT_SPILL_BLOCKS workgroups of RT_BLOCK lanes walking the 32 x 8 tiles
void rtk_launch_motion_mesh(hipStream_t st, const MotionMeshRequest &R);

// ---- rt_tonemap.hip: exposure and tone mapping ---------------------------------------------------------------------------
// on `st`: k_luminance_hist and k_exposure_meter (when R.meter), then k_tonemap<R.op>
void rtk_launch_tonemap(hipStream_t st, const ToneMapRequest &R);

// ---- rt_bloom.hip: bloom ahead of tone mapping ------------------------------------------------------------------------------
// the levels a width x height frame gets for `levels` requested, their sizes and offsets, and where the tail kernel starts
BloomPlan rtk_bloom_plan(int width, int height, int levels);
// on `st`: k_bloom_prefilter, k_bloom_down per level above the tail, k_bloom_tail, k_bloom_up per level above it, k_bloom_combine
hipError_t rtk_launch_bloom(hipStream_t st, const BloomRequest &R);

// ---- rt_motion_blur.hip: motion blur between the denoise and bloom ----------------------------------------------------------
// on `st`: k_mblur_tile_max, k_mblur_neighbour_max, k_mblur_gather
hipError_t rtk_launch_motion_blur(hipStream_t st, const MotionBlurRequest &R);

// ---- rt_dof.hip: depth of field between the denoise and motion blur ---------------------------------------------------------
// on `st`: k_dof_coc, k_dof_neighbour_max, k_dof_gather
hipError_t rtk_launch_dof(hipStream_t st, const DofRequest &R);

// ---- rt_refit.hip: mesh vertex updates ------------------------------------------------------------------------------------
// on `st`: k_mesh_retri over the slots, then k_bvh_refit_level once per level, the deepest first
hipError_t rtk_launch_mesh_refit(hipStream_t st, const MeshRefitRequest &R);
// on `st`: k_bvh_cost over all the tree's records in one launch
hipError_t rtk_launch_bvh_cost(hipStream_t st, const BvhCostRequest &R);

// ---- rt_mesh_normals.hip: smooth normals of a deforming mesh -------------------------------------------------------------
// on `st`: k_mesh_normals over the mesh's normals (ahead of k_mesh_retri, which copies them into the slots)
hipError_t rtk_launch_mesh_normals(hipStream_t st, const MeshNormalsRequest &R);

// ---- rt_mesh_pose.hip: a mesh posed on the device by bones, morph targets or both ------------------------------------------
// on `st`: k_mesh_pose over the mesh's vertices (ahead of k_mesh_normals and everything else that reads them): one launch a pose
hipError_t rtk_launch_mesh_pose(hipStream_t st, const MeshPoseRequest &R);

// ---- rt_bvh_build.hip: a mesh's tree built on the device ------------------------------------------------------------------
// bytes of the sort's temporary storage for n_faces keys
size_t rtk_mesh_build_sort_bytes(uint32_t n_faces);
// on `st`: centroid box, keys, sort, radix tree, boxes, collapse, slots (k_mesh_retri is the caller's next launch); *launches: how many
hipError_t rtk_launch_mesh_build(hipStream_t st, const MeshBuildRequest &R, int *launches);

// ---- rt_photon_build.hip: the photon set-up on the GPU ------------------------------------------------------------------
// progress of a photon pass on the device (state_dev[0], and [1] as the shadow a batch writes): attempts consumed, hits counted, photons stored
struct CompactState { unsigned long long attempts, counted; uint32_t stored, pad; };
// origin, cell size and dimensions of the density grid a structure build chose
struct PhotonGridOut { float min[3]; float cell; int dim[3]; };

// scratch = 4 arrays of n_attempts uint32 + the scan's temporary storage
size_t rtk_photon_compact_scratch(uint32_t n_attempts);
// Consumes the attempts of one k_photon_trace batch in order, until max_count is reached (mode 0: photons stored, mode 1:
// diffuse hits counted), and appends their photons to out (1-based, out_cap entries); state_dev carries on from batch to batch.
void rtk_photon_compact(hipStream_t st, const float *recs, const uint32_t *count, uint32_t n_attempts, int mode, unsigned long long max_count,
                        CompactState *state_dev, rt_photon *out, uint32_t out_cap, void *scratch, size_t scratch_bytes);
// ScalePhotonPowers over photons [1, n]
void rtk_photon_scale(hipStream_t st, rt_photon *ph, uint32_t n, float scale);
// out = in without the (at most 8, ascending, 0-based) positions of `skip`: the photons LocatePhotons can reach
void rtk_photon_copy_skipping(hipStream_t st, const rt_photon *in, uint32_t n_in, const uint32_t *skip, uint32_t n_skip, rt_photon *out);
// Scratch of a build over n photons with n_sub sub-leaves: perm x2, keys x2, boxu, sort temp.
size_t rtk_photon_structure_scratch(uint32_t n, uint32_t n_sub);
// Builds pa / pb ((n_sub + 1) * RT_SUB_PHOTONS slots each), box4 (2 * 2 * n_sub float4: heap node i at [2i, 2i+1]; the
// tree over the leaves is its head, the sub-leaf boxes the nodes [n_sub, 2 n_sub)) and the density grid (64^3 counters
// provided; dims / origin / cell come back in grid_out after a stream synchronisation inside this call).
hipError_t rtk_photon_structure(hipStream_t st, const rt_photon *ph, uint32_t n, uint32_t n_sub, float4 *pa, float4 *pb, float4 *box4,
                                uint32_t *grid, PhotonGridOut *grid_out, void *scratch, size_t scratch_bytes);
size_t rtk_photon_unreachable_scratch(uint32_t n);
// ph0: the photons as generated, 1-based ([0] all zero), on the device.  Heap slots [first, last] are wanted.  result (host):
// [0] = number of photons found, [1] = 1 when a median's key was not unique, 2 when the root paths need more levels or segments
// than the search holds (either way the caller must use the host's exact replay), [2..] = their 1-based raw indices (unsorted).
// Returns after the stream has been synchronised.
hipError_t rtk_photon_unreachable(hipStream_t st, const rt_photon *ph0, uint32_t n, uint32_t first, uint32_t last, void *scratch, size_t scratch_bytes,
                                  uint32_t result[16]);
// (position, raw index) records of photons [0, n], 16 bytes each: what the host's replay of BalanceSegment works on
void rtk_photon_pack_positions(hipStream_t st, const rt_photon *ph0, uint32_t n, void *recs16);
// DevPhotonMap::cell_start for `radius`: one entry per cell of the dim[0] x dim[1] x dim[2] density grid
void rtk_photon_cell_start(hipStream_t st, const float4 *tbox, uint32_t n_leaves, const float grid_min[3], float cell, const int dim[3], float radius, uint32_t *start);

#endif
