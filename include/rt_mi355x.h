/*
 * rt_mi355x.h -- C ABI of librt_mi355x.so, the MI355X (gfx950) replacement for the
 * per-pixel render loop of Roia2529/RayTracing-folder (RayTracingFinal / RayTracingProj13).
 *
 * The reference has no C ABI of its own: its boundary is a set of C++ abstract classes plus
 * globals plus three free functions.  Every entry point below names
 * the reference interface it replaces (paths relative to /root/reference;
 * FIN = RayTracingFinal/RayTracingFinal, P13 = RayTracingProj13/RayTracingProj13).
 *
 * Conventions
 *   - plain pointers and sizes only; no C++ or torch types.
 *   - every function returns RT_OK (0) or a negative rt_status; it never throws.
 *     rt_last_error() returns a thread-local message for the last failure.
 *   - "host" pointers are ordinary process memory; "dev" pointers are HIP device pointers
 *     (e.g. torch.Tensor.data_ptr() of a cuda tensor).
 *   - images are row-major, row 0 = top of the image (FIN/include/scene.h:540-656).
 *   - there is NO CPU fallback: calls that need the GPU return RT_ERR_NO_DEVICE when no
 *     gfx950 device is visible.
 */
#ifndef RT_MI355X_H
#define RT_MI355X_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RT_ABI_VERSION 4

typedef int rt_status;
#define RT_OK               0
#define RT_ERR_ARG         -1   /* bad argument (null pointer, out-of-range index, ...)   */
#define RT_ERR_STATE       -2   /* call not allowed in this state (e.g. job still live)  */
#define RT_ERR_NO_DEVICE   -3   /* no HIP device / not gfx950                            */
#define RT_ERR_DEVICE      -4   /* a HIP call failed (message has the HIP error string)  */
#define RT_ERR_IO          -5   /* file could not be read / parsed                       */
#define RT_ERR_LIMIT       -6   /* input exceeds a documented limit                      */

/* ---- scene records (all little-endian, packed exactly as declared) --------------------- */

/* object kinds: the reference's Object subclasses, FIN/include/objects.h:21,79,124 */
#define RT_OBJ_NONE   0
#define RT_OBJ_SPHERE 1
#define RT_OBJ_PLANE  2
#define RT_OBJ_MESH   3

/* One scene-graph node = the reference's Node (+ its Transformation base),
 * FIN/include/scene.h:224-262,438-514.  Matrices are column-major float[9] exactly like
 * cyMatrix3f::data (FIN/include/cyMatrix.h:290-296).  Nodes are listed parent-before-child
 * in the depth-first order TraceNode visits them (FIN/main.cpp:108-130); node 0 is the root
 * (parent = -1).  100 bytes. */
typedef struct rt_node {
    float   tm[9];      /* Transformation::tm  */
    float   itm[9];     /* Transformation::itm */
    float   pos[3];     /* Transformation::pos */
    int32_t parent;     /* index of parent node, -1 for the root */
    int32_t obj_type;   /* RT_OBJ_*                              */
    int32_t mesh;       /* mesh index for RT_OBJ_MESH, else -1   */
    int32_t material;   /* index into materials, -1 = none       */
} rt_node;

/* BVH node in the reference's 28-byte layout, FIN/include/cyBVH.h:187-200:
 * data bit31 = leaf; leaf: bits28-30 = count-1, bits0-27 = offset into elements;
 * internal: bits0-30 = index of first child (second child = first+1).  Root = node 1. */
typedef struct rt_bvh_node {
    float    box[6];
    uint32_t data;
} rt_bvh_node;

/* MtlBlinn parameter block, FIN/include/materials.h:377-383 (88 bytes). */
typedef struct rt_blinn {
    float diffuse[3];
    float specular[3];
    float reflection[3];
    float refraction[3];
    float emission[3];
    float absorption[3];
    float glossiness;
    float ior;
    float reflection_glossiness;
    float refraction_glossiness;
} rt_blinn;

/* lights, FIN/include/lights.h:30-174 */
#define RT_LIGHT_AMBIENT 0
#define RT_LIGHT_DIRECT  1
#define RT_LIGHT_POINT   2
typedef struct rt_light {
    int32_t type;
    float   intensity[3];
    float   position[3];    /* point light            */
    float   direction[3];   /* direct light (unit)    */
    float   size;           /* point light disc size  */
} rt_light;

/* Camera, FIN/include/scene.h:518-536; dir and up already orthonormalised the way
 * LoadScene does it (FIN/xmlload.cpp:124-127). */
typedef struct rt_camera {
    float   pos[3], dir[3], up[3];
    float   fov, focaldist, dof;
    int32_t width, height;
} rt_camera;

/* 24-byte photon, FIN/include/cyPhotonMap.h:47-65 (wire format of the reference's .dat dump,
 * FIN/main.cpp:398-400). */
typedef struct rt_photon {
    float    position[3];
    float    power;
    uint8_t  color[3];
    uint8_t  plane_and_dirz;   /* bits0-1 split plane, bit3 = direction z is negative */
    int16_t  dir_x, dir_y;
} rt_photon;

/* Textures (FIN/include/texture.h, FIN/texture.cpp, FIN/include/scene.h:323-434).
 * RT_TEX_FILE: width x height RGB8 texels at texel_offset (bytes) of the texel array, sampled
 * bilinearly with tiling (TextureFile::Sample); RT_TEX_CHECKER: TextureChecker (color1/color2).
 *
 * Three texture coordinates are undefined in the reference (a NaN, then a NaN converted to int); the library defines them,
 * and agrees with the reference wherever the reference is defined:
 *  - The sphere's v = 0.5 + asin(p.z) / pi is taken from the un-normalised float hit point p, whose |p.z| rounding lifts
 *    above 1 next to a pole: the argument of asin is clamped to [-1, 1], so such a hit has the pole's v.
 *  - The environment coordinate of a direction straight along +-z, where dir.x / (|dir.x| + |dir.y|) is 0/0, takes
 *    x = y = 0, which is the centre (0.5, 0.5) of the environment map; the argument of its asinf is clamped to [-1, 1] too.
 *  - A lookup (file or checker) at a coordinate with a component that is not finite -- a singular map transform can still
 *    make one -- returns black, as RT_MAP_EMPTY does.  Coordinates of magnitude >= 2^31 remain out of scope: their
 *    conversion to int is as undefined here as in the reference. */
#define RT_TEX_FILE    1
#define RT_TEX_CHECKER 2
typedef struct rt_texture {
    int32_t  type;
    int32_t  width, height;
    uint32_t texel_offset;
    float    color1[3], color2[3];
} rt_texture;
/* TextureMap = a texture reference + a Transformation of the uvw coordinate (scene.h:376-398).
 * texture: index into the texture array; RT_MAP_NONE = the colour has no map;
 * RT_MAP_EMPTY = a map whose texture failed to load (samples black, as in the reference). */
#define RT_MAP_NONE  (-1)
#define RT_MAP_EMPTY (-2)
typedef struct rt_texmap {
    int32_t texture;
    float   tm[9], itm[9], pos[3];
} rt_texmap;

/* shading semantics: which snapshot's MtlBlinn::Shade / primitives to follow */
#define RT_SHADE_FIN 0   /* FIN/main.cpp:516-708 (+ FIN primitives, two-sided triangles)      */
#define RT_SHADE_P13 1   /* P13/main.cpp:485-756 (+ P13 primitives, back-face-culled tris)    */
#define RT_SHADE_P12 2   /* RayTracingProj12 main.cpp:341-588: P13's tree + live path-traced GI  */
#define RT_SHADE_P6  3   /* RayTracingProj6 main.cpp:175-340 (BASELINE config 2): children gated by
                            reflection/refraction.Gray() > 0, no light fall-off, no environment;
                            its RenderPixel = 1 sample at the pixel centre, no gamma:
                            min_sample = max_sample = 1, gamma = 1                                 */
#define RT_SHADE_P3  4   /* RayTracingProj3 main.cpp:152-221 (BASELINE config 1): spheres without
                            bias, direct light only, V = camera - p                                */

/* The reference's compile-time #defines (FIN/main.cpp:19-32, FIN/include/lights.h:16-18,
 * FIN/include/materials.h:20-25, FIN/main.cpp:699) as one runtime block.
 * rt_params_default() fills the FIN values. */
typedef struct rt_params {
    int32_t  min_sample;         /* MIN_SAMPLE 4                                    */
    int32_t  max_sample;         /* MAX_SAMPLE 8                                    */
    float    threshold;          /* THRESHOLD 1e-3 (variance gate); <0 = never      */
    int32_t  bounce;             /* BOUNCE 4                                        */
    int32_t  hemisphere_sample;  /* HEMISPHERE_SAMPLE 30 (result discarded in FIN)  */
    int32_t  knn_k;              /* EstimateIrradiance<400>                         */
    float    knn_radius;         /* radius = 1                                      */
    int32_t  shade_model;        /* RT_SHADE_*                                      */
    int32_t  shadow_samples;     /* MIN_SHADOW_SAMPLES 4 (identical rays at size 0) */
    uint32_t seed;               /* counter-RNG seed for stochastic features        */
    double   gamma;              /* #define gamma 2.2 (a double literal)            */
    /* caustic map (RT_SHADE_P13 / P12 only; P13/main.cpp:518-531): EstimateIrradiance<caustic_k> with
     * `caustic_radius` on the scene's caustic photons at diffuse hits reached with specount > 2;
     * caustic_k = 0 (the default, as in the committed reference where the lookup is commented out)
     * switches it off.  prj13.html quotes k = 400, r = 0.5. */
    int32_t  caustic_k;
    float    caustic_radius;
    /* generatePhotonMap (FIN/main.cpp:27,29,350-402): MAX_NUM_OF_PHOTON 1000000 and PHOTON_BOUNCE 8.  rt_render_begin --
     * the replacement of BeginRender, which calls generatePhotonMap() before it spawns its workers (:984-998) -- runs the
     * photon pass first, on the job's thread, when shade_model is RT_SHADE_FIN, photon_count > 0 and the scene holds no
     * photon map yet (rt_scene_set_photons / rt_scene_generate_photons); photon_count = 0 renders the scene as it is.
     * The generator is seeded with `seed`.  The device-side entry points (rt_render_tiles_*) never generate.
     * A map the library generated is DERIVED from the scene (ABI 4): rt_scene_set_nodes / _mesh / _materials / _lights and
     * rt_scene_load_xml drop it, and rt_render_begin makes a new one when photon_count, photon_bounce or seed differ from
     * the ones it was made with -- the reference regenerates on every BeginRender (FIN/main.cpp:984-990).  A map the caller
     * handed over with rt_scene_set_photons is the caller's and stays until it is replaced. */
    int32_t  photon_count;
    int32_t  photon_bounce;
} rt_params;

/* Which tiles of the image this call renders.  Tiles are tile_w x tile_h pixels, numbered
 * row-major over the image; this call renders tiles first, first+stride, ... (< total).
 * first=0, stride=1 renders the whole image.  Replaces pixelIterator (FIN/main.cpp:65-85). */
typedef struct rt_tile_range {
    int32_t tile_w, tile_h;
    int32_t first, stride;
} rt_tile_range;

/* per-job statistics (rays by class, traversal work, kernel time) */
typedef struct rt_stats {
    uint64_t rays_primary, rays_shadow, rays_reflect, rays_refract;
    uint64_t instance_visits;       /* leaf-object transforms applied            */
    uint64_t bvh_nodes_visited;
    uint64_t tris_tested;
    uint64_t photon_queries;
    uint64_t photons_visited;
    uint64_t pixels;
    uint64_t samples;
    double   ms_trace;              /* sum of HIP-event durations: trace+shade kernels   */
    double   ms_gather;             /* photon gather kernels                              */
    double   ms_resolve;            /* resolve kernels                                    */
    double   ms_total;              /* wall time of the job on its stream (events)        */
    uint64_t launches_trace, launches_gather, launches_resolve;
    uint64_t gather_rounds;         /* (query, trial radius) pairs processed by the gather          */
    uint64_t gather_slow;           /* of those, how many overflowed the LDS leaf list               */
    uint64_t gather_leaf_reads;     /* photon slots read by the gather, all passes, in units of 32 slots (1 KiB) */
    /* ABI 2: the trace+shade time by kernel (ms_trace = ms_primary + ms_bounce).  Every ms_* field is a sum
     * of HIP-event intervals on the stream that ran the kernels.  With `streams` == 1 one chunk is in
     * flight at a time and the intervals are EXCLUSIVE kernel times; with more, a kernel shares the GPU
     * with the other chunks' kernels, the intervals overlap in time and their sum exceeds ms_total --
     * do not divide bytes by them then (bench.py takes its roofline from a streams == 1 pass). */
    double   ms_primary, ms_bounce;
    uint64_t launches_primary, launches_bounce;
    uint64_t streams;               /* chunks in flight at once during this call                     */
    uint64_t peak_rays, peak_queries;   /* largest ray-queue level / photon-query count of any chunk */
    uint64_t attempts;              /* ABI 3: 1, or 2 when queues sized from history overflowed and the library rendered the
                                       frame again with worst-case queues (the statistics are those of the last attempt) */
} rt_stats;

typedef struct rt_scene rt_scene;   /* opaque */
typedef struct rt_job   rt_job;     /* opaque */

/* ---- library ---------------------------------------------------------------------------- */
int          rt_abi_version(void);
const char  *rt_last_error(void);
/* number of usable gfx950 devices (0 when none); never fails */
int          rt_device_count(void);
void         rt_params_default(rt_params *p);

/* ---- scene: replaces the global singletons rootNode/materials/lights/objList/photonmap
 *      (FIN/main.cpp:36-49) ------------------------------------------------------------- */
rt_status rt_scene_create(rt_scene **out);
void      rt_scene_destroy(rt_scene *s);

/* Node tree as LoadScene builds it (FIN/xmlload.cpp:65-132,168-261).  nodes[0] is the root (parent -1); every other node's
 * parent precedes it in the array -- nothing more is asked of the array's order.  Rays visit the tree as the reference's
 * TraceNode does, whatever that order is: depth-first from node 0, a node's own object first, then its children by ascending
 * index.  (Where two objects are hit at exactly the same distance the first one visited is the hit; under RT_SHADE_FIN a mesh
 * hit is textured with the uvw of the sphere / plane hit accepted before it.)  A chain root .. node of more than 8 nodes that
 * ends in an object is accepted here and refused with RT_ERR_LIMIT by the first call that lowers the scene for a device. */
rt_status rt_scene_set_nodes(rt_scene *s, const rt_node *nodes, int32_t n);
/* One TriObj (FIN/include/objects.h:124-303): cyTriMesh arrays V/F/VN/FN
 * (FIN/include/cyTriMesh.h:104-111) and its cyBVH node/element arrays
 * (FIN/include/cyBVH.h:202-203).  f/fn are 3 indices per face.  nodes[0] is unused. */
rt_status rt_scene_set_mesh(rt_scene *s, int32_t mesh,
                            const float *v, int32_t nv,
                            const uint32_t *f, int32_t nf,
                            const float *vn, int32_t nvn, const uint32_t *fn,
                            const rt_bvh_node *nodes, int32_t nnodes,
                            const uint32_t *elements);
/* cyTriMesh VT/FT (FIN/include/cyTriMesh.h:108-109): the texture vertices (uvw triples) and the
 * 3 texture indices per face of a mesh already set.  Read by the PROJ13-family triangle, whose
 * hit takes uvw = GetTexCoord(face, barycentric) (P13/include/objects.h:203); the FINAL triangle
 * never writes uvw (FIN/include/objects.h:226-267).  nvt == 0 removes them; a PROJ13 mesh without
 * them leaves uvw as it was (the reference dereferences a null vt there).
 * rt_scene_set_mesh clears them, so call this after it. */
rt_status rt_scene_set_mesh_texcoords(rt_scene *s, int32_t mesh, const float *vt, int32_t nvt,
                                      const uint32_t *ft);
rt_status rt_scene_set_materials(rt_scene *s, const rt_blinn *m, int32_t n);
rt_status rt_scene_set_lights(rt_scene *s, const rt_light *l, int32_t n);
/* environment / background colour (FIN/include/scene.h:406-434; textures: not yet) */
rt_status rt_scene_set_environment(rt_scene *s, const float env_rgb[3], const float bg_rgb[3]);
rt_status rt_scene_get_environment(const rt_scene *s, float env_rgb[3], float bg_rgb[3]);
/* Texture store (replaces the TextureList global, FIN/main.cpp:46) and the maps of the colours the
 * render path samples: per material its diffuse and specular maps (MtlBlinn::Shade samples only
 * those two, FIN/main.cpp:531-532), the environment (SampleEnvironment, :635) and the background
 * (:328).  maps = 2 * n_materials records: [2m] diffuse, [2m+1] specular. */
rt_status rt_scene_set_textures(rt_scene *s, const rt_texture *tex, int32_t n, const uint8_t *texels, uint64_t n_bytes);
rt_status rt_scene_set_material_maps(rt_scene *s, const rt_texmap *maps, int32_t n_materials);
rt_status rt_scene_set_environment_maps(rt_scene *s, const rt_texmap *environment, const rt_texmap *background);
rt_status rt_scene_get_textures(const rt_scene *s, rt_texture *tex, int32_t cap, uint8_t *texels, uint64_t texel_cap,
                                int32_t *n_tex, uint64_t *n_bytes);
rt_status rt_scene_get_maps(const rt_scene *s, rt_texmap *material_maps, int32_t cap, rt_texmap *environment, rt_texmap *background);

/* Balanced photon array exactly as PhotonMap::photons after PrepareForIrradianceEstimation
 * (FIN/include/cyPhotonMap.h:196-218): photons[0] unused, photons[1..n_stored] heap-ordered.
 * n_stored = 0 clears the map (photon term contributes 0). */
rt_status rt_scene_set_photons(rt_scene *s, const rt_photon *photons, uint32_t n_stored);
/* The second map of RayTracingProj13 (`causticmap`, P13/main.cpp:338,379-404): same format, looked up only
 * by the P13-family shading models when rt_params.caustic_k > 0. */
rt_status rt_scene_set_caustic_photons(rt_scene *s, const rt_photon *photons, uint32_t n_stored);

/* Host-side loader with the reference's XML/OBJ schema (FIN/xmlload.cpp:65-554,
 * FIN/include/cyTriMesh.h:263-547, FIN/include/objects.h:137-145).  OBJ names resolve
 * relative to the XML file's directory.  Fills nodes/meshes/materials/lights/camera. */
rt_status rt_scene_load_xml(rt_scene *s, const char *path);
rt_status rt_scene_get_camera(const rt_scene *s, rt_camera *out);

/* Export the host-side arrays (so a caller can hand the same bytes to another consumer).
 * Pass NULL pointers to query counts only. */
rt_status rt_scene_counts(const rt_scene *s, int32_t *n_nodes, int32_t *n_meshes,
                          int32_t *n_materials, int32_t *n_lights, uint32_t *n_photons);
rt_status rt_scene_get_nodes(const rt_scene *s, rt_node *out, int32_t cap);
rt_status rt_scene_get_materials(const rt_scene *s, rt_blinn *out, int32_t cap);
rt_status rt_scene_get_lights(const rt_scene *s, rt_light *out, int32_t cap);
rt_status rt_scene_mesh_counts(const rt_scene *s, int32_t mesh, int32_t *nv, int32_t *nf,
                               int32_t *nvn, int32_t *nnodes);
rt_status rt_scene_get_mesh(const rt_scene *s, int32_t mesh, float *v, uint32_t *f, float *vn,
                            uint32_t *fn, rt_bvh_node *nodes, uint32_t *elements);
rt_status rt_scene_get_mesh_texcoords(const rt_scene *s, int32_t mesh, int32_t *nvt, float *vt,
                                      uint32_t *ft);

/* Image files: what TextureFile::Load gets from lodepng::decode(..., LCT_RGB) / LoadPPM
 * (FIN/texture.cpp:33-91) and RenderImage::SavePNG from lodepng::encode (FIN/include/scene.h:645-655).
 * rt_image_read_rgb with rgb == NULL only reports the size. comps: 1 = grey, 3 = RGB. */
rt_status rt_image_read_rgb(const char *path, int32_t *w, int32_t *h, uint8_t *rgb, uint64_t cap);
rt_status rt_image_write_png(const char *path, const uint8_t *data, int32_t w, int32_t h, int32_t comps);
/* The two derived images of RenderImage (FIN/include/scene.h:591-613 ComputeZBufferImage: 255*(zmax-z)/
 * (zmax-zmin) truncated, BIGFLOAT pixels 0 and ignored by the extrema; :615-637 ComputeSampleCountImage:
 * integer 255*(c-smin)/(smax-smin), all zero when smax == smin).  Bit-exact integer maps; *smax (may be
 * NULL) receives ComputeSampleCountImage's return value.  Host code, no GPU involved. */
rt_status rt_image_zbuffer(const float *zbuffer, int32_t w, int32_t h, uint8_t *zbuffer_img);
/* The linear plane as a file (additive to ABI 4): PFM, 3 channels ("PF\n<w> <h>\n-1.0\n", then little-endian f32 RGB
 * triples, scanlines stored BOTTOM to top as the format requires).  rgb is row-major, row 0 = top, like every image here.
 * rt_image_read_pfm accepts either sign of the scale (negative: little-endian, positive: big-endian samples); rgb == NULL
 * only reports the size; cap counts floats (3*w*h needed).  A malformed or truncated file is RT_ERR_IO, a too small cap
 * RT_ERR_ARG. */
rt_status rt_image_write_pfm(const char *path, const float *rgb, int32_t w, int32_t h);
rt_status rt_image_read_pfm(const char *path, int32_t *w, int32_t *h, float *rgb, uint64_t cap);
/* The same for a one-channel float plane (alpha): "Pf\n<w> <h>\n-1.0\n", one f32 per pixel, scanlines bottom to top.  Each
 * reader takes its own kind only: rt_image_read_pfm refuses "Pf" files, rt_image_read_pfm1 refuses "PF" files (RT_ERR_IO). */
rt_status rt_image_write_pfm1(const char *path, const float *v, int32_t w, int32_t h);
rt_status rt_image_read_pfm1(const char *path, int32_t *w, int32_t *h, float *v, uint64_t cap);
rt_status rt_image_sample_count(const uint8_t *sample_count, int32_t w, int32_t h, uint8_t *sample_count_img, int32_t *smax);

/* generatePhotonMap as a whole (FIN/main.cpp:350-402) on the GPU: the photon pass (rt_photon_pass), ScalePhotonPowers,
 * the optional dump of the unbalanced photons (:397-400 fwrite to a path the reference hard-codes; dat_path == NULL: no
 * dump), PrepareForIrradianceEstimation -- and the result becomes the scene's photon map on every device.  ms_out (may be
 * NULL) receives the wall time of the stages in milliseconds. */
typedef struct rt_setup_ms {
    double photon_pass;      /* emission + bounces + compaction of the stored photons (GPU)                      */
    double balance;          /* what of PrepareForIrradianceEstimation is needed to know the photons LocatePhotons
                                can reach (cyPhotonMap.h:217,371); host                                          */
    double structure_build;  /* decode + median-split sub-leaves + boxes + density grid                          */
    double upload;           /* host <-> device copies of photon records                                         */
    double total;
} rt_setup_ms;
rt_status rt_scene_generate_photons(rt_scene *s, int device, uint32_t max_photons, int photon_bounce, uint32_t seed,
                                    const char *dat_path, rt_setup_ms *ms_out);
/* where the photon pass that rt_render_begin runs (rt_params.photon_count) leaves its .dat dump; NULL (default) = no dump */
rt_status rt_scene_set_photon_dump(rt_scene *s, const char *dat_path);
/* the scene's photon map as PhotonMap::photons after PrepareForIrradianceEstimation (balanced, [0] unused): what
 * rt_scene_set_photons was given, or the balanced form of what rt_scene_generate_photons made.  out == NULL only counts
 * (*n_stored); cap counts records including [0]. */
rt_status rt_scene_get_photons(rt_scene *s, rt_photon *out, uint32_t cap, uint32_t *n_stored);

/* The tree the kernels walk for one mesh of the scene, as the host builds it at upload time (additive to ABI 4; needs no GPU and
 * makes no HIP call): 128-byte node records -- the boxes of up to four children, one axis after the other (float lo[3][4],
 * hi[3][4]), then four child refs (uint32: bit 31 = leaf, bits 28-30 its triangle count - 1, bits 0-27 its first triangle slot;
 * else the index of a node record), then 16 bytes of padding; an unused child has NaN bounds and is never entered -- and the
 * face of every triangle slot.  root_ref is a child ref (a mesh of at most four triangles is one leaf and has no node).
 * stack_need is the largest number of traversal-stack entries a ray can hold in this tree (over root-to-leaf paths, the sum of
 * children - 1): a scene loads when it is at most bvh_lds + bvh_spill.  bvh_lds / bvh_stack are the per-lane LDS entries of
 * k_wavefront / of the other tracing kernels, bvh_spill the entries per thread behind either in HBM, spill_blocks x block the
 * threads the spill buffer has room for.
 * info is required, info->struct_size must be the caller's sizeof (anything else: RT_ERR_ARG).  nodes and slot_face may be NULL
 * (sizes only); otherwise nodes_cap counts 128-byte records, slots_cap faces, and a too small one is RT_ERR_ARG (nothing is written then). */
typedef struct rt_device_bvh_info {
    uint32_t struct_size;
    uint32_t n_nodes, n_slots;
    uint32_t root_ref;
    int32_t stack_need;
    int32_t bvh_lds, bvh_stack, bvh_spill, spill_blocks, block;
} rt_device_bvh_info;
rt_status rt_scene_mesh_device_bvh(const rt_scene *s, int32_t mesh, rt_device_bvh_info *info, void *nodes, uint64_t nodes_cap,
                                   uint32_t *slot_face, uint64_t slots_cap);

/* ---- mesh vertex updates (additive to ABI 4: detected by the presence of the symbols; RT_ABI_VERSION and the structs above are
 *      unchanged) ---------------------------------------------------------------------------------------------------------------
 * New positions (and, optionally, normals) for a mesh whose faces stay as they are: a deforming surface, frame after frame.
 * nv and nvn must be the stored counts (anything else: RT_ERR_ARG, nothing changes); vn == NULL keeps the stored normals (or, for a mesh in RT_MESH_NORMALS_SMOOTH mode, computes them again for
 * the new v: "smooth normals" below).  The
 * scene must be idle (no live job).  flags: 0, or RT_MESH_UPDATE_REBUILD; rt_scene_update_mesh_vertices_flags takes either with or
 * without RT_MESH_UPDATE_KEEP_PREVIOUS.  Any other bit is RT_ERR_ARG.
 *   0        On every device that holds this scene as it is now, the mesh is updated IN PLACE: the vertices are uploaded,
 *            k_mesh_retri writes every triangle slot (A, B, C, the unit face normal computed operation by operation as the host
 *            computes it, the three vertex normals) and k_bvh_refit_level, once per level of the tree from the deepest up, sets
 *            every child box to the exact float min / max of the vertices beneath it.  The tree keeps its topology (refs and
 *            slot order); every box of it is as tight as a fresh build's, so the closest hit of every ray is the fresh build's --
 *            only how many boxes a ray enters can grow as the shape moves away from the one the tree was built for.  The mesh's
 *            root box and the cull boxes of the objects that use it follow; the call returns after the device has finished.
 *            Devices that do not hold the scene (never rendered on, or invalidated by another setter) lower it as usual later.
 *   REBUILD  what rt_scene_set_mesh does: every device builds the tree again at its next use.  For the caller that decides a
 *            refitted tree has degraded ("mesh tree quality" below is the measure of that, and
 *            rt_scene_update_mesh_vertices_auto the call that acts on it).
 * Either way the stored cyBVH arrays are built again for the new vertices when somebody reads them (rt_scene_get_mesh returns
 * what rt_bvh_build with leaves of four gives), and a photon map made by the photon pass is dropped, as by rt_scene_set_mesh.
 *   KEEP_PREVIOUS  (rt_scene_update_mesh_vertices_flags and rt_scene_update_mesh_vertices_auto_flags only: the two calls that came
 *            before the flag take the bits they always took, so a caller that relied on RT_ERR_ARG for it still gets it.  Combines
 *            with either of the above.)  The positions the mesh had before this call become its PREVIOUS POSITIONS: nv x 3 floats,
 *            indexed like v, which "motion vectors for deforming meshes" below follows a pixel through.  They are kept in the scene
 *            store, so that a later lowering or rebuild uploads them, and on every device that holds the scene: uploaded from the
 *            store ahead of the new vertices, in the update's stream.  They are per vertex, not per triangle slot, so they survive
 *            REBUILD and rt_scene_update_mesh_vertices_auto's rebuild.  rt_scene_set_mesh drops them (the faces may have changed),
 *            and so does an update WITHOUT the flag (the caller no longer vouches for the pairing): the mesh is rigid again.  The
 *            contract is one flagged update per mesh per frame; the previous positions are those before the LAST flagged update.
 *            Without the flag an update does what it always did, launch for launch, and nothing is allocated for a mesh that
 *            never used it. */
#define RT_MESH_UPDATE_REBUILD 1u
#define RT_MESH_UPDATE_KEEP_PREVIOUS 2u
rt_status rt_scene_update_mesh_vertices(rt_scene *s, int32_t mesh, const float *v, int32_t nv, const float *vn, int32_t nvn,
                                        uint32_t flags);
/* the same call, taking RT_MESH_UPDATE_KEEP_PREVIOUS as well (flags 0 and RT_MESH_UPDATE_REBUILD do what they do above) */
rt_status rt_scene_update_mesh_vertices_flags(rt_scene *s, int32_t mesh, const float *v, int32_t nv, const float *vn, int32_t nvn,
                                              uint32_t flags);
/* What sits on `device` for one mesh right now (the scene is lowered there first if it is not): info, nodes, slot_face as
 * rt_scene_mesh_device_bvh describes them -- after an in-place update the refitted tree, not the one a fresh build would give --
 * and per triangle slot its 12 floats of A, B, C, N and its 9 floats of vertex normals, and the mesh's root box (lo[3], hi[3]).
 * info is required and its struct_size checked; every other pointer may be NULL.  nodes_cap counts node records; slots_cap counts
 * slots and holds for slot_face, tris and nrm alike.  A too small capacity is RT_ERR_ARG and nothing is written. */
rt_status rt_scene_mesh_device_read(rt_scene *s, int device, int32_t mesh, rt_device_bvh_info *info, void *nodes, uint64_t nodes_cap,
                                    uint32_t *slot_face, uint64_t slots_cap, float *tris, float *nrm, float root_box[6]);
/* The last in-place update on `device`, timed with events on the library's stream: milliseconds of the vertex upload, of
 * k_mesh_retri and of the refit launches, and how many of those there were (one per level of the tree).  RT_ERR_STATE when that
 * device has not run one. */
typedef struct rt_mesh_update_ms {
    uint32_t struct_size;
    int32_t level_launches;
    float upload, retri, refit;
} rt_mesh_update_ms;
rt_status rt_scene_mesh_update_ms(rt_scene *s, int device, rt_mesh_update_ms *out);

/* ---- mesh tree quality (additive to ABI 4: detected by the presence of the symbols) --------------------------------------------
 * A refitted tree keeps the topology of the shape it was built for and gets slower to trace as the mesh moves away from it.  The
 * measure of that is the surface-area-heuristic (SAH) cost of the tree that sits on the device, against the cost the same mesh's
 * tree had when it was last built.  The definition fixes every operation and the order of every addition, so that the GPU
 * (k_bvh_cost) and the host mirror (rt_device_bvh_cost) give the same eight bytes.
 *
 * For a mesh whose tree has a root node (root_ref is not a leaf ref), over its n_nodes node records:
 *   term(n, c)  for record n and child c in 0..3: 0 when the child is unused (its lo bound on x is NaN); otherwise h(box(n, c)) * w
 *               as ONE float32 product, where
 *                 h    is half the surface area in float32: d = hi - lo per axis, then (dx*dy + dy*dz) + dz*dx, no contraction;
 *                 w    is 1.0f for an internal child and the leaf's triangle count (1..4: bits 28-30 of the ref, plus 1) for a leaf.
 *               The float32 term is converted to double before any summing.
 *   S           the sum of the 4 * n_nodes terms in double, in term order t = 4 n + c, with THIS order of additions: the terms
 *               are cut into blocks of 256 consecutive ones (the last padded with +0.0); a block is summed as the balanced binary
 *               tree over the bits of the index inside the block, lowest bit first --
 *                 ((t0 + t1) + (t2 + t3)) + ((t4 + t5) + (t6 + t7)), and so on up to the two halves of 128 --
 *               which is what an xor-butterfly over the lane index leaves in lane 0 of a wave of 64 and, above it, (w0 + w1) +
 *               (w2 + w3) over the four waves of a workgroup; the block sums are then added one after the other in block order,
 *               starting from +0.0.
 *   H_R         h of the root box: per axis the smallest lo and the largest hi over the used children of the root record.
 *   cost        1 + S / (double)H_R
 * A mesh that is one leaf (root_ref is a leaf ref, no node records) has cost = 1 + its triangle count.
 * RT_MESH_QUALITY_DEGENERATE: H_R is 0, or S or H_R is not finite (a tree without extent, or one whose areas overflow float32).
 * A degenerate result has cost = 0 and ratio = 1 and never triggers a rebuild.
 *
 * rt_device_bvh_cost is the host mirror: plain C++, no HIP call, on the records rt_scene_mesh_device_bvh and
 * rt_scene_mesh_device_read return.  RT_ERR_ARG: cost or flags NULL; root_ref not a leaf ref and its index >= n_nodes, or
 * nodes NULL.  *flags: 0 or RT_MESH_QUALITY_DEGENERATE. */
#define RT_MESH_QUALITY_DEGENERATE    1u
#define RT_MESH_QUALITY_REBUILT       2u   /* rt_scene_update_mesh_vertices_auto went on to RT_MESH_UPDATE_REBUILD's path        */
#define RT_MESH_QUALITY_NOT_ON_DEVICE 4u   /* no device held the scene: nothing was refitted or measured                        */
rt_status rt_device_bvh_cost(const void *nodes, uint64_t n_nodes, uint32_t root_ref, double *cost, uint32_t *flags);
/* The query: the scene is lowered on `device` first if it is not there (as by rt_scene_mesh_device_read, and with its
 * discipline: the device is claimed, a pending render waited for), k_bvh_cost runs on the library's stream -- one launch over all
 * levels, one double per 256 terms, folded on the host after one small copy -- and the call returns after it.  built_cost is the
 * cost of the tree as the host built it when the mesh was last lowered there (from the host mirror on the host's records: no
 * launch); it changes whenever the mesh is built again.  ratio = cost / built_cost, exactly 1 for a tree nobody has refitted.
 * A degenerate cost OR built_cost flags the result degenerate.  struct_size must be the caller's sizeof (else RT_ERR_ARG).
 * measure_ms: HIP events around k_bvh_cost and the copies that bring its block sums and the root record to the host. */
typedef struct rt_mesh_quality {
    uint32_t struct_size;
    uint32_t flags;          /* RT_MESH_QUALITY_DEGENERATE | _REBUILT | _NOT_ON_DEVICE */
    double   cost;           /* of the tree on the device now */
    double   built_cost;     /* of the tree as it was last built for this mesh */
    double   ratio;          /* cost / built_cost */
    float    measure_ms;     /* HIP events around k_bvh_cost and its fold */
} rt_mesh_quality;
rt_status rt_scene_mesh_quality(rt_scene *s, int device, int32_t mesh, rt_mesh_quality *out);
/* The update that uses it.  Arguments and their checks are rt_scene_update_mesh_vertices's, and max_ratio must be finite and
 * >= 1 (else RT_ERR_ARG, nothing changes); out may be NULL, otherwise its struct_size is checked the same way.  The call does
 * exactly what flags 0 does -- upload, k_mesh_retri, the refit launches, root box and cull boxes -- and measures the refitted
 * tree behind the refit, in the same stream, before the final synchronise: on the first device that holds the scene (every
 * device holds the same tree: the same host build, the same exact refit).  If ratio > max_ratio it then does what
 * RT_MESH_UPDATE_REBUILD does -- every device builds the tree again at its next use -- and sets RT_MESH_QUALITY_REBUILT; out holds
 * the REFITTED tree's cost, the one that triggered the rebuild.  If no device holds the scene there is nothing to refit or
 * measure: flags = RT_MESH_QUALITY_NOT_ON_DEVICE, cost = built_cost = 0, ratio = 1, and the next lowering builds a fresh tree
 * anyway.  There is no default for max_ratio: README.md has the measured table of SAH ratio against frame time to choose from. */
rt_status rt_scene_update_mesh_vertices_auto(rt_scene *s, int32_t mesh, const float *v, int32_t nv, const float *vn, int32_t nvn,
                                             double max_ratio, rt_mesh_quality *out);
/* ... with flags: 0 (the call above) or RT_MESH_UPDATE_KEEP_PREVIOUS; any other bit is RT_ERR_ARG (REBUILD is what max_ratio decides) */
rt_status rt_scene_update_mesh_vertices_auto_flags(rt_scene *s, int32_t mesh, const float *v, int32_t nv, const float *vn, int32_t nvn,
                                                   double max_ratio, uint32_t flags, rt_mesh_quality *out);
/* How many meshes of the scene hold previous positions, from the scene store (no GPU, no HIP call). */
rt_status rt_scene_previous_positions(const rt_scene *s, int32_t *n_meshes);
/* The previous positions of one mesh as they sit on `device` (the scene is lowered there first if it is not, with
 * rt_scene_mesh_device_read's discipline): *nv_out = their number, the mesh's nv, or 0 when the mesh holds none (nothing is written
 * then).  v_prev may be NULL (the count only); otherwise nv_cap counts vertices and a too small one is RT_ERR_ARG. */
rt_status rt_scene_mesh_device_previous(rt_scene *s, int device, int32_t mesh, float *v_prev, uint64_t nv_cap, uint32_t *nv_out);

/* ---- device tree build (additive to ABI 4: detected by the presence of the symbols; RT_ABI_VERSION and the structs above are
 *      unchanged) ---------------------------------------------------------------------------------------------------------------
 * A mesh's tree built again ON THE DEVICE that holds the mesh, for the caller whose refitted tree has degraded and who cannot
 * afford what RT_MESH_UPDATE_REBUILD costs (binned SAH on one host thread, then the whole scene lowered again).  The tree is a
 * linear BVH: a binary radix tree over Morton-sorted triangles, collapsed four-wide into the node records described at
 * rt_scene_mesh_device_bvh.  It is a worse tree than the host's (DESIGN.md section 3 has the measured costs) and it is opt-in:
 * nothing above changes what it does.  The definition fixes every choice, so that the kernels (csrc/rt_bvh_build.hip) and the host
 * mirror (rt_device_lbvh_build) produce the same tree; the arithmetic is written once, in csrc/rt_lbvh.h.  No product is fused
 * into a sum; every min / max keeps the value held so far unless the new one is smaller / larger (std::min / std::max).
 *
 * For a mesh of nf faces over the vertices v:
 *   1. boxes     per face, lo / hi are the min / max of its three vertices and its centroid is c = 0.5f * (lo + hi) (what the host
 *                builder uses); clo / chi are the min / max over all centroids.
 *   2. key       per axis q = clamp((int)((c - clo) * (1024.0f / (chi - clo))), 0, 1023), and q = 0 when chi - clo is not > 0 or
 *                not finite (flat and degenerate meshes).  The 30-bit Morton code interleaves qx, qy, qz (x highest); the 64-bit
 *                key is morton << 32 | face.  No two keys are equal, so every correct ascending sort gives the same order.
 *   3. slots     slot i holds the face of the i-th key (slot_face[i]).  A leaf's triangles are a contiguous slot range, in KEY
 *                order -- not by face index as in the host builder's leaves.  The closest hit does not depend on it; only two
 *                triangles at a bit-equal closest t could show the difference.
 *   4. tree      the binary radix tree of Karras (2012) over the sorted keys, delta(i, j) = clz64(k_i ^ k_j) and -1 out of range.
 *                A subtree whose key range holds at most 4 keys while its parent's holds more is a leaf (1..4 triangles).  nf <= 4
 *                is a root leaf and no node record.
 *   5. boxes     every box is the exact min / max of the vertices beneath it: no rounding, no padding.  A bound is defined up
 *                to the sign of a zero.
 *   6. collapse  a record stands for a binary node: it starts from that node's two children; while it has fewer than four and an
 *                internal one is left, the internal child with the largest 2 (dx dy + dy dz + dz dx) -- the first of equals -- is
 *                replaced by its two children, in place.  Unused children have NaN bounds and the ref of a leaf of one triangle at slot 0.
 *   7. numbering breadth-first: the root is record 0, the records of depth d + 1 follow those of depth d, ordered by (parent
 *                record, child position).
 *   8. stack_need  the maximum over root-to-leaf paths of the sum of (children - 1), as everywhere.  Nothing bounds it below
 *                bvh_lds + bvh_spill for every mesh (the radix tree can be 58 levels deep): a tree that needs more is not accepted
 *                by the build calls below, which fall back to RT_MESH_UPDATE_REBUILD's path and say so.
 *
 * rt_device_lbvh_build is the host mirror: plain C++, no GPU, no HIP call, on bare arrays (v: nv x 3 floats, f: nf x 3 indices
 * below nv, both required and positive in number, else RT_ERR_ARG).  info, nodes, nodes_cap, slot_face and slots_cap are those of
 * rt_scene_mesh_device_bvh: sizes only with NULL buffers, RT_ERR_ARG and nothing written when a capacity is too small. */
rt_status rt_device_lbvh_build(const float *v, int32_t nv, const uint32_t *f, int32_t nf, rt_device_bvh_info *info, void *nodes,
                               uint64_t nodes_cap, uint32_t *slot_face, uint64_t slots_cap);
/* What a build call reports.  struct_size must be the caller's sizeof (else RT_ERR_ARG).  flags is exactly one of
 *   ON_DEVICE      every device that held the scene built the tree; the figures are the first such device's;
 *   FELL_BACK      that device's tree came out with stack_need above the limit: the call took RT_MESH_UPDATE_REBUILD's path
 *                  (every device lowers the scene again at its next use); stack_need is the refused tree's;
 *   NOT_ON_DEVICE  no device held the scene: there was nothing to build on, the next lowering builds the host's tree.
 * The milliseconds are HIP events on the library's stream: the vertex (and, the first time, index) upload; centroid box, keys and
 * the sort; the radix tree and its boxes; the collapse; the slots with k_mesh_retri; k_bvh_cost.  launches counts the kernel
 * launches of the build (the sort's own included as one), syncs its host synchronisations. */
#define RT_MESH_BUILD_ON_DEVICE     1u
#define RT_MESH_BUILD_FELL_BACK     2u
#define RT_MESH_BUILD_NOT_ON_DEVICE 4u
typedef struct rt_mesh_build_info {
    uint32_t struct_size;
    uint32_t flags;
    uint32_t n_nodes, n_slots, root_ref;
    int32_t  stack_need, levels;
    int32_t  launches, syncs;
    uint32_t pad;
    double   cost;           /* of the tree just built (k_bvh_cost): the device's built_cost from now on */
    float    upload_ms, sort_ms, hierarchy_ms, collapse_ms, slots_ms, cost_ms;
} rt_mesh_build_info;
/* The update that builds.  Arguments, their checks and their messages are rt_scene_update_mesh_vertices_flags's; flags is 0 or
 * RT_MESH_UPDATE_KEEP_PREVIOUS, any other bit RT_ERR_ARG; out may be NULL.  The store takes the new vertices as for REBUILD (the
 * cyBVH arrays go stale, a generated photon map is dropped, the previous positions follow the flag); then every device that holds
 * the scene builds the mesh's tree from the vertices it has just been sent -- per-face index arrays and texture vertices go to a
 * device once, at the mesh's first build there -- writes the slots in the new order (k_mesh_retri, and tex where the mesh has
 * texture vertices), takes the root box and the cull boxes, and measures the new tree with k_bvh_cost: that cost is the device's
 * built_cost from then on, so rt_scene_mesh_quality's ratio is exactly 1 after a build.  A later flags-0 update refits the
 * device-built tree and rt_scene_mesh_device_read returns it.  A device that is in use or fails lowers the scene again at its
 * next use, as after an in-place update.  A device that lowers the scene LATER gets the host's SAH tree: the devices of one scene
 * can hold different trees from then on, and rt_scene_update_mesh_vertices_auto's measurement speaks for the first device only.
 * The limit on stack_need is bvh_lds + bvh_spill; the test hook RT_LBVH_STACK_CAP (environment, read at call time, like
 * RT_QUEUE_CAP) lowers it. */
rt_status rt_scene_update_mesh_vertices_build(rt_scene *s, int32_t mesh, const float *v, int32_t nv, const float *vn, int32_t nvn,
                                              uint32_t flags, rt_mesh_build_info *out);
/* rt_scene_update_mesh_vertices_auto_flags, building on the device instead of invalidating when ratio > max_ratio: q is as there
 * (RT_MESH_QUALITY_REBUILT set, the REFITTED tree's cost), out as above (flags 0 when nothing was built).  Either may be NULL. */
rt_status rt_scene_update_mesh_vertices_auto_build(rt_scene *s, int32_t mesh, const float *v, int32_t nv, const float *vn, int32_t nvn,
                                                   double max_ratio, uint32_t flags, rt_mesh_quality *q, rt_mesh_build_info *out);

/* ---- smooth normals (additive to ABI 4: detected by the presence of the symbols; RT_ABI_VERSION and the structs above are
 *      unchanged) ---------------------------------------------------------------------------------------------------------------
 * The vertex normals of a deforming mesh, computed again from its new positions at every update, on the device that refits it:
 * the normals a mesh gets when it brings none (cyTriMesh::ComputeNormals), with the order of every addition fixed, so that the
 * kernel (csrc/rt_mesh_normals.hip) and the host mirror (rt_mesh_smooth_normals) give the same bytes.  The arithmetic is written
 * once, in csrc/rt_mesh_normals.h.
 *
 * For a mesh with faces f, normal indices fn (both nf x 3) and positions v:
 *   corner    c = 3 i + k (k in 0..2) belongs to face i.
 *   N_i       the face's unnormalised normal cross(v[f[3i+1]] - v[f[3i]], v[f[3i+2]] - v[f[3i]]), operation by operation as
 *             k_mesh_retri and rt::Point3 compute it: float32, no product fused into a sum, with u and w the two differences the
 *             components uy*wz - uz*wy, uz*wx - ux*wz, ux*wy - uy*wx.
 *   S_j       starts at (0, 0, 0); N_i is added per component for every corner c with fn[c] == j, IN ASCENDING c (a face that
 *             names j at two corners is added twice, as ComputeNormals adds it).
 *   normal j  S_j / sqrtf(S_j.x^2 + S_j.y^2 + S_j.z^2): the sum of squares left to right, / and sqrtf correctly rounded.
 *   kept      a normal that no corner refers to keeps its stored value, and so does one whose length is 0 or not finite.
 * With fn == f and no degenerate input this is ComputeNormals byte for byte; with an OBJ's own fn != f it keeps the OBJ's seams.
 *
 * rt_mesh_smooth_normals is the host mirror: plain C++, no GPU, no HIP call, on bare arrays.  fn == NULL stands for f (nvn must
 * be able to hold its indices).  vn_inout holds the stored values on entry (nvn x 3 floats) and the normals on return.  RT_ERR_ARG
 * and nothing written: a NULL or empty array, a face index >= nv, a normal index >= nvn. */
rt_status rt_mesh_smooth_normals(const float *v, int32_t nv, const uint32_t *f, const uint32_t *fn, int32_t nf, float *vn_inout,
                                 int32_t nvn);
/* The mode of one mesh: what an update that brings no normals (vn == NULL) leaves the mesh with.
 *   STORED  (the default) the normals it had: everything above is what it was, launch for launch, and nothing is allocated.
 *   SMOOTH  the normals defined above for the new v -- after every one of the six update calls, in the store (rt_scene_get_mesh,
 *           and every later lowering: the store runs the mirror when its normals are next read, not inside the update) and on
 *           every device that holds the scene: k_mesh_normals writes the mesh's normals between the vertex upload and
 *           k_mesh_retri, which copies them into the slots; the refit or the build follows.  What the kernel works from -- the
 *           corners of every normal, nadj_off[nvn + 1] and nadj_corner[3 nf] with the corners of a row ascending, and the
 *           faces -- goes to a device once, at the mesh's first such update there.  A kept normal is not written: it keeps
 *           what the device's array held, the value last uploaded or computed there.
 * An update that does bring vn uses them for that call, in either mode.  Setting the mode touches no normal: it takes effect at
 * the next update.  rt_scene_set_mesh resets the mode to STORED, as it drops previous positions.  The scene must be idle; an
 * unknown mode or a mesh never set is RT_ERR_ARG and nothing changes. */
#define RT_MESH_NORMALS_STORED 0u
#define RT_MESH_NORMALS_SMOOTH 1u
rt_status rt_scene_set_mesh_normals_mode(rt_scene *s, int32_t mesh, uint32_t mode);
rt_status rt_scene_get_mesh_normals_mode(const rt_scene *s, int32_t mesh, uint32_t *mode);
/* Milliseconds of the last k_mesh_normals launch on `device`, by HIP events on the library's stream.  RT_ERR_STATE when that
 * device has run none (rt_mesh_update_ms does not grow: its struct_size is checked).  The launch sits behind the uploads and
 * ahead of the event that ends them: in SMOOTH mode rt_mesh_update_ms.upload and rt_mesh_build_info.upload_ms include it. */
rt_status rt_scene_mesh_normals_ms(rt_scene *s, int device, float *ms);

/* ---- mesh skinning (additive to ABI 4: detected by the presence of the symbols; RT_ABI_VERSION and the structs above are
 *      unchanged) ---------------------------------------------------------------------------------------------------------------
 * A second source of new vertices for the in-place update: linear-blend skinning on the device.  A skin is bound to a mesh once;
 * after that a frame brings a pose -- a few dozen matrices instead of a vertex array -- and k_mesh_pose (csrc/rt_mesh_pose.hip)
 * writes the posed positions where the refit, the device build, k_mesh_normals and k_motion_mesh read them.  The definition fixes
 * every operation and its order, so that the kernel and the host mirror (rt_mesh_skin) give the same bytes; the arithmetic is
 * written once, in csrc/rt_mesh_pose.h.
 *
 * A skin    belongs to one mesh of a scene: n_bones (1 .. RT_MESH_SKIN_MAX_BONES); per vertex four influences, bone_index as
 *           uint16[nv][4] and weight as float32[nv][4]; and the REST POSE, a copy of the positions the mesh holds when the skin
 *           is bound.  Every index must be < n_bones, every weight finite and >= 0.  Weights are used as given: the library does
 *           not normalise them.  An unused influence is weight 0 on any valid bone.
 * A pose    is n_bones matrices, float32[n_bones][3][4], row-major, in the mesh's object space (the space its vertices are in,
 *           under its node).  Every one of the 12 n_bones floats must be finite (checked on the host), n_bones must be the skin's.
 * The posed position of vertex i with rest position (x, y, z), for each row r of the output:
 *           for k = 0, 1, 2, 3 (ascending; all four always evaluated), with M = bones[bone_index[i][k]], w = weight[i][k]:
 *               t   = ((M[r][0]*x + M[r][1]*y) + M[r][2]*z) + M[r][3]
 *               acc = (k == 0) ? w*t : acc + w*t
 *           p[r] = acc
 *           Every * and + is one IEEE float32 operation, rounded to nearest; nothing is fused.
 * Normals   A pose brings none: it behaves exactly as an update with vn == NULL.  RT_MESH_NORMALS_STORED keeps the stored normals;
 *           RT_MESH_NORMALS_SMOOTH recomputes them from the posed positions (k_mesh_normals on the devices, the mirror in the
 *           store).  Skinned meshes are expected to use SMOOTH mode.
 *
 * rt_mesh_skin is the host mirror: plain C++, no scene, no GPU, no HIP call, on bare arrays; v_out (nv x 3 floats) may be v_rest.
 * RT_ERR_ARG and nothing written: a NULL array, nv <= 0, n_bones outside 1 .. RT_MESH_SKIN_MAX_BONES, an index >= n_bones, a
 * weight that is negative or not finite, a bone entry that is not finite. */
#define RT_MESH_SKIN_MAX_BONES 1024
rt_status rt_mesh_skin(const float *v_rest, int32_t nv, const uint16_t *bone_index, const float *weight, const float *bones,
                       int32_t n_bones, float *v_out);
/* Binds a skin to a mesh: the arrays are copied, the rest pose is taken from the store's current vertices, and nv must be the
 * mesh's.  A refused argument is RT_ERR_ARG and nothing changes.  A skin already bound is replaced.  rt_scene_set_mesh drops the
 * skin; a plain rt_scene_update_mesh_vertices* call on a skinned mesh keeps the skin and the rest pose and simply replaces the
 * current positions (the next pose starts from the rest pose again).  The scene must be idle. */
rt_status rt_scene_set_mesh_skin(rt_scene *s, int32_t mesh, int32_t n_bones, const uint16_t *bone_index, const float *weight, int32_t nv);
/* Unbinds it (RT_OK when there is none): the mesh keeps the positions it has, and what the devices held of the skin is released. */
rt_status rt_scene_clear_mesh_skin(rt_scene *s, int32_t mesh);
/* bound: 0 / 1, with n_bones and nv of the skin (0 when none is bound).  store_current: 1 when the store's per-vertex positions
 * are those of the last pose, 0 while they are still owed by the mirror -- a pose leaves the store with the matrices only, and
 * the mirror runs when the positions are next read (rt_scene_get_mesh, a lowering, rt_scene_set_mesh_skin).  struct_size must be
 * the caller's sizeof (else RT_ERR_ARG). */
typedef struct rt_mesh_skin_info {
    uint32_t struct_size;
    uint32_t bound;
    int32_t  n_bones, nv;
    uint32_t store_current;
} rt_mesh_skin_info;
rt_status rt_scene_mesh_skin_info(const rt_scene *s, int32_t mesh, rt_mesh_skin_info *out);
/* The pose: rt_scene_update_mesh_vertices_flags with the vertices of the definition above in place of v and with vn == NULL, on the
 * same entry path -- the same flags (RT_MESH_UPDATE_REBUILD, RT_MESH_UPDATE_KEEP_PREVIOUS; any other bit RT_ERR_ARG), the same
 * statuses, the same store discipline (tree stale, a generated photon map dropped).  On every device that holds the scene the
 * vertex upload is replaced by an upload of the bones (48 n_bones bytes) and one launch of k_mesh_pose ahead of k_mesh_normals;
 * rest pose, indices and weights go to a device once, at the mesh's first pose there.  With KEEP_PREVIOUS the device's previous
 * positions become the buffer its positions were in and the kernel writes the other one: two pointers are swapped, nothing is
 * uploaded or copied.  The mesh's root box and the objects' cull boxes come from the root record of the first device's refitted
 * (or built) tree, which holds the exact min / max of the vertices under the faces -- a second short synchronise in the refit; a
 * mesh whose tree is a single leaf has no such record and is posed by the mirror and uploaded as before.  With no device holding
 * the scene the store records the pose and the next lowering resolves it.  A pose on a mesh without a skin is RT_ERR_STATE, a
 * wrong n_bones or a bone that is not finite RT_ERR_ARG; nothing changes then. */
rt_status rt_scene_pose_mesh(rt_scene *s, int32_t mesh, const float *bones, int32_t n_bones, uint32_t flags);
/* ... as rt_scene_update_mesh_vertices_auto_flags (flags: 0 or RT_MESH_UPDATE_KEEP_PREVIOUS) */
rt_status rt_scene_pose_mesh_auto(rt_scene *s, int32_t mesh, const float *bones, int32_t n_bones, uint32_t flags, double max_ratio,
                                  rt_mesh_quality *out);
/* ... as rt_scene_update_mesh_vertices_build */
rt_status rt_scene_pose_mesh_build(rt_scene *s, int32_t mesh, const float *bones, int32_t n_bones, uint32_t flags, rt_mesh_build_info *out);
/* ... as rt_scene_update_mesh_vertices_auto_build */
rt_status rt_scene_pose_mesh_auto_build(rt_scene *s, int32_t mesh, const float *bones, int32_t n_bones, uint32_t flags, double max_ratio,
                                        rt_mesh_quality *q, rt_mesh_build_info *out);
/* Milliseconds of the last k_mesh_pose launch for a bone pose on `device`, by HIP events on the library's stream.  RT_ERR_STATE when that device
 * has run none.  Like k_mesh_normals it sits inside rt_mesh_update_ms.upload and rt_mesh_build_info.upload_ms. */
rt_status rt_scene_mesh_skin_ms(rt_scene *s, int device, float *ms);

/* ---- morph targets (additive to ABI 4: detected by the presence of the symbols; RT_ABI_VERSION and the structs above are
 *      unchanged) ---------------------------------------------------------------------------------------------------------------
 * A third source of new vertices for the in-place update: blend shapes on the device, ahead of the skin.  A morph set is bound to a
 * mesh once; after that a frame brings one weight a target -- and, for a skinned mesh, its bones -- and k_mesh_pose
 * (csrc/rt_mesh_pose.hip) writes the positions where the refit, the device build, k_mesh_normals and k_motion_mesh read them.
 * The definition fixes every operation and its order, so that the kernel and the host mirror (rt_mesh_morph) give the same bytes;
 * the arithmetic, and the order of morph and skin, is written once, in csrc/rt_mesh_pose.h.
 *
 * A morph set belongs to one mesh of a scene: n_targets (1 .. RT_MESH_MORPH_MAX_TARGETS); the deltas, float32[n_targets][nv][3],
 *           dense, in the mesh's object space, every one finite; and the BASE, a copy of the positions the mesh holds when the
 *           set is bound.
 * Weights   A frame brings float32[n_targets], every one finite, of any sign and size: negative weights and weights above 1 are
 *           used as given.
 * The morphed position of vertex i with base (x, y, z), for each component c:
 *               acc = base[i][c]
 *               for t ascending over the targets with weights[t] != 0:   acc = acc + weights[t] * deltas[t][i][c]
 *           Every * and + is one IEEE float32 operation, rounded to nearest; nothing is fused.  A target whose weight is +0 or -0
 *           is SKIPPED, not multiplied: with every weight zero the result is the base byte for byte, a -0.0 coordinate included
 *           (-0 + (+0) would be +0).
 * With a skin   When the pose also brings bones, the posed position is the formula of "mesh skinning" applied to the morphed
 *           position in place of the skin's rest position (x, y, z); the skin's own rest pose is not read.
 * Normals   A morph pose brings none, exactly as a bone pose: RT_MESH_NORMALS_STORED keeps the stored normals,
 *           RT_MESH_NORMALS_SMOOTH recomputes them from the new positions (k_mesh_normals on the devices, the mirror in the store).
 *
 * rt_mesh_morph is the host mirror: plain C++, no scene, no GPU, no HIP call, on bare arrays; v_out (nv x 3 floats) may be v_base.
 * RT_ERR_ARG and nothing written: a NULL array, nv <= 0, n_targets outside 1 .. RT_MESH_MORPH_MAX_TARGETS, a delta or a weight
 * that is not finite. */
#define RT_MESH_MORPH_MAX_TARGETS 256
rt_status rt_mesh_morph(const float *v_base, int32_t nv, const float *deltas, int32_t n_targets, const float *weights, float *v_out);
/* Binds a morph set to a mesh: the deltas are copied, the base is taken from the store's current vertices (positions a pose still
 * owes are resolved first), and nv must be the mesh's.  A refused argument is RT_ERR_ARG and nothing changes.  A set already bound
 * is replaced.  rt_scene_set_mesh drops the set; a plain rt_scene_update_mesh_vertices* call keeps it and simply replaces the
 * current positions (the next morph starts from the base again); a plain rt_scene_pose_mesh* call on a mesh with a set bound does
 * what it does without one (it skins the skin's rest pose).  The scene must be idle. */
rt_status rt_scene_set_mesh_morphs(rt_scene *s, int32_t mesh, int32_t n_targets, const float *deltas, int32_t nv);
/* Unbinds it (RT_OK when there is none): the mesh keeps the positions it has, and what the devices held of the set is released. */
rt_status rt_scene_clear_mesh_morphs(rt_scene *s, int32_t mesh);
/* bound: 0 / 1, with n_targets and nv of the set (0 when none is bound).  store_current: as rt_mesh_skin_info's -- 0 while the
 * store's positions are still owed by the mirrors (rt_mesh_morph, then rt_mesh_skin if bones came), which run when the positions
 * are next read.  struct_size must be the caller's sizeof (else RT_ERR_ARG). */
typedef struct rt_mesh_morph_info {
    uint32_t struct_size;
    uint32_t bound;
    int32_t  n_targets, nv;
    uint32_t store_current;
} rt_mesh_morph_info;
rt_status rt_scene_mesh_morph_info(const rt_scene *s, int32_t mesh, rt_mesh_morph_info *out);
/* The morph pose: rt_scene_pose_mesh with the vertices of the definition above, on the same entry path -- the same flags, the same
 * statuses, the same store discipline.  bones == NULL with n_bones == 0 is morph only; bones given is morph, then skin, and a skin
 * must be bound (n_bones the skin's).  On every device that holds the scene the base and the deltas go up once, at the mesh's first
 * morph pose there; a pose uploads the ACTIVE LIST -- (target, weight) of the non-zero weights, ascending, at most 2 KB -- and with
 * bones their 48 bytes each, and launches k_mesh_pose once.  KEEP_PREVIOUS, the root box, the single-leaf mesh and a scene no
 * device holds are as for rt_scene_pose_mesh.  RT_ERR_STATE: no morph set, or bones and no skin; RT_ERR_ARG: n_targets is not the
 * set's, n_bones not the skin's (or not 0 without bones), a weight or a bone that is not finite; nothing changes then. */
rt_status rt_scene_morph_mesh(rt_scene *s, int32_t mesh, const float *weights, int32_t n_targets, const float *bones, int32_t n_bones,
                              uint32_t flags);
/* ... as rt_scene_pose_mesh_auto */
rt_status rt_scene_morph_mesh_auto(rt_scene *s, int32_t mesh, const float *weights, int32_t n_targets, const float *bones, int32_t n_bones,
                                   uint32_t flags, double max_ratio, rt_mesh_quality *out);
/* ... as rt_scene_pose_mesh_build */
rt_status rt_scene_morph_mesh_build(rt_scene *s, int32_t mesh, const float *weights, int32_t n_targets, const float *bones, int32_t n_bones,
                                    uint32_t flags, rt_mesh_build_info *out);
/* ... as rt_scene_pose_mesh_auto_build */
rt_status rt_scene_morph_mesh_auto_build(rt_scene *s, int32_t mesh, const float *weights, int32_t n_targets, const float *bones,
                                         int32_t n_bones, uint32_t flags, double max_ratio, rt_mesh_quality *q, rt_mesh_build_info *out);
/* Milliseconds of the last k_mesh_pose launch for a morph pose (with bones or without) on `device`, by HIP events on the library's stream.  RT_ERR_STATE when that device
 * has run none.  Like a bone pose's it sits inside rt_mesh_update_ms.upload and rt_mesh_build_info.upload_ms. */
rt_status rt_scene_mesh_morph_ms(rt_scene *s, int device, float *ms);

/* ---- host helpers that mirror reference host code --------------------------------------- */
/* cyBVH build with MeanSplit (FIN/include/cyBVH.h:122-142,295-328) as TriObj::Load calls it
 * (maxElementsPerNode = 4, FIN/include/objects.h:143).  nodes_out needs room for 2*nf+1
 * nodes; returns the node count (including the unused node 0) in *nnodes. */
rt_status rt_bvh_build(const float *v, int32_t nv, const uint32_t *f, int32_t nf,
                       int32_t max_per_leaf, rt_bvh_node *nodes_out, int32_t *nnodes,
                       uint32_t *elements_out);
/* PhotonMap::PrepareForIrradianceEstimation (FIN/include/cyPhotonMap.h:196-284):
 * in = photons[1..n] unordered (in[0] unused), out = balanced heap order (out[0] = in[0]).
 * `in` is permuted in place exactly like the reference permutes its vector. */
rt_status rt_photon_balance(rt_photon *in, uint32_t n, rt_photon *out);

/* Which photons of an UNBALANCED array (in[1..n], in[0] as rt_photon_balance takes it) LocatePhotons will never reach once
 * the array is balanced: it descends only while index < halfStoredPhotons = n/2 - 1 (FIN/include/cyPhotonMap.h:217,371), so
 * the last three or four heap slots are never visited.  Found by running BalanceSegment's own partitions along the root
 * paths of those slots only (about 2n element visits); `in` is not modified.  raw_indices (1-based, ascending) needs room
 * for 4; *count receives how many there are. */
rt_status rt_photon_unreachable(const rt_photon *in, uint32_t n, uint32_t *raw_indices, uint32_t cap, uint32_t *count);
/* ABI 4: the same search ON THE DEVICE (what rt_scene_generate_photons runs: the root paths of those heap slots are followed with
 * radix selects, the photons never leave HBM).  *exact = 0 when the key of some median on those paths is not unique in its
 * segment -- then the reference's swap sequence decides which photon lands where, and only rt_photon_unreachable (the host's
 * replay of BalanceSegment, FIN/include/cyPhotonMap.h:222-284) gives the answer; *count is 0 in that case. */
rt_status rt_photon_unreachable_device(int device, const rt_photon *in, uint32_t n, uint32_t *raw_indices, uint32_t cap, uint32_t *count, int32_t *exact);

/* The photon dump generatePhotonMap leaves behind (FIN/main.cpp:397-400: fwrite of
 * Photon[NumPhotons], before balancing) and the way the reference's viewer reads it back
 * (PhotonMap/PhotonMapViz.cpp:172-193: whole 24-byte records, a trailing partial one dropped).
 * photons[0] is unused on both sides, records are photons[1..n].  rt_photons_read_dat with
 * out == NULL only counts. */
rt_status rt_photons_write_dat(const char *path, const rt_photon *photons, uint32_t n);
rt_status rt_photons_read_dat(const char *path, rt_photon *out, uint32_t cap, uint32_t *n);

/* Photon pass on the GPU: generatePhotonMap up to and including ScalePhotonPowers
 * (FIN/main.cpp:350-396; PhotonTracing :439-459; PointLight::RandomPhoton :489-497;
 * MtlBlinn::RandomPhotonBounce FIN/include/materials.h:99-256).  rand() is replaced by a
 * counter-based generator (Philox-4x32-10, key = seed, counter = emission attempt, draw), so the
 * result depends only on (scene, seed).  Emission attempts are consumed in order until at least
 * max_photons are stored (like the reference, the last attempt may overshoot by up to 7).
 * out[0] is unused, out[1..*n_out] are the photons in the reference's 24-byte .dat format, powers
 * already scaled by 4*pi/n; balance them with rt_photon_balance before rt_scene_set_photons. */
rt_status rt_photon_pass(rt_scene *s, int device, uint32_t max_photons, int photon_bounce, uint32_t seed,
                         rt_photon *out, uint32_t out_cap, uint32_t *n_out, uint64_t *attempts_out);

/* The caustic pass of RayTracingProj13 (P13/main.cpp:379-404 + CausticTracing :431-457; a comment block in the
 * committed file): every emitted photon is followed for up to photon_bounce (CAUSTIC_PHOTON_BOUNCE 5)
 * RandomPhotonBounce steps; a hit on a diffuse surface is STORED only after more than one specular hit on
 * the way (hitspec > 1: e.g. into and out of the glass sphere) but COUNTED either way, and emission stops
 * once `max_diffuse_hits` (MAX_NUM_OF_CAUSTIC_PHOTON) are counted.  Same generator, output format and
 * 4*pi/n_stored power scaling as rt_photon_pass.  out needs room for max_diffuse_hits + 9 records. */
rt_status rt_caustic_pass(rt_scene *s, int device, uint32_t max_diffuse_hits, int photon_bounce, uint32_t seed,
                          rt_photon *out, uint32_t out_cap, uint32_t *n_out, uint64_t *attempts_out);

/* ---- render flags (per scene; additive to ABI 4: a caller detects the feature by the presence of the
 *      rt_scene_set_render_flags symbol, RT_ABI_VERSION and the struct sizes are unchanged) ------------------------
 * RT_RENDER_REPRODUCIBLE: every render entry point -- rt_render_begin, rt_render_tiles_device,
 * rt_render_tiles_packed_device, rt_shade_rays and rt_estimate_irradiance -- is a deterministic function of (scene,
 * photon maps, camera, params, tiles).  Promised: byte-identical RGB8, z and count planes (and rt_shade_rays'
 * hit / rgb / z) for identical inputs on the same library build, whatever the tiling, RT_CHUNK_SAMPLES, RT_STREAMS,
 * RT_FRAME_PIPELINE, the rays that overflow k_wavefront's LDS stacks into the global queues, sync or async, job /
 * device / packed path, and (rt_shade_rays) whichever other rays share the call.  Not promised: the same bytes as
 * the default mode (flags 0, whose secondary contributions are float atomics in scheduling order: identical renders
 * agree to the 2e-5 colour gate, an 8-bit channel may move by one level), nor the same bytes across builds.
 * How: every contribution of a sample other than its primary one is added as a 32.32 fixed-point integer (integer
 * adds are associative), and the photon gathers run without their per-cell hints; design, cost and precision: DESIGN.md
 * sections 3 and 4.  The default is 0.  Setting touches no GPU.  Unknown bits: RT_ERR_ARG, flags unchanged.  While an
 * rt_render_begin job on the scene is live: RT_ERR_STATE.  The flags survive scene edits; a render reads them when it
 * is called, so asynchronous renders already enqueued keep the mode they were enqueued with. */
#define RT_RENDER_REPRODUCIBLE 1u
/* RT_RENDER_GENERAL_SHADING (a test hook, not a tuning knob; bit 1 stays unassigned): the lowering of the scene leaves every
 * material's class word clear (rt_scene_material_classes), so the FIN shading kernels run MtlBlinn::Shade in full for every hit
 * instead of leaving out the terms a material class makes exactly +0.  Promised: the same bytes in every plane and the same
 * rt_stats as without the flag -- which is what the flag is there to check, inside one library build.  Changing this bit
 * makes the next use of a device lower the scene again. */
#define RT_RENDER_GENERAL_SHADING 4u
rt_status rt_scene_set_render_flags(rt_scene *s, uint32_t flags);
rt_status rt_scene_get_render_flags(const rt_scene *s, uint32_t *flags);
/* The class word of every material as the lowering sets it (host only: no device, no HIP call): RT_MAT_NO_SPEC_TREE (1) =
 * reflection and refraction are +0.0f in every channel and ior is finite and > 0; RT_MAT_NO_SPECULAR (2) = specular is +0.0f in
 * every channel, it has no texture map and glossiness is finite and in [0, 2^20].  Bit patterns are compared: -0.0f or a NaN
 * leaves the bit clear.  All words are 0 under RT_RENDER_GENERAL_SHADING.  *n_out (may be NULL) = number of materials; out (may
 * be NULL with cap 0) needs room for that many words, else RT_ERR_ARG. */
rt_status rt_scene_material_classes(const rt_scene *s, uint32_t *out, int32_t cap, int32_t *n_out);

/* ---- rendering: replaces BeginRender/StopRender + RenderPixel + RenderImage progress
 *      (FIN/main.cpp:202-344,984-1012; FIN/include/scene.h:586-589) ---------------------- */
/* Asynchronous: returns after the job's worker thread has started.  Output buffers are
 * caller-owned host memory of width*height pixels (rgb8: 3 bytes per pixel) and may be read
 * at any time: finished bands of rows are copied into them chunk by chunk while the job runs
 * (the reference's viewport shows renderImage.GetPixels() as it fills, viewport.cpp:367), and
 * rt_render_progress counts only pixels that have already arrived.  Pixels of tiles this call
 * does not own, and of chunks not reached before rt_render_stop, keep the caller's values.
 * One render at a time per (scene, device): a second one started while the first still runs
 * fails with RT_ERR_STATE (reported by rt_render_wait for jobs); different devices may render
 * the same scene concurrently. */
rt_status rt_render_begin(rt_scene *s, const rt_camera *cam, const rt_params *p,
                          const rt_tile_range *tiles, int device,
                          uint8_t *rgb8, float *z, uint8_t *count, rt_job **out);
/* Same, but the outputs are DEVICE pointers on `device` and the work is enqueued on
 * `hip_stream` (an explicit hipStream_t; NULL = the library's own non-blocking stream, which is NOT
 * ordered with the caller's legacy default stream -- a caller that works on the default stream must
 * render under an explicit stream of its own and pass that); only this call's tiles are written.  Synchronous with respect to enqueueing; completion follows stream
 * order unless `sync` is non-zero.  A ray or photon query dropped by a full queue makes the image
 * wrong: with `sync` != 0 the call then returns RT_ERR_LIMIT (with or without stats_out); after
 * `sync` == 0 calls the verdict is collected by rt_render_check.  While an asynchronous render is
 * still in flight the next call on the same (scene, device) -- on whatever stream -- is ordered
 * behind it on the GPU. */
rt_status rt_render_tiles_device(rt_scene *s, const rt_camera *cam, const rt_params *p,
                                 const rt_tile_range *tiles, int device, void *hip_stream,
                                 uint8_t *rgb8_dev, float *z_dev, uint8_t *count_dev,
                                 int sync, rt_stats *stats_out);
/* Multi-GPU tile exchange (the reference shares one atomic pixel counter between its threads,
 * FIN/main.cpp:71-78).  A rank renders its tiles first, first+stride, ... straight into the buffer it
 * contributes to the all-gather: tile k of the call at packed_dev + k*tile_w*tile_h*8, pixels row-major
 * inside the tile, one 8-byte record per pixel = {r, g, b, z as 4 little-endian bytes, count}; slots of a
 * ragged tile that fall outside the image are zero.  rt_tiles_packed_size gives the bytes / tile count of
 * a call.  rt_tiles_unpack_device turns the gathered buffer of `world` ranks (rank r's block of
 * tiles_per_rank tiles at offset r, its tiles being r, r+world, ...) back into the three RenderImage
 * planes with one small HIP kernel on `hip_stream` (stream-ordered, no host synchronisation). */
rt_status rt_render_tiles_packed_device(rt_scene *s, const rt_camera *cam, const rt_params *p,
                                        const rt_tile_range *tiles, int device, void *hip_stream,
                                        void *packed_dev, uint64_t packed_bytes, int sync, rt_stats *stats_out);
rt_status rt_tiles_packed_size(int32_t width, int32_t height, const rt_tile_range *tiles, uint64_t *bytes, int32_t *n_tiles);
/* (hip_stream == NULL here means the device's legacy null stream, NOT the library's own stream: the call has no scene to
 * take one from; pass the stream the gather ran on.) */
rt_status rt_tiles_unpack_device(int device, void *hip_stream, const void *gathered_dev, int32_t world, int32_t tiles_per_rank,
                                 int32_t width, int32_t height, int32_t tile_w, int32_t tile_h,
                                 uint8_t *rgb8_dev, float *z_dev, uint8_t *count_dev);

/* ---- the linear plane (additive to ABI 4: detected by the presence of the symbols; RT_ABI_VERSION and the structs are
 *      unchanged) -----------------------------------------------------------------------------------------------------
 * An optional fourth output: float rgb_linear[width*height*3], row-major like rgb8, the pixel's colour BEFORE gamma.
 *   - a pixel with n >= 1 hit samples: the float32 average k_resolve computes, c += rgb_j * (1/(float)n) over the hit
 *     samples in sample order, with the same n and batch as the other planes (the first min_sample samples, or all
 *     max_sample for pixels the variance gate sent to the second batch).  On the device
 *     rgb8 == Color24(powf(rgb_linear, (float)(1.0/gamma))) by construction.
 *   - an all-miss pixel: the linear background, background.Sample(x/W, y/H) (FIN/main.cpp:326-328).
 *   - pixels of tiles the call does not own, and of chunks not reached before rt_render_stop, keep the caller's values.
 *   - RT_RENDER_REPRODUCIBLE: byte-identical for identical inputs whatever the chunking, streams, tiling, sync / async and
 *     entry point; in the default mode it inherits the float-atomic last-ulp variation of the samples.
 *   - asking for it changes nothing in the other three planes (under RT_RENDER_REPRODUCIBLE: the same bytes as without).
 * The _linear entry points are the ones above with the plane added; a NULL rgb_linear is RT_ERR_ARG.  Nothing is allocated
 * for the plane unless it is asked for.
 * Packed (_packed_linear_device / rt_tiles_unpack_linear_device): ONE 24-byte record per pixel at packed_dev + 24*q --
 * bytes 0-7 the 8-byte record of rt_render_tiles_packed_device, bytes 8-19 linear r, g, b as little-endian f32, bytes 20-23
 * zero; ragged-tile slots outside the image are all zero.  packed_bytes must be at least 3 x what rt_tiles_packed_size
 * reports. */
rt_status rt_render_begin_linear(rt_scene *s, const rt_camera *cam, const rt_params *p, const rt_tile_range *tiles, int device,
                                 uint8_t *rgb8, float *z, uint8_t *count, float *rgb_linear, rt_job **out);
rt_status rt_render_tiles_linear_device(rt_scene *s, const rt_camera *cam, const rt_params *p, const rt_tile_range *tiles,
                                        int device, void *hip_stream, uint8_t *rgb8_dev, float *z_dev, uint8_t *count_dev,
                                        float *rgb_linear_dev, int sync, rt_stats *stats_out);
rt_status rt_render_tiles_packed_linear_device(rt_scene *s, const rt_camera *cam, const rt_params *p, const rt_tile_range *tiles,
                                               int device, void *hip_stream, void *packed_dev, uint64_t packed_bytes, int sync,
                                               rt_stats *stats_out);
rt_status rt_tiles_unpack_linear_device(int device, void *hip_stream, const void *gathered_dev, int32_t world, int32_t tiles_per_rank,
                                        int32_t width, int32_t height, int32_t tile_w, int32_t tile_h,
                                        uint8_t *rgb8_dev, float *z_dev, uint8_t *count_dev, float *rgb_linear_dev);

/* ---- first-hit feature planes and the plane descriptor (additive to ABI 4: detected by the presence of the symbols;
 *      RT_ABI_VERSION and the structs above are unchanged) ---------------------------------------------------------------
 * What a caller needs AFTER the render: coverage for compositing, normal and albedo as denoising guides, an object id for
 * picking and masking.  All planes are row-major and image-sized like rgb8.  For a pixel let J be the samples its final
 * resolve used (0..min_sample-1, or 0..max_sample-1 when the variance gate sent it to the second batch), H the samples of J
 * whose primary ray hit something, in increasing sample index, n = |H| -- the samples, mask and n the colour is averaged over
 * (RenderPixel averages the hit samples only, FIN/main.cpp:273-338):
 *   normal    float[W*H*3]  sum over H of N_j * (1/n), in float, in sample order; N_j is the world-space normal of the
 *                           primary hit as the tracer returns it (what rt_trace_rays reports); NOT renormalised
 *   albedo    float[W*H*3]  the same average of kd_j: the hit material's diffuse colour times its diffuse map at the hit's
 *                           uvw (diffuse.Sample(uvw), FIN/main.cpp:531); the same definition for every shading model
 *   alpha     float[W*H]    (float)n / (float)|J|
 *   object_id int32[W*H]    the node (index into the scene's node array) of the LAST hit sample -- the sample z is taken
 *                           from, so (z, object_id) describe one surface point
 * An all-miss pixel holds 0, 0, 0 / 0, 0, 0 / 0 / -1.  Only the first hit is described: a mirror shows its own normal, albedo
 * and id.  Pixels of tiles the call does not own, and of chunks not reached before rt_render_stop, keep the caller's values.
 * The feature planes are byte-identical for identical inputs whatever the chunking, streams, tile range and entry point, in
 * the default mode as well as under RT_RENDER_REPRODUCIBLE (one thread sums a pixel's samples in order; no atomics), and
 * asking for them changes nothing in the other planes.  They cost a second trace of the hit primary rays (k_features, once
 * per chunk); nothing is allocated or launched for a plane that is NULL.
 * rt_outputs: struct_size must be sizeof(rt_outputs) of the caller (anything else: RT_ERR_ARG, so the struct can grow);
 * rgb8, z, count are required (NULL: RT_ERR_ARG), every other plane is optional, NULL = not wanted.  With all of them NULL
 * the two entry points are rt_render_begin / rt_render_tiles_device. */
typedef struct rt_outputs {
    uint32_t struct_size;
    uint8_t *rgb8; float *z; uint8_t *count;
    float *rgb_linear;
    float *normal; float *albedo; float *alpha; int32_t *object_id;
} rt_outputs;
rt_status rt_render_begin_outputs(rt_scene *s, const rt_camera *cam, const rt_params *p, const rt_tile_range *tiles, int device,
                                  const rt_outputs *host_planes, rt_job **out);
rt_status rt_render_tiles_outputs_device(rt_scene *s, const rt_camera *cam, const rt_params *p, const rt_tile_range *tiles,
                                         int device, void *hip_stream, const rt_outputs *device_planes, int sync, rt_stats *stats_out);

/* ---- the variance plane (additive to ABI 4: detected by the presence of the symbols; RT_ABI_VERSION and the structs above
 *      are unchanged -- rt_outputs cannot grow, so the plane is an argument of two new entry points, like the linear plane
 *      before it) ---------------------------------------------------------------------------------------------------------
 * variance: float[W*H*3], row-major like rgb_linear: per channel the VARIANCE OF THE MEAN over the samples the colour is
 * averaged over -- the per-pixel error estimate of the linear plane, and the input of the variance-guided denoiser below.
 * With H and n as in the feature-plane section above (the hit samples of the pixel's final batch in increasing sample index):
 *     s1_c = sum over H of (double)x_j,c          s2_c = sum over H of (double)x_j,c * (double)x_j,c      (sample order)
 *     variance_c = n >= 2 ? (float)( max(0, s2_c - s1_c*s1_c/n) / ((double)n * (n-1)) ) : 0
 *   - an all-miss pixel holds 0, and so does a pixel with one hit sample (the denoiser's 3 x 3 prefilter makes that usable).
 *   - pixels of tiles the call does not own, and of chunks not reached before rt_render_stop, keep the caller's values.
 *   - the one-pass double form is deliberate: products of floats are exact in double, the cancellation is harmless for up to
 *     2^16 samples, and the sums ride in the pass of k_resolve that already averages the colour (no second pass over the samples).
 *   - RT_RENDER_REPRODUCIBLE: byte-identical for identical inputs whatever the chunking, streams, tiling, sync / async and
 *     entry point; in the default mode it inherits the float-atomic last-ulp variation of the samples, like the linear plane.
 *   - asking for it changes nothing in any other plane (under RT_RENDER_REPRODUCIBLE: the same bytes as without), and nothing
 *     is allocated or launched for it when it is not asked for.
 * The two entry points are rt_render_begin_outputs / rt_render_tiles_outputs_device with the plane added: the descriptor checks
 * are theirs and come before anything is rendered; a NULL variance is RT_ERR_ARG.  The multi-GPU exchange carries the
 * plane as a section of the packed planes format ("packed planes" below). */
rt_status rt_render_begin_outputs_var(rt_scene *s, const rt_camera *cam, const rt_params *p, const rt_tile_range *tiles, int device,
                                      const rt_outputs *host_planes, float *variance, rt_job **out);
rt_status rt_render_tiles_outputs_var_device(rt_scene *s, const rt_camera *cam, const rt_params *p, const rt_tile_range *tiles,
                                             int device, void *hip_stream, const rt_outputs *device_planes, float *variance_dev,
                                             int sync, rt_stats *stats_out);
/* ---- packed planes: the feature and variance planes in the multi-GPU tile exchange (additive to ABI 4: detected by the
 *      presence of the symbols; RT_ABI_VERSION, the structs and every entry point above are unchanged) ---------------------
 * A rank's contribution to the all-gather stays ONE contiguous buffer, moved by ONE collective: the packed records of
 * rt_render_tiles_packed_device / _packed_linear_device, followed by one SECTION per optional plane.  With
 *     tile_px = tile_w * tile_h     tiles_total = the tile count of the image     per_rank = ceil(tiles_total / stride)
 *     Q = per_rank * tile_px
 * every section has Q slots, slot q being pixel q of the call's tile walk (tile k of the call at k * tile_px, row-major
 * inside the tile) -- the index of the packed records.  The sections, in this order, each present only when its plane is
 * in the mask:
 *     records     24 B per slot with RT_PLANE_LINEAR (the records of _packed_linear_device), 8 B without; always present
 *     normal      12 B per slot    float x 3   (RT_PLANE_NORMAL)
 *     albedo      12 B per slot    float x 3   (RT_PLANE_ALBEDO)
 *     alpha        4 B per slot    float       (RT_PLANE_ALPHA)
 *     object_id    4 B per slot    int32       (RT_PLANE_OBJECT_ID)
 *     variance    12 B per slot    float x 3   (RT_PLANE_VARIANCE)
 * and the contribution is the sum of the sections, rounded up to a multiple of 16 bytes (so that contributions laid end to
 * end keep the alignment of the first; with the usual 32 x 8 tiles nothing is added).  The records section holds the very
 * bytes the existing packed entry points write for the same call; the plane values are those of rt_outputs and of the
 * variance plane above.
 * The sections are sized by per_rank, NOT by the call's own tile count: the ranks of an interleaved frame own
 * ceil(tiles_total / stride) tiles or one fewer, and a collective moves the same number of bytes from every rank.  With
 * sections sized by the call, a short rank's albedo would begin where a full rank's normals still run, and the reader of a
 * gathered buffer would have to know which ranks were short.  Sized by per_rank, the offset of every section depends only on
 * (width, height, tile size, stride, mask), never on `first`: one set of offsets reads every rank's block.
 * Every slot that belongs to no pixel of the call is all zero in every section -- the slots of a ragged tile outside the
 * image, the whole last tile of a rank that is one tile short, the object_id section included (0, not -1) -- and so is the
 * rounding.  The buffer is therefore a pure function of the call's inputs (byte-comparable under RT_RENDER_REPRODUCIBLE).
 * The zeros are written in stream order by every call, not expected from the caller.
 *
 * rt_tiles_packed_planes_size: *bytes (required) is the size of one contribution, *n_tiles (may be NULL) is per_rank -- the
 * tiles_per_rank of the unpack -- and section_offsets (may be NULL) receives the byte offset of the six sections in the
 * order above, UINT64_MAX for an absent one.  Unknown mask bits, a NULL `bytes`, a bad tile range: RT_ERR_ARG.
 * rt_render_tiles_packed_outputs_device: rt_render_tiles_packed_device with the planes of `mask`; packed_bytes must be at
 * least what the size query reports.  A NULL or short buffer and unknown mask bits are RT_ERR_ARG before anything is rendered.
 * With mask 0 or RT_PLANE_LINEAR the records of the call's own tiles are the existing packed call's, to the byte.
 * Stream-ordered; `sync` and stats_out as for rt_render_tiles_packed_device.
 * rt_tiles_unpack_outputs_device: un-interleaves the gathered buffer of `world` ranks (rank r's contribution at
 * r * bytes, each with the sections of (tiles_per_rank, mask)) into image-sized device planes with one HIP kernel on
 * `hip_stream` (NULL: the device's legacy null stream, as for rt_tiles_unpack_device).  device_planes: rgb8, z and count are
 * required as everywhere; every plane in the mask needs a destination (rgb_linear, normal, albedo, alpha, object_id of the
 * descriptor, variance_dev), otherwise RT_ERR_ARG; destinations of planes outside the mask are not touched.  gathered_dev
 * must be 16-byte aligned.  The motion plane needs no transport: it is a function of z and object_id (rt_motion_device) and
 * is computed after the unpack. */
#define RT_PLANE_LINEAR    1u
#define RT_PLANE_NORMAL    2u
#define RT_PLANE_ALBEDO    4u
#define RT_PLANE_ALPHA     8u
#define RT_PLANE_OBJECT_ID 16u
#define RT_PLANE_VARIANCE  32u
rt_status rt_tiles_packed_planes_size(int32_t width, int32_t height, const rt_tile_range *tiles, uint32_t mask,
                                      uint64_t *bytes, int32_t *n_tiles, uint64_t section_offsets[6]);
rt_status rt_render_tiles_packed_outputs_device(rt_scene *s, const rt_camera *cam, const rt_params *p, const rt_tile_range *tiles,
                                                int device, void *hip_stream, void *packed_dev, uint64_t packed_bytes, uint32_t mask,
                                                int sync, rt_stats *stats_out);
rt_status rt_tiles_unpack_outputs_device(int device, void *hip_stream, const void *gathered_dev, int32_t world, int32_t tiles_per_rank,
                                         int32_t width, int32_t height, int32_t tile_w, int32_t tile_h, uint32_t mask,
                                         const rt_outputs *device_planes, float *variance_dev);
/* Waits for the asynchronous renders (sync == 0) issued so far on (scene, device) and returns
 * RT_ERR_LIMIT if any of them dropped rays or photon queries, RT_OK otherwise. */
rt_status rt_render_check(rt_scene *s, int device);
/* ABI 4: the device-side work counters (rays by class, traversal visits, photon queries / photons examined, gather rounds:
 * the uint64 counting fields of rt_stats; its timings, launches and pixels stay zero) accumulated by every render on
 * (scene, device) since they were last cleared -- a render that collects statistics (stats_out, a job) clears them at its
 * start, asynchronous renders only add.  Waits for the renders issued so far.  `reset` != 0 clears them after the read:
 * read-and-reset before a run of asynchronous frames and read again after it to count exactly those frames (bench.py's timed
 * region).  The reference has no counterpart (its only statistic is the wall-clock timer of viewport.cpp:442). */
rt_status rt_render_counters(rt_scene *s, int device, int reset, rt_stats *out);
int       rt_render_progress(rt_job *j);      /* pixels finished so far (monotonic)       */
rt_status rt_render_stop(rt_job *j);          /* cooperative cancel (StopRender)          */
rt_status rt_render_wait(rt_job *j);          /* join; returns the job's final status     */
rt_status rt_job_stats(rt_job *j, rt_stats *out);
/* the photon pass the job ran before rendering (rt_params.photon_count): stage times, all zero when it ran none */
rt_status rt_job_setup_ms(rt_job *j, rt_setup_ms *out);
void      rt_job_destroy(rt_job *j);

/* ---- denoising (additive to ABI 4: detected by the presence of the symbols; RT_ABI_VERSION and the structs above are
 *      unchanged) ---------------------------------------------------------------------------------------------------------
 * An edge-avoiding a-trous wavelet filter (Dammertz, Sewtz, Hanika, Lensch 2010) on albedo-demodulated linear colour: the
 * consumer of the linear plane and of the first-hit planes.  It is an image-space operation on image-sized planes (row-major,
 * W x H like rgb8) and knows nothing of scenes: it serves whatever wrote the planes -- a job, the device entry points, a
 * gathered multi-GPU frame.  The reference has no counterpart.  Definition:
 *   1. A pixel is VALID when object_id >= 0 (id plane given) or z < 1e30 (the render's BIGFLOAT for "nothing hit", no id
 *      plane).  An invalid pixel's output is its input, bit for bit, and it never contributes to another pixel.
 *   2. Demodulate per channel: a_c = albedo_c > 1e-3f ? albedo_c : 1.0f (mirrors and black surfaces have kd = 0), d = rgb_linear / a.
 *   3. Levels i = 0 .. levels-1 with step s = 2^i; taps (dx, dy) in {-2..2}^2, row-major with dy outer, q = p + s * (dx, dy),
 *      1-D kernel h = {1/16, 1/4, 3/8, 1/4, 1/16}.  A tap is skipped when it lies outside the image, is an invalid pixel, has
 *      another id than p (id plane given), or when its weight or colour is not finite.  Otherwise
 *        t = |d_q - d_p|^2 / (sigma_color * 2^-i)^2 + |n_q - n_p|^2 / sigma_normal^2 + ((z_q - z_p) / (sigma_depth * max(z_q, z_p)))^2
 *        w = h[dx+2] * h[dy+2] * exp(-t)            (the centre tap has t = 0)
 *      and d'_p = sum(w * d_q) / sum(w).  Every level reads the previous level's complete output; normals are used as stored.
 *      A pixel whose own colour is not finite passes through (bit for bit, like an invalid one) and contributes nowhere.
 *   4. Remodulate: out_linear = d * a.
 *   5. Optionally out_rgb8 = Color24(powf(out_linear, 1/gamma)), k_resolve's rule: for a pixel the filter left alone, the bytes
 *      k_resolve wrote.  (The exponent is (float)(1.0 / g) with g the double that prints like the float `gamma` to 7 digits:
 *      for gamma = 2.2f that is k_resolve's (float)(1.0 / 2.2).)
 * No atomics and a fixed tap order: the output is byte-identical for identical inputs on one build.  out_linear may be
 * rgb_linear (in place): the input is read completely before anything is written.  No other planes may overlap.
 * rt_denoise_params: levels 1..8; the sigmas positive and finite; gamma positive and finite (used only for out_rgb8).
 * rt_denoise_planes: object_id and out_rgb8 are optional (NULL = not given), the other planes are required.  struct_size must be
 * the caller's sizeof for both structs (anything else: RT_ERR_ARG), so that they can grow.  Arguments are checked before the
 * GPU is touched: w, h <= 0, a levels or sigma out of range, a missing plane are RT_ERR_ARG, more than 2^30 pixels RT_ERR_LIMIT;
 * then, without a gfx950 device: RT_ERR_NO_DEVICE (there is no CPU path).
 * Scratch: 48 bytes per pixel per device, allocated by the first denoise on a device, grown on demand, shared by every later
 * one (calls on one device are ordered on the GPU one behind the other, whatever their streams) and released when the last
 * rt_scene of the process is destroyed -- or with the process. */
typedef struct rt_denoise_params {
    uint32_t struct_size;
    int32_t  levels;            /* 5    */
    float    sigma_color;       /* 1.0  */
    float    sigma_normal;      /* 0.3  */
    float    sigma_depth;       /* 0.05 */
    float    gamma;             /* 2.2  */
} rt_denoise_params;
typedef struct rt_denoise_planes {
    uint32_t struct_size;
    const float *rgb_linear, *normal, *albedo, *z;
    const int32_t *object_id;
    float *out_linear;
    uint8_t *out_rgb8;
} rt_denoise_planes;
void      rt_denoise_default_params(rt_denoise_params *p);
/* The planes are DEVICE pointers on `device`; the kernels are enqueued on `hip_stream` (NULL = the device's legacy null stream,
 * as for rt_tiles_unpack_device) and the call returns without waiting for them unless `sync` is non-zero. */
rt_status rt_denoise_device(int device, void *hip_stream, int32_t w, int32_t h, const rt_denoise_params *p,
                            const rt_denoise_planes *device_planes, int sync);
/* The planes are HOST arrays: upload, denoise, download. */
rt_status rt_denoise(int device, int32_t w, int32_t h, const rt_denoise_params *p, const rt_denoise_planes *host_planes);

/* ---- variance-guided denoising (additive to ABI 4: detected by the presence of the symbols; rt_denoise, rt_denoise_device,
 *      their structs and their output bytes are unchanged) ---------------------------------------------------------------
 * The same filter with a per-pixel colour tolerance: each pixel's own standard error (the variance plane above) instead of the
 * one global sigma_color -- tight where the frame has converged, loose where it is noisy (SVGF's weights, without its temporal
 * part).  Everything of the "denoising" definition above that is not restated here is unchanged: validity, the id rule,
 * pass-through, the tap set and order, h, the normal and depth terms, remodulation and the RGB8 rule.
 *   - Demodulated variance: u_c = variance_c / a_c^2, a the albedo divisor of step 2.  A component of `variance` that is
 *     negative or not finite counts as 0.
 *   - Prefilter, per level and per pixel p: ubar_p,c = sum(g * u_q,c) / sum(g) over the 3 x 3 neighbourhood at UNIT step,
 *     whatever the level, g = {1/4, 1/2, 1/4} in each direction.  The skip rule is the tap's: a neighbour is skipped when it is
 *     outside the image, invalid, or has another id; the centre is always taken.
 *   - Colour term, in place of |d_q - d_p|^2 / (sigma_color * 2^-i)^2:
 *         t_col = sum over c of (d_q,c - d_p,c)^2 / (k_sigma^2 * ubar_p,c + 1e-10)
 *     sigma_color is validated but not used; there is no 2^-i tightening (the variance shrinks instead).  1e-10 only guards
 *     0 / 0, it is not a tuning knob.
 *   - Level output: d'_p = sum(w * d_q) / sum(w) and u'_p,c = sum(w^2 * u_q,c) / sum(w)^2.  Every level reads the previous
 *     level's complete colour and variance.
 *   - out_variance_c = u_c * a_c^2 after the last level; for a pass-through pixel it is the input, bit for bit.
 * No atomics and a fixed tap order: byte-identical for identical inputs on one build.  out_linear may be rgb_linear and
 * out_variance may be `variance`: the inputs are read completely before any level writes.
 * rt_denoise_var: struct_size must be the caller's sizeof (anything else: RT_ERR_ARG); `variance` is required; k_sigma positive
 * and finite.  The checks are rt_denoise's, then these, all before the GPU is touched.  Scratch: 80 bytes per pixel in this mode
 * (the variance rides in a float4 ping-pong pair of its own), in the same per-device allocation, grown on demand. */
typedef struct rt_denoise_var {
    uint32_t struct_size;          /* caller's sizeof, anything else RT_ERR_ARG */
    const float *variance;         /* required: the variance plane (variance of the mean, per channel) */
    float *out_variance;           /* optional: the filtered variance, remodulated; may be `variance` */
    float k_sigma;                 /* 4.0: colour tolerance in standard errors; positive and finite */
} rt_denoise_var;
void      rt_denoise_var_default(rt_denoise_var *v);
/* device planes, like rt_denoise_device */
rt_status rt_denoise_var_device(int device, void *hip_stream, int32_t w, int32_t h, const rt_denoise_params *p,
                                const rt_denoise_planes *device_planes, const rt_denoise_var *v, int sync);
/* host arrays, like rt_denoise: upload, denoise, download */
rt_status rt_denoise_var_host(int device, int32_t w, int32_t h, const rt_denoise_params *p,
                              const rt_denoise_planes *host_planes, const rt_denoise_var *v);

/* ---- temporal accumulation (additive to ABI 4: detected by the presence of the symbols; RT_ABI_VERSION and the structs above
 *      are unchanged) ------------------------------------------------------------------------------------------------------
 * The temporal part the variance-guided filter leaves out: a viewer or a fly-through renders the same STATIC scene frame after
 * frame with independent noise, and an rt_history blends each new frame into what the earlier ones left, reprojected from the
 * camera of the frame it holds into the new one.  Like the denoiser it is an image-space operation on image-sized planes (row-
 * major, W x H) and knows nothing of scenes; rt_temporal reprojects with the camera alone, so only the camera may move between
 * frames -- when nodes move too, rt_motion ("motion vectors" below) says where each pixel was and rt_temporal_motion takes the
 * reprojection from that plane.  The accumulated
 * colour and variance are what rt_denoise_var_* takes as rgb_linear and variance.  The reference has no counterpart.
 * Definition, per pixel p = (x, y) of the new frame:
 *   1. Validity and demodulation are the denoiser's steps 1-2: p is VALID when object_id >= 0 (id plane given) or z < 1e30 (no
 *      id plane); a_c = albedo_c > 1e-3f ? albedo_c : 1.0f; d = rgb_linear / a; u_c = variance_c / a_c^2, where a component of
 *      `variance` that is negative or not finite counts as 0, and u = 0 without a variance plane.  A pixel that is invalid, or
 *      whose colour d is not finite, PASSES THROUGH: out_linear and out_variance are its inputs bit for bit, out_history is 0,
 *      it stores history length 0 and contributes to no later frame.
 *   2. Camera.  With the quantities of the render's camera set-up -- l = focaldist, h = 2 l tan(fov / 2), w = h W / H,
 *      u = w / W, v = -h / H, b = (-w/2 + u/2, h/2 + v/2, -l) (the half-pixel shift included), and the orthonormal rows
 *      x_new = up x (-dir), up, z_new = -dir, M the matrix with these as its columns -- the pixel's representative ray goes
 *      through s(x, y) = (b.x + (x + 0.5) u, b.y + (y + 0.5) v, -l): the centre of the area its Halton-jittered samples
 *      cover.  World point: P = pos + z_p * normalize(M s).  `dof` is ignored: z of a depth-of-field frame is measured from a
 *      point of the lens, so P -- and with it the reprojection -- is off by at most dof.  To have both a lens and an exact
 *      reprojection, render with dof = 0 and defocus the final plane with the stage of "depth of field" below.
 *   3. Reprojection into the STORED camera (primed: the camera of the frame the history holds):
 *      q = (x_new', up', z_new') . (P - pos'); no history if q.z >= 0; s' = q * (-l' / q.z);
 *      fx = (s'.x - b'.x) / u' - 0.5, fy = (s'.y - b'.y) / v' - 0.5; z_exp = |P - pos'|.
 *   4. Bilinear taps: x0 = floor(fx), y0 = floor(fy); the taps (x0 + i, y0 + j) in the order (0,0), (1,0), (0,1), (1,1) with
 *      the weights (1-tx)(1-ty), tx(1-ty), (1-tx)ty, tx ty, tx = fx - x0, ty = fy - y0.  A tap is ACCEPTED when it lies inside
 *      the image, its stored length is N > 0, its stored id equals p's (id plane given; a frame without an id plane stores id 0),
 *      |n_tap - n_p|^2 <= sigma_normal^2 (normals as stored) and |z_tap - z_exp| <= sigma_depth * max(z_tap, z_exp).  W is
 *      the sum of the accepted weights; p HAS A HISTORY iff the rt_history holds a frame, q.z < 0 and W >= 0.01.
 *   5. Blend.  With a history: d_h = sum(w d_tap) / W, u_h = sum(w u_tap) / W, N_h = sum(w N_tap) / W (evaluated as
 *      N_0 + sum(w (N_tap - N_0)) / W with N_0 the first accepted tap's length: taps of equal length give exactly that length);
 *      N = min(N_h + 1, max_history), beta = max(alpha, 1 / N), d' = (1 - beta) d_h + beta d,
 *      u' = (1 - beta)^2 u_h + beta^2 u (u is a variance of the mean: it propagates exactly through the blend of independent
 *      frames).  Without: N = 1, d' = d, u' = u.  Stored for the next frame: d', u', N, z_p, n_p, id_p (0 without an id
 *      plane) per pixel, and the camera.
 *   6. Outputs: out_linear = d' a, out_variance = u' a^2, out_history = N (float), out_rgb8 by step 5 of "denoising"
 *      (Color24(powf(out_linear, 1/gamma)), the same exponent rule).
 * No atomics and a fixed tap order: the outputs are byte-identical for an identical sequence of calls on one build.  out_linear
 * may be rgb_linear and out_variance may be `variance`: a pixel's inputs are read, by the one lane that writes it, before
 * anything of that pixel is written, and the taps read the history only.  No other planes may overlap.
 * rt_history owns the device planes of one W x H stream of frames on one device: two ping-pong sets of three 16-byte records
 * per pixel ({d, z}, {u, N}, {n, id}), 96 bytes a pixel in one allocation, and the camera of the frame it holds.  Calls on one
 * history are ordered on the GPU one behind the other, whatever their streams.  Frames of several histories do not disturb
 * each other.
 * rt_temporal_params: alpha in (0, 1]; max_history 1..65535; sigma_normal, sigma_depth and gamma positive and finite (gamma is
 * used only for out_rgb8).  rt_temporal_planes: rgb_linear, normal, albedo, z and out_linear are required, the others optional
 * (NULL = not given); out_variance needs variance.  struct_size must be the caller's sizeof for both structs.  Everything is
 * checked before the GPU is touched and is RT_ERR_ARG: NULL arguments, a struct_size, a parameter out of range or not finite, a
 * missing plane, out_variance without variance, a NULL history, cam->width or cam->height differing from the history's.
 * rt_history_create: w, h <= 0 or out == NULL is RT_ERR_ARG, more than 2^30 pixels RT_ERR_LIMIT, no gfx950 device
 * RT_ERR_NO_DEVICE (there is no CPU path). */
typedef struct rt_history rt_history;
rt_status rt_history_create(int device, int32_t w, int32_t h, rt_history **out);
/* the next frame starts from nothing; ordered behind the earlier calls on this history */
rt_status rt_history_reset(rt_history *hst);
/* NULL is ignored; waits for the work that still uses it */
void      rt_history_destroy(rt_history *hst);
/* frames accumulated since create / reset (0 for NULL) */
int32_t   rt_history_frames(const rt_history *hst);
typedef struct rt_temporal_params {
    uint32_t struct_size;
    float    alpha;             /* 0.2  : floor of the blend weight, (0, 1]                        */
    int32_t  max_history;       /* 32   : cap of the per-pixel history length, 1..65535            */
    float    sigma_normal;      /* 0.3  : a tap is rejected when |n_tap - n_p|^2 > sigma_normal^2  */
    float    sigma_depth;       /* 0.05 : ... or |z_tap - z_exp| > sigma_depth * max(z_tap, z_exp) */
    float    gamma;             /* 2.2  : out_rgb8 only                                            */
} rt_temporal_params;
typedef struct rt_temporal_planes {
    uint32_t struct_size;
    const float *rgb_linear, *normal, *albedo, *z;
    const int32_t *object_id;   /* optional */
    const float *variance;      /* optional */
    float *out_linear;
    float *out_variance;        /* optional, needs variance */
    float *out_history;         /* optional, float W*H: N_p */
    uint8_t *out_rgb8;          /* optional */
} rt_temporal_planes;
void      rt_temporal_default_params(rt_temporal_params *p);
/* The planes are DEVICE pointers on the history's device; the kernel is enqueued on `hip_stream` (NULL = the device's legacy
 * null stream) and the call returns without waiting for it unless `sync` is non-zero. */
rt_status rt_temporal_device(rt_history *hst, void *hip_stream, const rt_camera *cam, const rt_temporal_params *p,
                             const rt_temporal_planes *device_planes, int sync);
/* The planes are HOST arrays: upload, accumulate, download. */
rt_status rt_temporal(rt_history *hst, const rt_camera *cam, const rt_temporal_params *p, const rt_temporal_planes *host_planes);

/* ---- motion vectors (additive to ABI 4: detected by the presence of the symbols; RT_ABI_VERSION and the structs above are
 *      unchanged) --------------------------------------------------------------------------------------------------------------
 * rt_scene_set_nodes lets a caller move any node between two frames.  Under a fixed camera a moved node's pixels reproject onto
 * themselves, find the same object id and normal and (almost always) an acceptable depth: rt_temporal would blend in history
 * from another surface point.  rt_motion computes, in image space and without tracing a ray, where each pixel's surface point
 * was in the PREVIOUS frame's image; rt_temporal_motion accumulates with that plane in place of its own reprojection.  Only node
 * transforms move here: deforming meshes are followed by rt_scene_motion ("motion vectors for deforming meshes" below), and lights
 * are not followed.  The reference has no counterpart.
 * `motion` is float[W*H*3], row-major: for the pixel p = (x, y) of the new frame (fx, fy, z_exp) -- (fx, fy) the position of p's
 * surface point in the previous frame's image, in the coordinates of step 3 of "temporal accumulation" (an integer coordinate is
 * a pixel centre: fx = x, fy = y means "did not move"), z_exp the expected depth of that point measured from the previous
 * camera.  Definition:
 *   a. World point: step 2 of "temporal accumulation", unchanged: P = pos + z_p * normalize(M s(x, y)) from this frame's camera
 *      (`dof` is ignored, with the same error; "depth of field" below is the way to a lens with exact motion vectors).
 *   b. Node transform.  i = object_id[p]; the ancestor chain of i runs root -> ... -> i through `parent`.  X_obj = TransformTo
 *      down the chain of the CURRENT nodes (per node itm (X - pos), from the root downwards); P_prev = TransformFrom up the chain
 *      of the PREVIOUS nodes (per node tm X + pos, from node i up to the root).  The two chains are composed on the host in
 *      double into one affine map per node, A_i = (R_i, t_i), rounded to float once; a node whose whole chain is bit-identical in
 *      both arrays gets exactly the identity (R = I, t = 0), so a static node's P_prev is P bit for bit.  The kernel evaluates
 *      P_prev = R_i P + t_i, per component ((R_k0 P.x + R_k1 P.y) + R_k2 P.z) + t_k.
 *   c. Step 3 of "temporal accumulation" applied to P_prev with the previous camera (primed): q, fx, fy and
 *      z_exp = |P_prev - pos'|.  (The device code of a. and c. is the one function k_temporal runs.)
 *   d. NO PREVIOUS POSITION: the pixel holds (x, y, 0) when object_id[p] < 0, z_p >= 1e30 or z_p is not finite, i >= n_nodes, or
 *      q.z >= 0.  z_exp <= 0 is the marker.
 *   e. DID NOT MOVE: when A_i is exactly the identity and the two cameras are bit-identical, the pixel holds (x, y, z_p) --
 *      what a.-c. give in exact arithmetic -- provided z_p > 0 (otherwise d. would not be told apart: the steps are run).
 * One lane per pixel, no atomics: the outputs are byte-identical for identical inputs.
 * rt_temporal_motion / rt_temporal_motion_device are rt_temporal / rt_temporal_device with one more argument, the motion plane
 * of this frame (W*H*3 floats; the struct cannot grow).  Steps 2-3 of "temporal accumulation" are replaced by reading
 * (fx, fy, z_exp) of the pixel itself: the pixel has NO HISTORY when z_exp <= 0, when any of the three values is not finite, or
 * when the history holds no frame.  Steps 1, 4, 5 and 6 are unchanged -- the tap order, the (-1, W) x (-1, H) guard on (fx, fy),
 * the id, normal and depth tests, and `cam` stored as the history's camera (a later rt_temporal reprojects from it).  Stored
 * normals are NOT rotated with the object: a node that turns by more than sigma_normal allows between two frames (|n' - n| >
 * sigma_normal, about 17 degrees at 0.3) loses its history for that frame, which is conservative.  A NULL motion plane is
 * RT_ERR_ARG.  rt_temporal and rt_temporal_device are unchanged, to the byte.
 * rt_motion / rt_motion_device: `nodes` and `prev_nodes` are HOST arrays of n_nodes rt_node each (rt_scene_get_nodes' order: the
 * indices the object_id plane holds), consumed before the call returns; prev_nodes == NULL means "nothing moved": every node
 * gets the identity.  Checked before the GPU is touched, RT_ERR_ARG: a NULL cam, prev_cam, nodes or planes; a wrong struct_size;
 * a NULL z, object_id or motion; n_nodes <= 0; in either array a `parent` that is not < its own index or is < -1; a camera of
 * size <= 0, or cameras whose sizes differ from each other.  No gfx950 device is RT_ERR_NO_DEVICE (there is no CPU path).
 * The library keeps the node table of the last call on each device (48 bytes a node) and uploads a call's table only when it
 * differs; calls on one device are therefore ordered on the GPU one behind the other, whatever their streams, like rt_denoise's.
 * The table is released with the denoiser's scratch, when the last rt_scene is destroyed; a process that never creates a scene
 * keeps it until it exits. */
typedef struct rt_motion_planes {
    uint32_t struct_size;
    const float *z;
    const int32_t *object_id;
    float *motion;              /* float W*H*3: (fx, fy, z_exp) */
} rt_motion_planes;
/* The planes are DEVICE pointers on `device`; the kernel is enqueued on `hip_stream` (NULL = the device's legacy null stream)
 * and the call returns without waiting for it unless `sync` is non-zero. */
rt_status rt_motion_device(int device, void *hip_stream, const rt_camera *cam, const rt_camera *prev_cam,
                           const rt_node *nodes, const rt_node *prev_nodes, int32_t n_nodes,
                           const rt_motion_planes *device_planes, int sync);
/* The planes are HOST arrays: upload, compute, download. */
rt_status rt_motion(int device, const rt_camera *cam, const rt_camera *prev_cam, const rt_node *nodes,
                    const rt_node *prev_nodes, int32_t n_nodes, const rt_motion_planes *host_planes);

/* ---- motion vectors for deforming meshes (additive to ABI 4: detected by the presence of the symbols; RT_ABI_VERSION and the
 *      structs above are unchanged) ----------------------------------------------------------------------------------------------
 * "motion vectors" follows node transforms only: a pixel of a mesh whose vertices were moved between two frames
 * (rt_scene_update_mesh_vertices) gets the motion of its node, and under a fixed node and camera that is "did not move".
 * rt_scene_motion is rt_motion for a scene: the same plane, with the pixels of every mesh that holds PREVIOUS POSITIONS
 * (RT_MESH_UPDATE_KEEP_PREVIOUS) followed through the deformation -- the one motion call that traces rays (k_motion_mesh: one lane
 * per pixel, workgroups of 256, the per-lane traversal stack of the tracing kernels).  The current nodes are the scene's; the
 * planes, the cameras and prev_nodes are rt_motion's.  For a pixel p = (x, y) with object id i:
 *   RIGID   node i carries no mesh, or its mesh holds no previous positions: the pixel is exactly what rt_motion writes, to the
 *           byte -- steps a.-e. of "motion vectors", markers and the DID NOT MOVE shortcut included (the same device function).
 *   d. applies unchanged to every pixel: object_id[p] < 0, z_p >= 1e30 or not finite, or i >= n_nodes hold (x, y, 0).
 *   Otherwise, for a MESH pixel:
 *   a'. The ray: the pinhole ray through the pixel centre, o = pos, d = normalize(M s(x, y)) as in step 2 of "temporal
 *       accumulation", taken into the object's coordinates down the chain of the CURRENT nodes as the lowered scene holds them,
 *       the way the renderer takes a ray: per node p' = itm (p - pos), d' = itm ((p + d) - pos) - p', from the root downwards.
 *       The direction is not renormalised, so the ray parameter t is a world distance.
 *   b'. The hit: the closest hit of that ray with the mesh's tree on the device, by the triangle test of `shade_model`, the model
 *       the frame was rendered with (as for rt_trace_rays: RT_SHADE_FIN's two-sided test, or the back-face-culled one of every other
 *       model) -- the slot s of the triangle, its barycentrics bc and the distance t.
 *   c'. The gate: the pixel has NO PREVIOUS POSITION and holds (x, y, 0) when the ray misses the mesh or |t - z_p| >
 *       depth_tol * z_p (one float32 difference against one float32 product).  z_p belongs to a jittered sample: a centre ray that
 *       slips past a silhouette onto a farther layer must not borrow that layer's motion.
 *   d'. The previous point: X'_obj = (bc.x A' + bc.y B') + bc.z C' per component, in this order, without contraction; A', B', C'
 *       the previous positions of the three vertices of slot s's face.  P_prev = F_i X'_obj, F_i the object-to-world map up the
 *       chain of the PREVIOUS nodes (per node tm X + pos, from node i up to the root; the current nodes when prev_nodes is
 *       NULL), composed on the host in double into one affine map per node, rounded to float once -- a second 48-byte table
 *       beside rt_motion's, uploaded only when it differs -- and evaluated per component ((R_k0 X + R_k1 Y) + R_k2 Z) + t_k.
 *   e'. Step c. of "motion vectors" with the previous camera: q, fx, fy and z_exp = |P_prev - pos'|.  q.z >= 0: (x, y, 0).
 * A mesh pixel ALWAYS runs a'.-e'.: there is no DID NOT MOVE shortcut for it (a mesh at rest under a camera at rest comes out
 * as (x, y, t) within rounding, not exactly).  No atomics: the outputs are byte-identical for identical inputs.
 * Checked before the GPU is touched, RT_ERR_ARG: a NULL scene; a shade_model that is no RT_SHADE_*; n_nodes other than the scene's node count; every check of rt_motion
 * (on the scene's nodes and prev_nodes); depth_tol not finite or <= 0 (0.05, sigma_depth's default, is the usual value).  A scene
 * with a live job is RT_ERR_STATE.  The scene is lowered on `device` first if it is not there, with rt_scene_mesh_device_read's
 * discipline (the device is claimed, a pending render waited for).  Calls on one device are ordered one behind the other like
 * rt_motion_device's, with which they share the node table.  A call with sync == 0 may still be reading the lowered scene when
 * it returns: every setter and update that changes the scene on the device waits for it first.
 * rt_motion, rt_motion_device and every rt_temporal_* call are unchanged, to the byte. */
/* The planes are DEVICE pointers on `device`; the kernel is enqueued on `hip_stream` (NULL = the device's legacy null stream)
 * and the call returns without waiting for it unless `sync` is non-zero. */
rt_status rt_scene_motion_device(rt_scene *s, int shade_model, int device, void *hip_stream, const rt_camera *cam, const rt_camera *prev_cam,
                                 const rt_node *prev_nodes, int32_t n_nodes, float depth_tol, const rt_motion_planes *device_planes,
                                 int sync);
/* The planes are HOST arrays: upload, compute, download. */
rt_status rt_scene_motion(rt_scene *s, int shade_model, int device, const rt_camera *cam, const rt_camera *prev_cam, const rt_node *prev_nodes,
                          int32_t n_nodes, float depth_tol, const rt_motion_planes *host_planes);

/* motion_dev: a DEVICE plane on the history's device, read by the kernel (it must stay valid until the call's work is done) */
rt_status rt_temporal_motion_device(rt_history *hst, void *hip_stream, const rt_camera *cam, const rt_temporal_params *p,
                                    const rt_temporal_planes *device_planes, const float *motion_dev, int sync);
/* The planes and `motion` are HOST arrays: upload, accumulate, download. */
rt_status rt_temporal_motion(rt_history *hst, const rt_camera *cam, const rt_temporal_params *p,
                             const rt_temporal_planes *host_planes, const float *motion);

/* ---- history rectification (additive to ABI 4: detected by the presence of the symbols; RT_ABI_VERSION and the structs above
 *      are unchanged) ------------------------------------------------------------------------------------------------------
 * "temporal accumulation" accepts a history tap on geometry alone (id, normal, depth): it is right only while the light a surface
 * point sends to the camera does not change.  A light that moves or changes, what is seen IN a mirror or a glass surface under a
 * moving camera, and a moving node's shadow on a static receiver all pass every geometric test and fade out at (1 - alpha)^k.
 * rt_temporal_clip_* are rt_temporal / rt_temporal_motion with one more step between steps 4 and 5: the reprojected history
 * colour is clamped into a box built from the CURRENT frame's neighbourhood (variance clipping), and a pixel whose history had to
 * be clamped keeps only a short history length.  The reference has no counterpart.  Definition:
 *   4b. For a pixel p = (x, y) that HAS A HISTORY (step 4), with r = radius:
 *      Window pixels: the q with |qx - x| <= r and |qy - y| <= r.  A window pixel COUNTS when it lies inside the image, is VALID
 *      (step 1), its demodulated colour d_q (step 1) is finite, and id_q == id_p; without an id plane every valid pixel with a
 *      finite d_q counts.  p itself always counts (it has a history, so it is valid and finite).
 *      Order: the window is visited row-major -- qy from y - r to y + r, inside a row qx from x - r to x + r -- and the pixels that
 *      count are summed in that order, in float, in two passes: m = their number, mu_c = (sum d_q,c) / m, then
 *      s2_c = (sum (d_q,c - mu_c)^2) / m (the mean first; never E[x^2] - mu^2).
 *      m < min_count: the step does nothing (the pixel is KEPT).
 *      Otherwise e_c = k_clip * sqrt(s2_c), lo_c = mu_c - e_c, hi_c = mu_c + e_c and d_h,c := min(max(d_h,c, lo_c), hi_c)
 *      (fmaxf / fminf: a bound that is NaN -- sums that overflowed -- does not clamp).  p is CLIPPED iff that changed any
 *      channel; for a clipped pixel N_h := min(N_h, clip_history) before N = min(N_h + 1, max_history).
 *      u_h is left as it is.  The blend's variance u' = (1 - beta)^2 u_h + beta^2 u is then an APPROXIMATION for a clipped
 *      pixel: the clamped history is a function of the current frame and no longer independent of it, and a clamp towards
 *      the frame's own neighbourhood also changes the history's spread.  (The shortened N raises beta, so u' leans on the
 *      frame's own u, which is exact.)
 *   Everything else -- pass-through, the taps, the blend, the outputs and what is stored -- is steps 1-6 unchanged, with the
 *   clamped d_h and the shortened N_h in step 5.  With a box so wide that nothing is clamped (k_clip = 1e9 on a noisy frame) the
 *   outputs are those of rt_temporal / rt_temporal_motion to the byte.
 * One more optional output, out_clipped (float W*H): 0 the pixel has no history (pass-through pixels included), 1 it has one and
 * it was kept (also when m < min_count), 2 it was clipped.  rt_temporal_planes cannot grow, so the pointer travels in
 * rt_temporal_clip, next to the parameters it reports on: a device plane for rt_temporal_clip_device, a host array for
 * rt_temporal_clip_host, NULL = not wanted.  It may overlap no other plane.
 * Rectification BOUNDS the error a changed light leaves in the history by the box; it does not track the light.  A stale value
 * inside k_clip sigma of a noisy neighbourhood survives and fades at the blend's rate as before.
 * out_linear may still be rgb_linear and out_variance `variance`.  The kernel reads the neighbours' rgb_linear, so for
 * out_linear overlapping rgb_linear the library lets it write a plane the history owns (12 bytes a pixel, allocated by the first
 * such call) and copies it to out_linear on the same stream; the bytes are those of the call with separate planes.  The costs:
 * every such call -- rt_temporal_clip_host always, rt_temporal_clip_device in place -- pays that 12 B a pixel copy, the history
 * keeps the plane until it is destroyed, and the FIRST such call on a history allocates device memory although it only
 * enqueues (sync = 0): it must not be made while its stream is being captured into a graph.  With separate planes there is
 * neither copy nor allocation.
 * No atomics, a fixed window order, a fixed tap order: byte-identical outputs for an identical sequence of calls on one build.
 * Checked before the GPU is touched, RT_ERR_ARG: a NULL clip, a struct_size that is not the caller's sizeof, radius outside
 * 1..3, k_clip not positive and finite, min_count < 1, clip_history outside 1..65535 -- and every check of rt_temporal.  motion /
 * motion_dev NULL: reproject with the cameras (rt_temporal); otherwise this frame's motion plane (rt_temporal_motion).  Calls
 * with and without rectification may be mixed freely on one history. */
typedef struct rt_temporal_clip {
    uint32_t struct_size;
    int32_t  radius;        /* 2   : window (2r+1)^2, 1..3                                  */
    float    k_clip;        /* 1.5 : half-width of the box in standard deviations, > 0      */
    int32_t  min_count;     /* 4   : fewer window pixels than this -> no rectification, >=1 */
    int32_t  clip_history;  /* 2   : N_h of a clipped pixel is at most this, 1..65535       */
    float   *out_clipped;   /* NULL: optional output, float W*H: 0 no history, 1 kept, 2 clipped */
} rt_temporal_clip;
void      rt_temporal_clip_default(rt_temporal_clip *c);
rt_status rt_temporal_clip_device(rt_history *hst, void *hip_stream, const rt_camera *cam, const rt_temporal_params *p,
                                  const rt_temporal_clip *clip, const rt_temporal_planes *device_planes,
                                  const float *motion_dev /* NULL: reproject with the cameras */, int sync);
rt_status rt_temporal_clip_host(rt_history *hst, const rt_camera *cam, const rt_temporal_params *p, const rt_temporal_clip *clip,
                                const rt_temporal_planes *host_planes, const float *motion /* NULL allowed */);

/* ---- exposure and tone mapping (additive to ABI 4: detected by the presence of the symbols; RT_ABI_VERSION and the structs
 *      above are unchanged) -------------------------------------------------------------------------------------------------
 * The last stage of the image-space pipeline: every stage above ends in Color24(powf(out_linear, 1/gamma)), the reference's hard
 * clamp at a white level of 1.0.  This one meters the frame, adapts an exposure from frame to frame, applies a tone curve and
 * encodes -- on image-sized planes (row-major, W x H), without a host round trip.  The reference has no counterpart.  Definition:
 *   1. Luminance.  Y = ((0.2126f * r) + (0.7152f * g)) + (0.0722f * b), every product and every sum rounded to float on its own
 *      (no fused multiply-add): Y, and with it the histogram, is an exact function of the input bits.
 *   2. Metered pixels and bins.  A pixel is METERED when (no id plane is given or object_id >= 0) and Y is finite and
 *      Y >= 2^-16.  256 bins, eight per octave over 2^-16 .. 2^16, read off the bit pattern:
 *      bin = min(255, (float_as_uint(Y) >> 20) - 888), 888 = (127 - 16) * 8.  The bin's log2 value is
 *      L_b = (2 bin + 1) / 16 - 16, the piecewise-linear log2 of the bin's centre.
 *   3. Metering, in integers.  n = number of metered pixels; lo = floor((double)p_low * n), hi = ceil((double)p_high * n), so
 *      that lo < hi <= n whenever n > 0 (hi is lo + 1 should the two roundings ever meet).  With the samples in bin order the
 *      ranks [lo, hi) count: bin b, with c_b samples below it and h_b in it, contributes
 *      k_b = max(0, min(c_b + h_b, hi) - max(c_b, lo)); S = sum(k_b * (2 b + 1)) as a 64-bit integer;
 *      Lbar = S / (16 * (hi - lo)) - 16 in double.  Integer sums are associative: the histogram and Lbar do not depend on the
 *      order in which workgroups or atomics arrive.
 *   4. Target.  E_t = clamp(log2(key) + ev_bias - Lbar, ev_min, ev_max), log2(key) taken on the host in double.  n == 0 (nothing
 *      metered): E stays what it was -- with no metered frame since create / reset, E = clamp(ev_bias, ev_min, ev_max), and the
 *      next metered frame still counts as the first; log2_metered keeps its last value.  auto_exposure == 0: no metering, no
 *      state, E = ev_bias (not clamped).
 *   5. Adaptation.  The first metered frame after create / reset: E = E_t.  Otherwise E = E_prev + a * (E_t - E_prev), a =
 *      adapt_up if E_t > E_prev, else adapt_down, in double.  E is stored as float; scale = (float)exp2((double)E).
 *   6. Apply, per pixel: x = rgb_linear * scale, then
 *        RT_TONEMAP_CLAMP     y = x
 *        RT_TONEMAP_REINHARD  Yx = the luminance of x by step 1; y = x when !(Yx > 0), else y = x * f,
 *                             f = (1 + Yx / white^2) / (1 + Yx) (white^2 rounded to float once)
 *        RT_TONEMAP_ACES      per channel y = clamp((x (2.51f x + 0.03f)) / (x (2.43f x + 0.59f) + 0.14f), 0, 1); a NaN stays NaN
 *      in float, every operation rounded on its own.  out_display = y (float, optional, may be rgb_linear);
 *      out_rgb8 = Color24(powf(y, 1/gamma)) by step 5 of "denoising", its exponent rule included.  At least one of the two.
 * Byte-identical outputs, histogram and exposure for an identical sequence of calls on one build.  out_display may be
 * rgb_linear: the frame is metered before anything is written and a pixel is read, by the one lane that writes it, before it is
 * written.  No other planes may overlap.
 * rt_exposure is one per stream of frames on one device and is not tied to an image size.  On the device it holds the 256-bin
 * working histogram, a copy of the last metered frame's, E, scale, Lbar, n and whether it holds a metered frame.  Calls on one
 * state are ordered on the GPU one behind the other, whatever their streams; two states share nothing.  The device entry point
 * never waits for the GPU unless `sync` is set: k_tonemap loads scale from the state.
 * Everything is checked before the GPU is touched and is RT_ERR_ARG: NULL params or planes, a struct_size that is not the
 * caller's sizeof, w or h <= 0, an unknown operator, key / white / gamma not positive and finite, ev_bias / ev_min / ev_max not
 * finite or ev_min > ev_max, not 0 <= p_low < p_high <= 1, adapt_up / adapt_down outside (0, 1], a NULL rgb_linear, no output
 * plane, a NULL state with auto_exposure != 0, a `device` that is not the state's.  More than 2^30 pixels: RT_ERR_LIMIT.  Then,
 * without a gfx950 device: RT_ERR_NO_DEVICE (there is no CPU path). */
enum { RT_TONEMAP_CLAMP = 0, RT_TONEMAP_REINHARD = 1, RT_TONEMAP_ACES = 2 };
typedef struct rt_exposure rt_exposure;
/* out == NULL: RT_ERR_ARG; no gfx950 device: RT_ERR_NO_DEVICE */
rt_status rt_exposure_create(int device, rt_exposure **out);
/* the next metered frame is the first again; ordered behind the earlier calls on this state */
rt_status rt_exposure_reset(rt_exposure *e);
/* NULL is ignored; waits for the work that still uses it */
void      rt_exposure_destroy(rt_exposure *e);
/* Waits for the calls issued on the state, then what the last METERED call (auto_exposure != 0) left: E (log2 of its scale), n,
 * and Lbar of the last frame that metered anything.  A call with auto_exposure == 0 does not touch the state.  Any pointer may be NULL */
rt_status rt_exposure_get(rt_exposure *e, float *log2_exposure, double *log2_metered, uint32_t *metered_pixels);
/* Waits likewise; the histogram of the last frame that went through the meter (all zero before the first) */
rt_status rt_exposure_histogram(rt_exposure *e, uint32_t out[256]);
typedef struct rt_tonemap_params {
    uint32_t struct_size;
    int32_t  op;                /* RT_TONEMAP_ACES */
    int32_t  auto_exposure;     /* 1    : 0 = fixed exposure ev_bias, no state needed      */
    float    key;               /* 0.18 : the luminance the metered mean is brought to      */
    float    ev_bias;           /* 0    : added to the exposure, in stops                   */
    float    ev_min, ev_max;    /* -16, 16 : the range of the target                        */
    float    p_low, p_high;     /* 0.10, 0.90 : the percentile window of the meter          */
    float    adapt_up, adapt_down;  /* 1, 1 : fraction of the way to the target per frame, (0, 1] */
    float    white;             /* 4    : REINHARD's white point                            */
    float    gamma;             /* 2.2  : out_rgb8 only                                     */
} rt_tonemap_params;
typedef struct rt_tonemap_planes {
    uint32_t struct_size;
    const float *rgb_linear;
    const int32_t *object_id;   /* optional: pixels with id < 0 are not metered */
    float *out_display;         /* optional, may be rgb_linear */
    uint8_t *out_rgb8;          /* optional */
} rt_tonemap_planes;
void      rt_tonemap_default_params(rt_tonemap_params *p);
/* The planes are DEVICE pointers on `device`; the kernels are enqueued on `hip_stream` (NULL = the device's legacy null stream)
 * and the call returns without waiting for them unless `sync` is non-zero.  e may be NULL only with auto_exposure == 0. */
rt_status rt_tonemap_device(rt_exposure *e, int device, void *hip_stream, int32_t w, int32_t h, const rt_tonemap_params *p,
                            const rt_tonemap_planes *device_planes, int sync);
/* The planes are HOST arrays: upload, tone-map, download. */
rt_status rt_tonemap(rt_exposure *e, int device, int32_t w, int32_t h, const rt_tonemap_params *p, const rt_tonemap_planes *host_planes);

/* ---- bloom (additive to ABI 4: detected by the presence of the symbols; RT_ABI_VERSION and the structs above are unchanged) ----
 * The stage ahead of "exposure and tone mapping": after the tone curve a light 50 times over white and one twice over white are
 * the same flat patch.  Bloom spreads the energy above the display range into the neighbourhood BEFORE the curve, so that
 * brightness stays visible as extent.  A linear float RGB plane (row-major, W x H x 3) in, one out; the reference has no
 * counterpart.  Definition, in float, every operation rounded on its own (no fused multiply-add):
 *   1. Exposure.  The threshold is relative to `scale`: scale = (float)exp2((double)exposure_ev) when no rt_exposure is passed
 *      or the one passed holds no metered frame (since create / reset); otherwise the scale the state holds at that point of the
 *      stream -- the PREVIOUS frame's when the frame's own rt_tonemap follows.  The kernel loads it from the state (as k_tonemap
 *      does): the device entry never waits.  The stage does not meter and does not write the state.
 *   2. Bright pass, per source pixel.  c = the pixel with every channel that is not finite or is negative replaced by 0.
 *      Y = the luminance of c by step 1 of "exposure and tone mapping"; Ys = scale * Y.  With t = threshold, k = knee * t (rounded to float once):
 *        x = min(max((Ys - t) + k, 0), 2 k);  s = (x * x) / (4 k + 1e-5f);  wgt = max(s, Ys - t) / max(Ys, 1e-5f)
 *      (the soft knee: 0 up to Ys = t - k, quadratic up to t + k, Ys - t above; never more than 1).  threshold == 0: wgt = 1 for
 *      every pixel.  Ys not finite (an overflow of scale * Y): wgt = 1.  The pixel contributes P = c * wgt per channel -- in
 *      scene-linear units, not multiplied by scale.
 *   3. Pyramid.  Level 0 is W_0 x H_0 = ceil(W / 2) x ceil(H / 2), level l + 1 is ceil(W_l / 2) x ceil(H_l / 2).  L = min(levels,
 *      1 + the number of halvings that take level 0 to 1 x 1): no level is computed from a 1 x 1 level.  Downsample (level 0
 *      from P, level l + 1 from level l): texel (i, j) is the separable 4-tap [1 3 3 1] / 8 over the source texels 2i-1 .. 2i+2
 *      by 2j-1 .. 2j+2, indices clamped to the source's edge.  With f(a, b, c, d) = ((a + 3 b) + (3 c + d)) * 0.125f: the four
 *      rows first, r_m = f(the row's four texels, left to right), then B = f(r_0, r_1, r_2, r_3), top to bottom.
 *      Upsample up(X) of a level X (w x h) at a texel (x, y) of the next finer grid: per axis the near coarse index is x >> 1,
 *      the far one x >> 1 + 1 when x is odd and x >> 1 - 1 when it is even, the far one clamped to 0 .. w-1; with
 *      g(n, f) = 0.75f * n + 0.25f * f: the near row and the far row first, each g(near column, far column), then
 *      g(near row's, far row's).  Every weight is non-negative and the weights of one output texel sum to 1, at edges and odd
 *      sizes too (a clamped index only moves weight onto the edge texel).
 *   4. Recombination, from the coarsest level up: U_{L-1} = B_{L-1}; U_l = a * B_l + spread * up(U_{l+1}), a = 1 - spread
 *      rounded to float once.  A lerp, not a sum: a partition of unity whatever L is.
 *   5. Output.  out = rgb + intensity * up(U_0), with the ORIGINAL pixel: a NaN pixel stays NaN and changes no other pixel.
 *      out_bloom (optional) = up(U_0) alone.  A lane reads its own pixel before it writes it: out may be rgb_linear.  No other
 *      planes may overlap.
 *   6. No atomics, fixed orders: byte-identical outputs for identical inputs on one build.  A constant frame c with threshold 0
 *      gives c (1 + intensity) to rounding; a frame wholly below Ys = t - k comes back bit for bit (finite, no -0).
 *   Sums that overflow float (pixels near FLT_MAX) are outside the definition.
 * rt_bloom owns the pyramid of one W x H stream of frames on one device (16 bytes per source pixel at most), so the device entry
 * never allocates.  Calls on one rt_bloom are ordered on the GPU one behind the other, whatever their streams; a call that is
 * given an rt_exposure is also ordered behind the earlier calls on that state, and the state's later calls behind it.
 * Everything is checked before the GPU is touched and is RT_ERR_ARG: NULL arguments, a struct_size that is not the caller's
 * sizeof, w or h <= 0, threshold / knee / intensity / spread not finite or negative, spread > 1, knee > 1, levels < 1,
 * exposure_ev not finite, an rt_exposure on another device than the rt_bloom, a NULL rgb_linear, no output plane, planes that
 * overlap other than out == rgb_linear.  More than 2^30 pixels: RT_ERR_LIMIT.  Then, without a gfx950 device:
 * RT_ERR_NO_DEVICE (there is no CPU path). */
typedef struct rt_bloom rt_bloom;
typedef struct rt_bloom_params {
    uint32_t struct_size;
    float    threshold;         /* 1    : bright-pass threshold, relative to scale: display white        */
    float    knee;              /* 0.5  : soft-knee width as a fraction of threshold, 0..1               */
    float    intensity;         /* 0.25 : weight of the bloom plane in the output                        */
    float    spread;            /* 0.7  : lerp weight towards the coarser level in the recombination, 0..1 */
    int32_t  levels;            /* 6    : pyramid levels requested, >= 1 (clipped to what the size allows) */
    float    exposure_ev;       /* 0    : fixed exposure, in stops, when no metered state applies        */
} rt_bloom_params;
typedef struct rt_bloom_planes {
    uint32_t struct_size;
    const float *rgb_linear;
    float *out;                 /* optional, may be rgb_linear */
    float *out_bloom;           /* optional: up(U_0) alone     */
} rt_bloom_planes;
/* w, h <= 0 or out == NULL: RT_ERR_ARG; more than 2^30 pixels: RT_ERR_LIMIT; no gfx950 device: RT_ERR_NO_DEVICE */
rt_status rt_bloom_create(int device, int32_t w, int32_t h, rt_bloom **out);
/* NULL is ignored; waits for the work that still uses it */
void      rt_bloom_destroy(rt_bloom *b);
void      rt_bloom_default_params(rt_bloom_params *p);
/* DIAGNOSTIC ONLY, for tests and timing tools; nothing a caller needs.  What a call on a w x h frame runs, without a device:
 * *levels_used = L of step 3; *tail_level = -1 in the shipped build (every level is a launch of its own), and in a build with
 * k_bloom_tail (RT_BLOOM_TAIL=1) the level from which its one workgroup runs the rest of the pyramid inside LDS, -1 when no
 * level is left to it.  tail_level says how a build schedules its launches, never what it computes. */
rt_status rt_bloom_plan(int32_t w, int32_t h, int32_t levels, int32_t *levels_used, int32_t *tail_level);
/* The planes are DEVICE pointers on the rt_bloom's device; the kernels are enqueued on `hip_stream` (NULL = the device's legacy
 * null stream) and the call returns without waiting for them unless `sync` is non-zero.  e may be NULL. */
rt_status rt_bloom_device(rt_bloom *b, rt_exposure *e, void *hip_stream, const rt_bloom_params *p,
                          const rt_bloom_planes *device_planes, int sync);
/* The planes are HOST arrays: upload, run, download. */
rt_status rt_bloom_host(rt_bloom *b, rt_exposure *e, const rt_bloom_params *p, const rt_bloom_planes *host_planes);

/* ---- motion blur (additive to ABI 4: detected by the presence of the symbols; RT_ABI_VERSION and the structs above are unchanged) ----
 * The stage between the denoise and "bloom": every frame is an instantaneous shutter, so a fast node strobes from frame to frame, and
 * temporal accumulation rejects exactly that history.  Motion blur stands in for the open shutter, in image space, from planes the
 * chain already has (after McGuire et al. 2012, "A reconstruction filter for plausible motion blur"): tile-max velocity,
 * neighbour-max velocity and a depth-aware gather along the dominant velocity.  The reference has no counterpart.
 * Inputs, all row-major and W x H: rgb_linear (float x 3), motion (float x 3, the plane of "motion vectors": (fx, fy, z_exp)) and z
 * (float, this frame's depth).  Parameters: shutter, max_blur (K), samples (N), depth_extent.  Definition, in float, every operation
 * rounded on its own (no fused multiply-add); sqrtf and the divisions are the correctly rounded ones:
 *   1. Velocity of the pixel p = (x, y): v = (h * ((float)x - fx), h * ((float)y - fy)) with h = 0.5f * shutter rounded once: the blur
 *      is shutter times the displacement long and centred on p.  v = (0, 0) when z_exp <= 0 or one of fx, fy, z_exp is not finite
 *      (the markers of "no previous position").  m = vx * vx + vy * vy.
 *   2. Tile max.  K x K tiles from (0, 0), partial ones at the right and bottom: TX = ceil(W / K) by TY = ceil(H / K).  A tile's
 *      value is the v of its pixel with the largest m; among equal m the lowest row-major pixel index wins.  Only m is compared:
 *      no sqrt, and (max m, then min index) is associative, so any reduction order gives the same bits.
 *   3. Neighbour max.  Per tile, the tile-max value with the largest m (taken again from the stored v) over the 3 x 3 tiles around
 *      it; tiles outside the grid are skipped; among equal m the first in row-major order of the 3 x 3.  This is vn, UNCLAMPED.
 *   4. Clamp, applied only where a velocity is used, never before a selection: clampK(v) = v when m <= K * K, else
 *      v * (K / sqrtf(m)) per component; its length is lenK(m) = min(sqrtf(m), (float)K).
 *   5. Early out.  vn's m < 0.25f (half a pixel): out[p] = rgb[p] bit for bit -- a static frame comes back byte-identical.
 *   6. Gather, otherwise.  c = clampK(vn), L = lenK(vn's m), lp = max(lenK(m of p), 0.5f).  rgb[p] with a channel that is not
 *      finite: out[p] = rgb[p].  Else N taps i = 0 .. N-1, in this order:
 *        j = {0, 2, 3, 1}[(y & 1) * 2 + (x & 1)];  a_i = (float)i + (0.125f + 0.25f * j);  t_i = a_i * g - 1 with g = 2 / N rounded once;
 *        q = ((float)x + t_i * c.x, (float)y + t_i * c.y);  the tap pixel s = (floorf(q.x + 0.5f), floorf(q.y + 0.5f)).
 *      A tap outside the image, or with a colour channel that is not finite, has weight 0.  Otherwise, with d = |t_i| * L,
 *      ls = max(lenK(m of s), 0.5f), and every z that is not finite or is >= 1e30 counted as 1e30f:
 *        cone(d, l) = min(max(1 - d / l, 0), 1)
 *        cyl(d, l)  = 1 - (u * u) * (3 - 2 * u),  u = min(max((d - 0.95f * l) / (1.05f * l - 0.95f * l), 0), 1)
 *        near(a, b) = min(max(1 - (a - b) / e, 0), 1),  e = depth_extent * max(min(a, b), 1e-6f)
 *        w_i = (near(z_s, z_p) * cone(d, ls) + near(z_p, z_s) * cone(d, lp)) + 2 * (cyl(d, ls) * cyl(d, lp))
 *      The centre: w_p = 1 / lp on rgb[p].  Per channel, sums from the centre term on, taps in order:
 *        out[p] = (w_p * rgb[p] + sum w_i * rgb[s_i]) / (w_p + sum w_i)
 *      Every l is at least 0.5 and w_p at least 1 / K, so no NaN arises from finite colours.
 *   7. No atomics, fixed orders: byte-identical outputs for identical inputs on one build.  The weights are normalised: a frame
 *      of one colour keeps it to rounding whatever the motion.  out must NOT be rgb_linear (the gather reads neighbours), and no
 *      two planes may overlap.  Products that overflow float (colours near FLT_MAX) are outside the definition.
 * rt_motion_blur owns the two tile planes of one W x H stream of frames on one device, sized for the smallest K, so the device entry
 * never allocates.  Calls on one rt_motion_blur are ordered on the GPU one behind the other, whatever their streams.
 * Everything is checked before the GPU is touched and is RT_ERR_ARG: NULL arguments, a struct_size that is not the caller's sizeof,
 * w or h <= 0, shutter not finite, negative or > 2, max_blur outside 2..32, samples outside 3..63 or even, depth_extent not finite
 * or < 1e-3, a NULL rgb_linear, motion, z or out, planes that overlap.  More than 2^30 pixels: RT_ERR_LIMIT.  Then, without a
 * gfx950 device: RT_ERR_NO_DEVICE (there is no CPU path). */
typedef struct rt_motion_blur rt_motion_blur;
typedef struct rt_motion_blur_params {
    uint32_t struct_size;
    float    shutter;           /* 0.5  : the fraction of the frame interval the shutter is open, 0..2      */
    int32_t  max_blur;          /* 16   : K, the tile size and the longest half-extent of a blur in pixels, 2..32 */
    int32_t  samples;           /* 15   : N, taps per pixel, odd, 3..63                                     */
    float    depth_extent;      /* 0.05 : the relative depth difference over which near() falls from 1 to 0 */
} rt_motion_blur_params;
typedef struct rt_motion_blur_planes {
    uint32_t struct_size;
    const float *rgb_linear;
    const float *motion;
    const float *z;
    float *out;                 /* not rgb_linear */
    float *out_tiles;           /* optional: float TX*TY*2, the UNCLAMPED neighbour-max vector of each tile */
} rt_motion_blur_planes;
/* w, h <= 0 or out == NULL: RT_ERR_ARG; more than 2^30 pixels: RT_ERR_LIMIT; no gfx950 device: RT_ERR_NO_DEVICE */
rt_status rt_motion_blur_create(int device, int32_t w, int32_t h, rt_motion_blur **out);
/* NULL is ignored; waits for the work that still uses it */
void      rt_motion_blur_destroy(rt_motion_blur *mb);
void      rt_motion_blur_default_params(rt_motion_blur_params *p);
/* DIAGNOSTIC, needs no device: the tile grid of step 2, *tx = TX and *ty = TY (either may be NULL) */
rt_status rt_motion_blur_tiles(int32_t w, int32_t h, int32_t max_blur, int32_t *tx, int32_t *ty);
/* The planes are DEVICE pointers on the rt_motion_blur's device; the kernels are enqueued on `hip_stream` (NULL = the device's
 * legacy null stream) and the call returns without waiting for them unless `sync` is non-zero. */
rt_status rt_motion_blur_device(rt_motion_blur *mb, void *hip_stream, const rt_motion_blur_params *p,
                                const rt_motion_blur_planes *device_planes, int sync);
/* The planes are HOST arrays: upload, run, download. */
rt_status rt_motion_blur_host(rt_motion_blur *mb, const rt_motion_blur_params *p, const rt_motion_blur_planes *host_planes);

/* ---- depth of field (additive to ABI 4: detected by the presence of the symbols; RT_ABI_VERSION and the structs above are unchanged) ----
 * The stage between the denoise / temporal accumulation and "motion blur": the lens, in image space.  rt_camera.dof rendered as a
 * lens (a disk of radius dof at the camera position, focused at focaldist) is the noisiest part of a 4 spp frame, smears the
 * first-hit planes every other stage uses as guides, and moves the point z is measured from.  Rendered pinhole (dof = 0) and
 * defocused here from the exact z plane, the chain keeps crisp guides and an exact reprojection.  The circle of confusion is the
 * renderer's own lens model, so the result is comparable with a lens render.  The reference has no counterpart.
 * Inputs, row-major and W x H: rgb_linear (float x 3), z (float, the render's depth plane: distance along the pixel's ray, >= 1e30 =
 * nothing hit) and the frame's rt_camera, of which only fov, focaldist, dof, width and height are used.  Parameters: max_coc (K),
 * samples (N), depth_extent, aperture_scale, focus.  Definition, in float, every operation rounded on its own (no fused multiply-
 * add); sqrtf and the divisions are the correctly rounded ones; no transcendental function runs on the device:
 *   0. Host set-up.  fd = focus, or focaldist when focus is 0, as a float; in double, from the floats widened,
 *      A = (aperture_scale * |dof| * H) / (2 * fd * tan(fov / 2 * (pi / 180))), rounded to float once: the radius in pixels of a
 *      point at infinity.  l, u, v, b are the camera quantities of "temporal accumulation" step 2 (l = focaldist there: cos(theta)
 *      below does not depend on it).
 *   1. Circle of confusion of the pixel p = (x, y): sx = b.x + ((float)x + 0.5f) * u, sy = b.y + ((float)y + 0.5f) * v,
 *      cos(theta) = l / sqrtf((sx * sx + sy * sy) + l * l); the axial depth D = max(z * cos(theta), 1e-6f); the signed radius
 *      c = A * (1 - fd / D), negative: nearer than the focus.  A z that is not finite, is <= 0 or is >= 1e30 counts as infinitely
 *      far: c = A and D = 1e30f.  r = min(|c|, (float)K).
 *   2. Tile max.  K x K tiles from (0, 0), partial ones at the right and bottom: TX = ceil(W / K) by TY = ceil(H / K).  A tile's
 *      value is the largest r of its pixels (a float max is associative: any reduction order gives the same bits).
 *   3. Neighbour max.  Per tile, the largest tile-max value over the 3 x 3 tiles around it; tiles outside the grid are skipped.
 *      This is R.
 *   4. Early out.  R < 0.5f: out[p] = rgb[p] bit for bit -- a frame with dof = 0, aperture_scale = 0 or everything in focus comes
 *      back byte-identical.
 *   5. Gather, otherwise: scatter-as-gather in one layer.  rgb[p] with a channel that is not finite: out[p] = rgb[p].
 *      The tap table: N unit-disk offsets of a Vogel spiral, rho_i = sqrt((i + 0.5) / N), phi_i = i * pi * (3 - sqrt(5)),
 *      (ox_i, oy_i) = (rho_i cos(phi_i), rho_i sin(phi_i)), computed on the host in double and rounded to float (rt_dof_taps
 *      returns these bits).  Per pixel the table is turned by j quarter turns, j = {0, 2, 3, 1}[(y & 1) * 2 + (x & 1)]:
 *      (ox, oy), (-oy, ox), (-ox, -oy), (oy, -ox) for j = 0, 1, 2, 3 -- exact.  Taps i = 0 .. N-1, in this order:
 *        the tap pixel s = (floorf(((float)x + R * ox) + 0.5f), floorf(((float)y + R * oy) + 0.5f)).
 *      A tap outside the image, on p itself, or with a colour channel that is not finite, has weight 0.  Otherwise, with
 *      d = sqrtf(dx * dx + dy * dy) the distance of the two pixel centres and rp = r of p, rs = r of s:
 *        behind = min(max((D_s - D_p) / (depth_extent * max(min(D_s, D_p), 1e-6f)), 0), 1)
 *        r_e    = max(rs + behind * (min(rs, rp) - rs), 0.5f)
 *        cov    = min(max((r_e - d) + 0.5f, 0), 1)
 *        w_i    = (((R * R) / (float)N) * cov) / (r_e * r_e)
 *      -- the tap's share of the gathered disk's area times the energy density of its own disk; a tap that lies behind p cannot
 *      spread further over p than p's own blur, so an in-focus foreground stays sharp against a blurred background.
 *      The centre: w_p = 1 / (q * q), q = max(rp, 0.5f), on rgb[p].  Per channel, sums from the centre term on, taps in order:
 *        out[p] = (w_p * rgb[p] + sum w_i * rgb[s_i]) / (w_p + sum w_i)
 *      If no tap has a weight > 0 (that is, cov > 0): out[p] = rgb[p] bit for bit.
 *      Settled constants: N = 32 by default (the spiral then has a tap per 25 pixels of the largest default disk, K = 16, and
 *      the quarter turns quadruple that over a 2 x 2 block); a half-pixel linear edge on the disks (the + 0.5f of cov); 0.5f as
 *      the floor of every radius (a sharp pixel is a disk of one pixel's area to within pi / 4).
 *   6. No atomics, fixed orders: byte-identical outputs for identical inputs on one build.  The weights are normalised: a frame
 *      of one colour keeps it to rounding whatever z is.  out must NOT be rgb_linear (the gather reads neighbours), and no two
 *      planes may overlap.  Products that overflow float (colours near FLT_MAX) are outside the definition.
 * The stage's limit: it has ONE layer.  What a blurred foreground hides is not in the frame and is not recovered -- the background
 * seen through the soft edge of a near object is what lies beside it, not behind it -- and a blurred foreground over a sharp
 * background is an approximation by normalised weights.
 * rt_dof owns the (c, D) plane (8 bytes a pixel) and the two tile planes of one W x H stream of frames on one device, sized for the
 * smallest K, so the device entry never allocates.  Calls on one rt_dof are ordered on the GPU one behind the other, whatever
 * their streams.
 * Everything is checked before the GPU is touched and is RT_ERR_ARG: NULL arguments, a struct_size that is not the caller's sizeof,
 * max_coc outside 2..32, samples outside 8..64, depth_extent not finite or < 1e-3, aperture_scale not finite or negative, focus
 * not 0 and not in (0, 1e20], a NULL rgb_linear, z or out, a camera whose fov is not in (0, 180), whose dof is not finite, whose
 * focaldist (used when focus is 0) is not in (0, 1e20], whose size is <= 0 or differs from the rt_dof's, or whose A is not finite,
 * planes that overlap.  More than 2^30 pixels: RT_ERR_LIMIT.  Then, without a gfx950 device: RT_ERR_NO_DEVICE (there is no CPU
 * path). */
typedef struct rt_dof rt_dof;
typedef struct rt_dof_params {
    uint32_t struct_size;
    int32_t  max_coc;           /* 16   : K, the tile size and the largest radius of a circle of confusion in pixels, 2..32 */
    int32_t  samples;           /* 32   : N, taps per pixel, 8..64                                                          */
    float    depth_extent;      /* 0.05 : the relative depth difference over which `behind` rises from 0 to 1               */
    float    aperture_scale;    /* 1    : multiplies the camera's dof; 0 switches the stage off                             */
    float    focus;             /* 0    : the camera's focaldist; otherwise the distance in focus (a focus pull without a new render) */
} rt_dof_params;
typedef struct rt_dof_planes {
    uint32_t struct_size;
    const float *rgb_linear;
    const float *z;
    float *out;                 /* not rgb_linear */
    float *out_coc;             /* optional: float W*H, the signed UNCLAMPED c of each pixel */
    float *out_tiles;           /* optional: float TX*TY, R of each tile                     */
} rt_dof_planes;
/* w, h <= 0 or out == NULL: RT_ERR_ARG; more than 2^30 pixels: RT_ERR_LIMIT; no gfx950 device: RT_ERR_NO_DEVICE */
rt_status rt_dof_create(int device, int32_t w, int32_t h, rt_dof **out);
/* NULL is ignored; waits for the work that still uses it */
void      rt_dof_destroy(rt_dof *d);
void      rt_dof_default_params(rt_dof_params *p);
/* DIAGNOSTIC, needs no device: the tile grid of step 2, *tx = TX and *ty = TY (either may be NULL) */
rt_status rt_dof_tiles(int32_t w, int32_t h, int32_t max_coc, int32_t *tx, int32_t *ty);
/* DIAGNOSTIC, needs no device: the tap table of step 5 for N = samples (8..64), xy[2 * i] = ox_i and xy[2 * i + 1] = oy_i */
rt_status rt_dof_taps(int32_t samples, float *xy);
/* The planes are DEVICE pointers on the rt_dof's device; the kernels are enqueued on `hip_stream` (NULL = the device's legacy null
 * stream) and the call returns without waiting for them unless `sync` is non-zero. */
rt_status rt_dof_device(rt_dof *d, void *hip_stream, const rt_camera *cam, const rt_dof_params *p,
                        const rt_dof_planes *device_planes, int sync);
/* The planes are HOST arrays: upload, run, download. */
rt_status rt_dof_host(rt_dof *d, const rt_camera *cam, const rt_dof_params *p, const rt_dof_planes *host_planes);

/* ---- single-stage entry points (used by parity tests and by hosts that keep their own
 *      RenderPixel): inputs/outputs are HOST arrays, the work runs on the GPU -------------- */
/* n closest-hit queries = n calls of TraceNode(rootNode, ray, hit) (FIN/main.cpp:94-130).
 * rays: n x 6 floats (p, dir).  Outputs per ray: hit flag, z, p[3], N[3], node index, front. */
rt_status rt_trace_rays(rt_scene *s, int shade_model, int device, const float *rays, int64_t n,
                        uint8_t *hit, float *z, float *p, float *N, int32_t *node,
                        uint8_t *front);
/* n irradiance estimates = n calls of photonmap.EstimateIrradiance<k>(irr, dir, radius, pos,
 * &normal, 1, CONSTANT) (FIN/include/cyPhotonMap.h:288-336).  pos, normal: n x 3 floats;
 * outputs irr, dir: n x 3 floats. */
rt_status rt_estimate_irradiance(rt_scene *s, int device, int32_t k, float radius,
                                 const float *pos, const float *normal, int64_t n,
                                 float *irr, float *dir);
/* n shades of primary-ray samples = Trace + MtlBlinn::Shade(ray, hit, lights, bounce, 0)
 * (FIN/main.cpp:294-297): rays n x 6; outputs hit flag, rgb (linear, before gamma), z. */
rt_status rt_shade_rays(rt_scene *s, const rt_params *p, int device, const float *rays,
                        int64_t n, uint8_t *hit, float *rgb, float *z);

#ifdef __cplusplus
}
#endif
#endif /* RT_MI355X_H */
