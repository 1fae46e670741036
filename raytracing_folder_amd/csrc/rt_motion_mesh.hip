// rt_motion_mesh.hip -- motion vectors for a scene whose meshes deform: k_motion's plane, with the pixels of a mesh that holds
// previous positions followed through the deformation.  The definition the kernel follows is in include/rt_mi355x.h ("motion
// vectors for deforming meshes"); the reference has no counterpart.  This is the one motion unit that traces: rt_motion.hip stays
// free of rt_trace.h, and rt_trace.h stays as the tracing kernels have it -- the walk below is put together from its pieces
// (box_entry, the triangle tests, the stack), because the kernel needs the slot and the barycentrics of the closest hit, which
// mesh_hit computes and does not return.
//
//   k_motion_mesh  one lane per pixel, RT_BLOCK lanes = one 32 x 8 tile (k_motion's), at most RT_SPILL_BLOCKS workgroups that walk
//                  the tiles one after the other (the spill part of the traversal stack is sized for that many).  A lane reads its
//                  z and object id and its node's DevMotionMeshNode.  Rigid: k_motion's pixel, the same function.  Mesh: the
//                  pinhole ray through the pixel centre, down the object's chain as trace() takes it, the closest hit in the
//                  mesh's tree (while-while, near child first, RT_BVH_STACK entries in LDS and the spill behind them), the depth
//                  gate against z, the hit's barycentrics applied to the previous positions of its slot's vertices, the previous
//                  chain's object-to-world map, the previous camera.
//
// No atomics: identical inputs give identical bytes.  Neighbouring lanes mostly share an object, so the per-lane loads of the
// chain and the mesh record coalesce into broadcasts.
#include <hip/hip_runtime.h>
#include <string.h>

#include "rt_launch.h"
#include "rt_reproject.h"
#include "rt_trace.h"

#define RT_MOTION_TILE_W 32
#define RT_MOTION_TILE_H 8
#define RT_MOTION_NO_HIT 1.0e30f         /* the z plane's "nothing hit" (BIGFLOAT) */
static_assert(RT_MOTION_TILE_W * RT_MOTION_TILE_H == RT_BLOCK, "bvh_stack strides the LDS stack by RT_BLOCK");

// the kernel's argument: members, order and types are its layout
struct MotionMeshArgs {
    int width, height, tiles_x, n_tiles, n_nodes;
    int same_camera;                    // cur and old are bit-identical
    float depth_tol;
    DevCamera cur, old;
    const float *z; const int32_t *object_id;
    const DevNodeMotion *table;         // [n_nodes] this frame's world -> the previous frame's (rigid pixels)
    const DevMotionMeshNode *mesh_nodes;    // [n_nodes]
    const DevNodeMotion *from;          // [n_nodes] the previous chain's object -> world (mesh pixels)
    const DevNodeXf *nodes; const DevObject *objects; const DevMesh *meshes;
    uint32_t *spill;
    float *motion;                      // [width * height * 3]
};

// The closest hit of (o, d) in one mesh's tree: mesh_hit<false, MODEL>'s traversal -- the root box first, near child first, the
// same triangle test, `t < z` keeps the nearest -- returning what the motion needs of it: the slot and the barycentrics.
template <bool P13>
__device__ bool mesh_closest_slot(const DevMesh &M, V3 o, V3 d, const BvhStack &stack, float &z, uint32_t &best_slot, V3 &bc)
{
    const V3 inv = mk(slab_inv(d.x, 1.0f / d.x), slab_inv(d.y, 1.0f / d.y), slab_inv(d.z, 1.0f / d.z));
    if (box_entry(M.root_box, M.root_box + 3, o, inv, z) > 2.0e30f) return false;
    uint32_t cur = M.root_ref;          // a mesh of at most four triangles: a leaf ref, and no node record is read
    uint32_t sp = 0;
    bool any = false;
    V3 hp; int front;
    const uint32_t DONE = 0xFFFFFFFFu;  // has LEAF_BIT set: ends the inner loop
    while (cur != DONE) {
        while (!(cur & LEAF_BIT)) {
            const float4 *np = (const float4 *)(M.nodes + cur);
            const float4 lx = np[0], ly = np[1], lz = np[2], hx = np[3], hy = np[4], hz = np[5];
            const uint4 cr = *(const uint4 *)(np + 6);
            const float l0[3] = {lx.x, ly.x, lz.x}, h0[3] = {hx.x, hy.x, hz.x}, l1[3] = {lx.y, ly.y, lz.y}, h1[3] = {hx.y, hy.y, hz.y};
            const float l2[3] = {lx.z, ly.z, lz.z}, h2[3] = {hx.z, hy.z, hz.z}, l3[3] = {lx.w, ly.w, lz.w}, h3[3] = {hx.w, hy.w, hz.w};
            float e0 = box_entry(l0, h0, o, inv, z), e1 = box_entry(l1, h1, o, inv, z);
            float e2 = box_entry(l2, h2, o, inv, z), e3 = box_entry(l3, h3, o, inv, z);      // an unused child's bounds are NaN: never entered
            uint32_t c0 = cr.x, c1 = cr.y, c2 = cr.z, c3 = cr.w;
            // nearest first, as mesh_hit sorts them (misses carry 3e30 and end up last)
#define RT_CSWAP(ea, ca, eb, cb) do { const bool s_ = (eb) < (ea); const float te_ = s_ ? (eb) : (ea); const uint32_t tc_ = s_ ? (cb) : (ca); \
                                      (eb) = s_ ? (ea) : (eb); (cb) = s_ ? (ca) : (cb); (ea) = te_; (ca) = tc_; } while (0)
            RT_CSWAP(e0, c0, e1, c1); RT_CSWAP(e2, c2, e3, c3); RT_CSWAP(e0, c0, e2, c2); RT_CSWAP(e1, c1, e3, c3); RT_CSWAP(e1, c1, e2, c2);
#undef RT_CSWAP
            if (e3 < 2.0e30f) bvh_push(stack, sp, c3);
            if (e2 < 2.0e30f) bvh_push(stack, sp, c2);
            if (e1 < 2.0e30f) bvh_push(stack, sp, c1);
            cur = (e0 < 2.0e30f) ? c0 : (sp ? bvh_pop(stack, sp) : DONE);
        }
        if (cur == DONE) break;
        const uint32_t count = ((cur >> 28) & 7u) + 1;
        const uint32_t first = cur & 0x0FFFFFFFu;
        for (uint32_t i = 0; i < count; i++) {
            const DevTri T = M.tris[first + i];
            const bool h = P13 ? tri_hit_p13(T, o, d, z, hp, bc, front) : tri_hit_fin(T, o, d, z, hp, bc, front);
            if (h) { any = true; best_slot = first + i; }
        }
        cur = sp ? bvh_pop(stack, sp) : DONE;
    }
    return any;
}

template <bool P13>
__global__ __launch_bounds__(RT_BLOCK) void k_motion_mesh(MotionMeshArgs A)
{
    __shared__ uint32_t s_stack[RT_BVH_STACK * RT_BLOCK];
    const BvhStack stack = bvh_stack(s_stack, RT_BVH_STACK, A.spill);
    for (int tile = (int)blockIdx.x; tile < A.n_tiles; tile += (int)gridDim.x) {
        const int tx = tile % A.tiles_x, ty = tile / A.tiles_x;
        const int x = tx * RT_MOTION_TILE_W + (int)(threadIdx.x % RT_MOTION_TILE_W);
        const int y = ty * RT_MOTION_TILE_H + (int)(threadIdx.x / RT_MOTION_TILE_W);
        if (x >= A.width || y >= A.height) continue;        // (no barrier in this loop: a lane's stack is its own)
        const size_t p = (size_t)y * A.width + x;
        const float zp = A.z[p];
        const int id = A.object_id[p];
        float fx = (float)x, fy = (float)y, zexp = 0.0f;    // "no previous position"
        // (zp < 1e30 is false for NaN and +inf; -inf fails zp - zp == 0)
        if (id >= 0 && id < A.n_nodes && zp < RT_MOTION_NO_HIT && zp - zp == 0.0f) {
            const DevMotionMeshNode mn = A.mesh_nodes[id];
            if (mn.object < 0) motion_rigid_pixel(A.cur, A.old, A.same_camera, A.table + id, x, y, zp, fx, fy, zexp);
            else {
                // a'. the pinhole ray through the pixel centre, into the object's coordinates down the current chain: Node::ToNodeCoords
                // level by level as trace() applies it (the direction is the image of p + d minus the image of p, not renormalised)
                float rx, ry, rz;
                pixel_ray(A.cur, x, y, rx, ry, rz);
                V3 lp = ld3(A.cur.pos), ldir = mk(rx, ry, rz);
                const DevObject *ob = A.objects + mn.object;
                const int len = ob->chain_len;
                for (int c = 0; c < len; c++) {
                    const DevNodeXf *X = A.nodes + ob->chain[c];
                    const V3 pos = ld3(X->pos);
                    const V3 rp = mmul(X->itm, lp - pos);
                    ldir = mmul(X->itm, (lp + ldir) - pos) - rp;
                    lp = rp;
                }
                // b'. the closest hit in the mesh's tree
                const DevMesh M = A.meshes[mn.mesh];
                float t = BIGFLOAT;
                uint32_t slot = 0;
                V3 bc = mk(0, 0, 0);
                const bool hit = mesh_closest_slot<P13>(M, lp, ldir, stack, t, slot, bc);
                // c'. the gate: the centre ray must have found the surface the (jittered) sample's depth belongs to
                if (hit && !(fabsf(t - zp) > A.depth_tol * zp)) {
                    // d'. the same barycentrics on the slot's previous vertices, then the previous chain's object-to-world map
                    const uint32_t *ix = mn.slot_idx + 6 * (size_t)slot;
                    const V3 Ap = ld3(mn.v_prev + 3 * (size_t)ix[0]), Bp = ld3(mn.v_prev + 3 * (size_t)ix[1]), Cp = ld3(mn.v_prev + 3 * (size_t)ix[2]);
                    float Px = (bc.x * Ap.x + bc.y * Bp.x) + bc.z * Cp.x;
                    float Py = (bc.x * Ap.y + bc.y * Bp.y) + bc.z * Cp.y;
                    float Pz = (bc.x * Ap.z + bc.y * Bp.z) + bc.z * Cp.z;
                    const float4 *rows = A.from[id].row;
                    DevNodeMotion a;
                    a.row[0] = rows[0]; a.row[1] = rows[1]; a.row[2] = rows[2];
                    affine_apply(&a, Px, Py, Pz);
                    // e'. into the previous camera
                    Reprojected r;
                    if (project_previous(A.old, Px, Py, Pz, r)) { fx = r.fx; fy = r.fy; zexp = r.zexp; }
                }
            }
        }
        A.motion[3 * p] = fx; A.motion[3 * p + 1] = fy; A.motion[3 * p + 2] = zexp;
    }
}

void rtk_launch_motion_mesh(hipStream_t st, const MotionMeshRequest &R)
{
    const MotionRequest &Q = R.rigid;
    MotionMeshArgs A = {};
    A.width = Q.width; A.height = Q.height; A.tiles_x = (Q.width + RT_MOTION_TILE_W - 1) / RT_MOTION_TILE_W;
    const long long tiles = (long long)A.tiles_x * ((Q.height + RT_MOTION_TILE_H - 1) / RT_MOTION_TILE_H);     // (< 2^31: the callers cap the image at 2^30 pixels)
    A.n_tiles = (int)tiles; A.n_nodes = Q.n_nodes;
    A.cur = Q.cur; A.old = Q.old;
    A.same_camera = memcmp(&Q.cur, &Q.old, sizeof(DevCamera)) == 0;     // (DevCamera is 4-byte members only: no padding)
    A.depth_tol = R.depth_tol;
    A.z = Q.z; A.object_id = Q.object_id; A.table = Q.table; A.motion = Q.motion;
    A.mesh_nodes = R.mesh_nodes; A.from = R.from;
    A.nodes = R.S.nodes; A.objects = R.S.objects; A.meshes = R.S.meshes;
    A.spill = R.spill;
    const unsigned grid = (unsigned)(tiles < RT_SPILL_BLOCKS ? tiles : RT_SPILL_BLOCKS);
    if (R.p13) hipLaunchKernelGGL(k_motion_mesh<true>, dim3(grid), dim3(RT_BLOCK), 0, st, A);
    else hipLaunchKernelGGL(k_motion_mesh<false>, dim3(grid), dim3(RT_BLOCK), 0, st, A);
}
