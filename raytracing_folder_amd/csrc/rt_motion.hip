// rt_motion.hip -- motion vectors in image space: where each pixel's surface point was in the previous frame's image, when nodes
// as well as the camera may have moved.  The definition the kernel follows is in include/rt_mi355x.h ("motion vectors"); the
// reference has no counterpart.  Like k_temporal it works on image-sized planes and never traces a ray: z and object_id describe
// one surface point per pixel, and the host hands it one affine map per node (this frame's world -> the previous frame's).
//
//   k_motion     one lane per pixel, 32 x 8 pixels per workgroup (k_temporal's tile): the lane's z and object id, its node's map
//                (48 bytes gathered from a table that stays in cache: a frame has few nodes and neighbouring lanes share them),
//                steps 2-3 of "temporal accumulation" through rt_reproject.h with the map between them, and the lane's
//                (fx, fy, z_exp).  A pixel without a previous position holds (x, y, 0); a pixel of a node that did not move,
//                under a camera that did not move either, holds (x, y, z) -- what the steps give in exact arithmetic.
//
// No atomics, no LDS: identical inputs give identical bytes.  20 bytes a pixel: z and id in, three floats out.
#include <hip/hip_runtime.h>
#include <string.h>

#include "rt_launch.h"
#include "rt_reproject.h"

#define RT_MOTION_TILE_W 32
#define RT_MOTION_TILE_H 8
#define RT_MOTION_NO_HIT 1.0e30f         /* the z plane's "nothing hit" (BIGFLOAT) */

// the kernel's argument: members, order and types are its layout
struct MotionArgs {
    int width, height, tiles_x, n_nodes;
    int same_camera;                    // cur and old are bit-identical
    DevCamera cur, old;                 // this frame's camera and the previous frame's (camera_setup's quantities)
    const float *z; const int32_t *object_id;
    const DevNodeMotion *table;         // [n_nodes]
    float *motion;                      // [width * height * 3]
};

__global__ __launch_bounds__(RT_MOTION_TILE_W * RT_MOTION_TILE_H) void k_motion(MotionArgs A)
{
    const int tx = (int)(blockIdx.x % (unsigned)A.tiles_x), ty = (int)(blockIdx.x / (unsigned)A.tiles_x);
    const int x = tx * RT_MOTION_TILE_W + (int)(threadIdx.x % RT_MOTION_TILE_W);
    const int y = ty * RT_MOTION_TILE_H + (int)(threadIdx.x / RT_MOTION_TILE_W);
    if (x >= A.width || y >= A.height) return;
    const size_t p = (size_t)y * A.width + x;
    const float zp = A.z[p];
    const int id = A.object_id[p];
    float fx = (float)x, fy = (float)y, zexp = 0.0f;        // "no previous position"
    // (zp < 1e30 is false for NaN and +inf; -inf fails zp - zp == 0)
    if (id >= 0 && id < A.n_nodes && zp < RT_MOTION_NO_HIT && zp - zp == 0.0f)
        motion_rigid_pixel(A.cur, A.old, A.same_camera, A.table + id, x, y, zp, fx, fy, zexp);
    A.motion[3 * p] = fx; A.motion[3 * p + 1] = fy; A.motion[3 * p + 2] = zexp;
}

void rtk_launch_motion(hipStream_t st, const MotionRequest &R)
{
    MotionArgs A = {};
    A.width = R.width; A.height = R.height; A.tiles_x = (R.width + RT_MOTION_TILE_W - 1) / RT_MOTION_TILE_W;
    A.n_nodes = R.n_nodes;
    A.cur = R.cur; A.old = R.old;
    A.same_camera = memcmp(&R.cur, &R.old, sizeof(DevCamera)) == 0;     // (DevCamera is 4-byte members only: no padding)
    A.z = R.z; A.object_id = R.object_id; A.table = R.table; A.motion = R.motion;
    const long long tiles = (long long)A.tiles_x * ((R.height + RT_MOTION_TILE_H - 1) / RT_MOTION_TILE_H);
    hipLaunchKernelGGL(k_motion, dim3((unsigned)tiles), dim3(RT_MOTION_TILE_W * RT_MOTION_TILE_H), 0, st, A);
}
