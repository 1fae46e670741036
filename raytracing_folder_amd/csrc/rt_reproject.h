// rt_reproject.h -- steps 2-3 of "temporal accumulation" (rt_mi355x.h) as the one device function k_temporal (rt_temporal.hip),
// k_motion (rt_motion.hip) and the rigid pixels of k_motion_mesh (rt_motion_mesh.hip) all run, and its pieces, which the mesh pixels
// of k_motion_mesh put together around a ray walk: a pixel's world point from z and this frame's camera, optionally carried by a node's affine
// map into the previous frame's world ("motion vectors"), and that point's position in the previous camera's image.
// Device code only.  Every operation rounds once (the translation units are built with -ffp-contract=off), in the order written
// here: this order is part of what the tests' pixel bounds count.
#ifndef RT_REPROJECT_H
#define RT_REPROJECT_H

#include <hip/hip_runtime.h>

#include "rt_launch.h"          // DevCamera, DevNodeMotion

struct Reprojected { float fx, fy, zexp; };

// step 2's representative ray of pixel (x, y): the unit direction normalize(M s(x, y)) through s = (b.x + (x + 0.5) u, b.y + (y + 0.5) v, -l)
__device__ __forceinline__ void pixel_ray(const DevCamera &cur, int x, int y, float &rx, float &ry, float &rz)
{
    const float sx = cur.b[0] + ((float)x + 0.5f) * cur.u, sy = cur.b[1] + ((float)y + 0.5f) * cur.v, sz = cur.b[2];
    const float *m = cur.m;
    rx = sx * m[0] + sy * m[3] + sz * m[6]; ry = sx * m[1] + sy * m[4] + sz * m[7]; rz = sx * m[2] + sy * m[5] + sz * m[8];
    const float inv = 1.0f / sqrtf(rx * rx + ry * ry + rz * rz);
    rx *= inv; ry *= inv; rz *= inv;
}

// an affine map of "motion vectors" applied to a point, per component ((R_k0 X + R_k1 Y) + R_k2 Z) + t_k: an identity map (R = I,
// t = 0) returns the point bit for bit (-0 as +0)
__device__ __forceinline__ void affine_apply(const DevNodeMotion *a, float &Px, float &Py, float &Pz)
{
    const float ax = a->row[0].x * Px + a->row[0].y * Py + a->row[0].z * Pz + a->row[0].w;
    const float ay = a->row[1].x * Px + a->row[1].y * Py + a->row[1].z * Pz + a->row[1].w;
    const float az = a->row[2].x * Px + a->row[2].y * Py + a->row[2].z * Pz + a->row[2].w;
    Px = ax; Py = ay; Pz = az;
}

// step 3: a world point into the previous camera, q = (x_new', up', z_new') . (P - pos').  false: q.z >= 0, the point lies in or
// behind the previous camera's plane and has no position in its image (`out` is not written).
__device__ __forceinline__ bool project_previous(const DevCamera &old, float Px, float Py, float Pz, Reprojected &out)
{
    const float ex = Px - old.pos[0], ey = Py - old.pos[1], ez = Pz - old.pos[2];
    const float *o = old.m;
    const float qx = o[0] * ex + o[1] * ey + o[2] * ez, qy = o[3] * ex + o[4] * ey + o[5] * ez, qz = o[6] * ex + o[7] * ey + o[8] * ez;
    if (!(qz < 0.0f)) return false;
    const float t = old.b[2] / qz;      // -l' / q.z
    out.fx = (qx * t - old.b[0]) / old.u - 0.5f;
    out.fy = (qy * t - old.b[1]) / old.v - 0.5f;
    out.zexp = sqrtf(ex * ex + ey * ey + ez * ez);
    return true;
}

// Steps 2 and 3 of one pixel; false as project_previous.
// AFFINE: P goes through `a` between the two steps (k_motion); without it `a` is not read and the code is k_temporal's as it
// always was.
template <bool AFFINE>
__device__ __forceinline__ bool reproject_pixel(const DevCamera &cur, const DevCamera &old, int x, int y, float zp, const DevNodeMotion *a, Reprojected &out)
{
    float rx, ry, rz;
    pixel_ray(cur, x, y, rx, ry, rz);
    float Px = cur.pos[0] + zp * rx, Py = cur.pos[1] + zp * ry, Pz = cur.pos[2] + zp * rz;
    if (AFFINE) affine_apply(a, Px, Py, Pz);        // the node's motion
    return project_previous(old, Px, Py, Pz, out);
}

// Steps a.-e. of "motion vectors" for one pixel whose z and id passed d.'s tests on them: k_motion's pixel, and a rigid pixel of
// k_motion_mesh.  (fx, fy, zexp) come in as (x, y, 0), "no previous position", and stay so when q.z >= 0.  same_camera: cur and old
// are bit-identical.
__device__ __forceinline__ void motion_rigid_pixel(const DevCamera &cur, const DevCamera &old, int same_camera, const DevNodeMotion *entry,
                                                   int x, int y, float zp, float &fx, float &fy, float &zexp)
{
    const float4 *rows = entry->row;
    DevNodeMotion a;
    a.row[0] = rows[0]; a.row[1] = rows[1]; a.row[2] = rows[2];
    Reprojected r;
    const bool still = same_camera && zp > 0.0f &&
                       a.row[0].x == 1.0f && a.row[0].y == 0.0f && a.row[0].z == 0.0f && a.row[0].w == 0.0f &&
                       a.row[1].x == 0.0f && a.row[1].y == 1.0f && a.row[1].z == 0.0f && a.row[1].w == 0.0f &&
                       a.row[2].x == 0.0f && a.row[2].y == 0.0f && a.row[2].z == 1.0f && a.row[2].w == 0.0f;
    if (still) zexp = zp;               // did not move: (x, y, z) exactly
    else if (reproject_pixel<true>(cur, old, x, y, zp, &a, r)) { fx = r.fx; fy = r.fy; zexp = r.zexp; }
}

#endif
