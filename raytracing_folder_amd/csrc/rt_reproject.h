// rt_reproject.h -- steps 2-3 of "temporal accumulation" (rt_mi355x.h) as the one device function k_temporal (rt_temporal.hip) and
// k_motion (rt_motion.hip) both run: a pixel's world point from z and this frame's camera, optionally carried by a node's affine
// map into the previous frame's world ("motion vectors"), and that point's position in the previous camera's image.
// Device code only.  Every operation rounds once (the translation units are built with -ffp-contract=off), in the order written
// here: this order is part of what the tests' pixel bounds count.
#ifndef RT_REPROJECT_H
#define RT_REPROJECT_H

#include <hip/hip_runtime.h>

#include "rt_launch.h"          // DevCamera, DevNodeMotion

struct Reprojected { float fx, fy, zexp; };

// false: q.z >= 0, the point lies in or behind the previous camera's plane and has no position in its image (`out` is not written).
// AFFINE: P goes through `a` between the two steps (k_motion); without it `a` is not read and the code is k_temporal's as it
// always was.
template <bool AFFINE>
__device__ __forceinline__ bool reproject_pixel(const DevCamera &cur, const DevCamera &old, int x, int y, float zp, const DevNodeMotion *a, Reprojected &out)
{
    // 2. the pixel's representative ray through s = (b.x + (x + 0.5) u, b.y + (y + 0.5) v, -l) and its world point
    const float sx = cur.b[0] + ((float)x + 0.5f) * cur.u, sy = cur.b[1] + ((float)y + 0.5f) * cur.v, sz = cur.b[2];
    const float *m = cur.m;
    float rx = sx * m[0] + sy * m[3] + sz * m[6], ry = sx * m[1] + sy * m[4] + sz * m[7], rz = sx * m[2] + sy * m[5] + sz * m[8];
    const float inv = 1.0f / sqrtf(rx * rx + ry * ry + rz * rz);
    rx *= inv; ry *= inv; rz *= inv;
    float Px = cur.pos[0] + zp * rx, Py = cur.pos[1] + zp * ry, Pz = cur.pos[2] + zp * rz;
    if (AFFINE) {                       // the node's motion: an identity map (R = I, t = 0) returns P bit for bit (-0 as +0)
        const float ax = a->row[0].x * Px + a->row[0].y * Py + a->row[0].z * Pz + a->row[0].w;
        const float ay = a->row[1].x * Px + a->row[1].y * Py + a->row[1].z * Pz + a->row[1].w;
        const float az = a->row[2].x * Px + a->row[2].y * Py + a->row[2].z * Pz + a->row[2].w;
        Px = ax; Py = ay; Pz = az;
    }
    // 3. into the previous camera: q = (x_new', up', z_new') . (P - pos')
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

#endif
