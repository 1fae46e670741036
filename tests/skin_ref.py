"""An independent float32 transcription of linear-blend skinning as include/rt_mi355x.h defines it ("mesh skinning"): the yardstick
the host mirror rt_mesh_skin is held against, byte for byte.  Vectorised over the vertices: every `*` and `+` of the definition
is ONE numpy float32 array operation, in the stated order -- numpy rounds each to float32 and fuses nothing."""
import numpy as np

F = np.float32


def skin(v_rest, bone_index, weight, bones):
    """posed positions float32 (nv, 3):
        for k = 0, 1, 2, 3, with M = bones[bone_index[i][k]], w = weight[i][k]:
            t   = ((M[r][0]*x + M[r][1]*y) + M[r][2]*z) + M[r][3]
            acc = (k == 0) ? w*t : acc + w*t
        p[r] = acc"""
    v = np.ascontiguousarray(v_rest, F).reshape(-1, 3)
    idx = np.ascontiguousarray(bone_index, np.uint16).reshape(-1, 4).astype(np.int64)
    w = np.ascontiguousarray(weight, F).reshape(-1, 4)
    B = np.ascontiguousarray(bones, F).reshape(-1, 3, 4)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    out = np.empty_like(v)
    for r in range(3):
        acc = None
        for k in range(4):
            M = B[idx[:, k], r]                      # (nv, 4): row r of the k-th bone of every vertex
            t = M[:, 0] * x
            t = t + M[:, 1] * y
            t = t + M[:, 2] * z
            t = t + M[:, 3]
            assert t.dtype == F
            wt = w[:, k] * t
            acc = wt if k == 0 else acc + wt
        assert acc.dtype == F
        out[:, r] = acc
    return out
