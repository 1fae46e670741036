"""An independent float32 transcription of include/rt_mi355x.h, "smooth normals": a Python loop over the corners in ascending
order with np.float32 scalars, one operation at a time -- no vectorised sum whose order numpy chooses.  Shares no code with the
library (csrc/rt_mesh_normals.h), which tests/test_mesh_normals.py holds against it byte for byte."""
import numpy as np

F = np.float32


def _face_normal(v, tri):
    a, b, c = v[tri[0]], v[tri[1]], v[tri[2]]
    ux, uy, uz = F(b[0] - a[0]), F(b[1] - a[1]), F(b[2] - a[2])
    wx, wy, wz = F(c[0] - a[0]), F(c[1] - a[1]), F(c[2] - a[2])
    return (F(F(uy * wz) - F(uz * wy)), F(F(uz * wx) - F(ux * wz)), F(F(ux * wy) - F(uy * wx)))


def smooth_normals(v, f, fn=None, vn=None):
    """float32 (nvn, 3): normal j is S_j / |S_j|, S_j the face normals of the corners c with fn[c] == j added in ascending c from
    (0, 0, 0); a normal no corner names, or whose length is 0 or not finite, keeps its stored value (vn; None: nv zeros)"""
    v = np.ascontiguousarray(v, F).reshape(-1, 3)
    f = np.ascontiguousarray(f, np.uint32).reshape(-1, 3)
    fn = f if fn is None else np.ascontiguousarray(fn, np.uint32).reshape(-1, 3)
    out = np.zeros((len(v), 3), F) if vn is None else np.array(vn, F).reshape(-1, 3)
    S = [[F(0), F(0), F(0)] for _ in range(len(out))]
    named = [False] * len(out)
    with np.errstate(all="ignore"):
        for i in range(len(f)):
            N = _face_normal(v, f[i])
            for k in range(3):                                   # corner c = 3 i + k, ascending
                j = int(fn[i, k])
                S[j] = [F(S[j][0] + N[0]), F(S[j][1] + N[1]), F(S[j][2] + N[2])]
                named[j] = True
        for j, (x, y, z) in enumerate(S):
            if not named[j]:
                continue
            length = F(np.sqrt(F(F(F(x * x) + F(y * y)) + F(z * z))))
            if not np.isfinite(length) or not length > 0:
                continue
            out[j] = (F(x / length), F(y / length), F(z / length))
    return out
