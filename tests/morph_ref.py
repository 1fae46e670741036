"""An independent float32 transcription of morph targets as include/rt_mi355x.h defines them ("morph targets"): the yardstick the
host mirror rt_mesh_morph is held against, byte for byte.  Vectorised over the vertices, a Python loop over the targets whose
weight is not zero, ascending; every `*` and `+` of the definition is ONE float32 array operation wrapped in F(...), in the
stated order -- numpy rounds each to float32 and fuses nothing."""
import numpy as np

F = np.float32


def morph(v_base, deltas, weights):
    """morphed positions float32 (nv, 3):
        acc = base[i][c]
        for t ascending over the targets with weights[t] != 0:  acc = acc + weights[t] * deltas[t][i][c]"""
    v = np.ascontiguousarray(v_base, F).reshape(-1, 3)
    w = np.ascontiguousarray(weights, F).reshape(-1)
    d = np.ascontiguousarray(deltas, F).reshape(len(w), len(v), 3)
    acc = v.copy()
    for t in range(len(w)):
        if w[t] != 0:                                # +0 and -0 alike: the target is skipped, not multiplied
            acc = F(acc + F(w[t] * d[t]))
            assert acc.dtype == F
    return acc
