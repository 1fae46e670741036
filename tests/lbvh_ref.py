"""The device tree build's definition (include/rt_mi355x.h, "device tree build") written a second, independent way (TEST
INFRASTRUCTURE, from the definition's text, not from csrc/rt_lbvh.h): keys in NumPy float32, a TOP-DOWN recursive split of the
sorted key range at its highest differing bit -- no Karras ranges, no parent links --, every box as the min / max over the
vertices of the faces beneath it, the four-wide collapse and the breadth-first numbering in plain Python.  The yardstick of
tests/test_lbvh_host.py and tests/test_mesh_device_build.py; the mirror and the kernels are the code under test.  Also the meshes
both files run on."""
import numpy as np

from raytracing_folder_amd import capi, workloads
from tests import deep_meshes, test_mesh_refit as R

F = np.float32
LEAF = 0x80000000


def leafref(off, cnt):
    return LEAF | ((cnt - 1) << 28) | off


def keys_of(v, f):
    tri = np.asarray(v, F).reshape(-1, 3)[np.asarray(f).reshape(-1, 3)]
    c = F(0.5) * (tri.min(1) + tri.max(1))
    clo, chi = c.min(0), c.max(0)
    morton = np.zeros(len(c), np.uint64)
    for a in range(3):
        with np.errstate(all="ignore"):
            ext = F(chi[a] - clo[a])
            if not (ext > 0 and np.isfinite(ext)):
                q = np.zeros(len(c), np.int64)
            else:
                x = (c[:, a] - clo[a]) * (F(1024.0) / ext)
                q = np.clip(np.trunc(x).astype(np.int64), 0, 1023)
        for b in range(10):
            morton |= (((q >> b) & 1).astype(np.uint64)) << np.uint64(3 * b + 2 - a)
    return (morton << np.uint64(32)) | np.arange(len(c), dtype=np.uint64)


def build(v, f):
    """(nodes DEVBVHNODE, slot_face uint32, root_ref, stack_need, level_off) of the definition"""
    v, f = np.asarray(v, F).reshape(-1, 3), np.asarray(f).reshape(-1, 3)
    keys = np.sort(keys_of(v, f))
    slot_face = (keys & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    nf = len(f)
    if nf <= 4:
        return np.zeros(0, capi.DEVBVHNODE), slot_face, leafref(0, nf), 0, [0]
    pts = v[f[slot_face]]                                    # (slot, corner, axis)
    ik = [int(k) for k in keys]
    binary = []                                              # [left, right, lo, hi]: a child is ("leaf", first, count) or ("node", index)

    def box(first, last):
        p = pts[first:last + 1].reshape(-1, 3)
        return p.min(0), p.max(0)

    def split(first, last):
        """the binary node over slots first .. last (more than four of them): its index in `binary`"""
        bit = (ik[first] ^ ik[last]).bit_length() - 1        # the highest bit in which the range's keys differ
        prefix = (ik[first] >> bit) << bit                   # ... is clear in the first key: the right part starts where it is set
        mid = int(np.searchsorted(keys, np.uint64(prefix | (1 << bit)), side="left"))
        me = len(binary)
        binary.append(None)
        kids = []
        for a, b in ((first, mid - 1), (mid, last)):
            kids.append((("leaf", a, b - a + 1) if b - a + 1 <= 4 else ("node", split(a, b))) + box(a, b))
        binary[me] = kids
        return me

    import sys
    sys.setrecursionlimit(max(sys.getrecursionlimit(), 10000))
    root = split(0, nf - 1)

    def area(lo, hi):
        with np.errstate(all="ignore"):
            d = hi - lo
            return F(2.0) * ((d[0] * d[1] + d[1] * d[2]) + d[2] * d[0])

    records, level_off, need = [], [0], 0
    level = [(root, 0)]
    while level:
        nxt = []
        base = len(records) + len(level)
        for b, held in level:
            ch = list(binary[b])
            while len(ch) < 4:
                pick, big = -1, F(-1.0)
                for i, c in enumerate(ch):
                    if c[0] == "node":
                        s = area(c[-2], c[-1])
                        if s > big:
                            pick, big = i, s
                if pick < 0:
                    break
                ch[pick:pick + 1] = binary[ch[pick][1]]
            held2 = held + len(ch) - 1
            need = max(need, held2)
            rec = np.zeros((), capi.DEVBVHNODE)
            rec["lo"][:], rec["hi"][:] = np.nan, np.nan
            rec["c"][:] = leafref(0, 1)
            for i, c in enumerate(ch):
                rec["lo"][:, i], rec["hi"][:, i] = c[-2], c[-1]
                if c[0] == "leaf":
                    rec["c"][i] = leafref(c[1], c[2])
                else:
                    rec["c"][i] = base + len(nxt)
                    nxt.append((c[1], held2))
            records.append(rec)
        level_off.append(len(records))
        level = nxt
    return np.array(records, capi.DEVBVHNODE), slot_face, 0, need, level_off


def same_tree(got_nodes, got_slot_face, want_nodes, want_slot_face, what=""):
    """refs, padding and slot order byte for byte; bounds equal as floats (the sign of a zero is free), NaNs in the same places"""
    assert got_slot_face.tobytes() == want_slot_face.tobytes(), (what, "slot_face")
    assert len(got_nodes) == len(want_nodes), (what, len(got_nodes), len(want_nodes))
    assert got_nodes["c"].tobytes() == want_nodes["c"].tobytes(), (what, "refs")
    assert not got_nodes["pad"].any(), (what, "pad")
    for k in ("lo", "hi"):
        a, b = got_nodes[k], want_nodes[k]
        assert (np.isnan(a) == np.isnan(b)).all(), (what, k, "NaN places")
        assert (a[~np.isnan(a)] == b[~np.isnan(b)]).all(), (what, k)


# ---- the meshes ---------------------------------------------------------------------------------------------------------------
REFIT = ("teapot", "strip5", "tri3", "deep")                 # tests/test_mesh_refit.py's, with its rays and its qualification


def coincident(n=64):
    """n copies of one triangle: every Morton code is equal and only the face bits tell the keys apart"""
    return (np.tile(np.array([[0.5, 0.25, 1.0], [2.5, 0.5, 1.25], [1.0, 2.0, 0.75]], F), (n, 1)), np.arange(3 * n, dtype=np.uint32).reshape(n, 3))


_meshes = {}


def meshes():
    """name -> (v, f): every mesh of the issue's list, undeformed"""
    if not _meshes:
        for name in REFIT:
            _meshes[name] = R._mesh(name)[:2]
        for name, m in deep_meshes.awkward_meshes().items():
            _meshes["awkward_" + name] = m
        _meshes["sheet16"] = workloads.sheet(16, 4.0)        # flat: no centroid extent along z
        _meshes["coincident64"] = coincident(64)
        _meshes["clustered2000"] = deep_meshes.clustered_soup(2000)
    return _meshes
