"""The host mirror of the device tree build (rt_device_lbvh_build: csrc/rt_lbvh.h behind the C ABI; the definition is in
include/rt_mi355x.h, "device tree build").  No GPU.  The yardstick is tests/lbvh_ref.py, the definition written a second way
(top-down splits at the highest differing key bit, boxes as min / max over the faces beneath); the mirror is the code under test,
and tests/test_mesh_device_build.py then holds the kernels against the mirror.

Meshes: the four of tests/test_mesh_refit.py (teapot, strip5, tri3 -- a root leaf --, the tower), the awkward six of
tests/deep_meshes.py, a flat sheet (no centroid extent on one axis), 64 coincident triangles (equal Morton codes: the face bits
alone separate the keys) and a clustered soup of 2000."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from raytracing_folder_amd import capi
from tests import bvh_walk, lbvh_ref, test_mesh_refit as R

F = np.float32
L = capi.lib
NAMES = tuple(lbvh_ref.meshes())

_built = {}


def _mirror(name):
    if name not in _built:
        _built[name] = capi.device_lbvh_build(*lbvh_ref.meshes()[name])
    return _built[name]


def test_symbols_are_exported():
    for name in ("rt_device_lbvh_build", "rt_scene_update_mesh_vertices_build", "rt_scene_update_mesh_vertices_auto_build"):
        assert hasattr(L(), name) and name in capi.SYMBOLS, name
    assert C.sizeof(capi.MeshBuildInfo) == 72
    assert (capi.MESH_BUILD_ON_DEVICE, capi.MESH_BUILD_FELL_BACK, capi.MESH_BUILD_NOT_ON_DEVICE) == (1, 2, 4)


def test_argument_errors_and_sizes_only_calls():
    v, f = lbvh_ref.meshes()["strip5"]
    p = capi._p
    info = capi.DeviceBvhInfo(struct_size=C.sizeof(capi.DeviceBvhInfo))
    call = L().rt_device_lbvh_build
    assert call(None, len(v), p(f), len(f), C.byref(info), None, 0, None, 0) == -1
    assert call(p(v), len(v), None, len(f), C.byref(info), None, 0, None, 0) == -1
    assert call(p(v), len(v), p(f), len(f), None, None, 0, None, 0) == -1
    assert L().rt_last_error() == b"rt_device_lbvh_build: NULL argument"
    assert call(p(v), 0, p(f), len(f), C.byref(info), None, 0, None, 0) == -1
    assert call(p(v), len(v), p(f), 0, C.byref(info), None, 0, None, 0) == -1
    assert call(p(v), len(v) - 1, p(f), len(f), C.byref(info), None, 0, None, 0) == -1          # a face index past nv
    assert L().rt_last_error() == b"rt_device_lbvh_build: face index 7 >= nv"
    bad = capi.DeviceBvhInfo(struct_size=C.sizeof(capi.DeviceBvhInfo) + 4)
    assert call(p(v), len(v), p(f), len(f), C.byref(bad), None, 0, None, 0) == -1
    assert L().rt_last_error() == b"rt_device_lbvh_build: rt_device_bvh_info.struct_size is 44, this library's is 40"
    assert info.n_nodes == 0 and info.n_slots == 0                                              # a refused call writes nothing
    assert call(p(v), len(v), p(f), len(f), C.byref(info), None, 0, None, 0) == 0               # sizes only
    assert (info.n_nodes, info.n_slots, info.root_ref) == (1, 5, 0)
    assert (info.bvh_lds, info.bvh_spill, info.block) == (8, 32, 256)
    nodes, slots = np.full(1, 7, capi.DEVBVHNODE), np.full(5, 7, np.uint32)
    assert call(p(v), len(v), p(f), len(f), C.byref(info), p(nodes), 0, p(slots), 5) == -1
    assert L().rt_last_error() == b"rt_device_lbvh_build: room for 0 node records, 1 needed"
    assert call(p(v), len(v), p(f), len(f), C.byref(info), p(nodes), 1, p(slots), 4) == -1
    assert L().rt_last_error() == b"rt_device_lbvh_build: room for 4 triangle slots, 5 needed"
    assert (nodes["c"] == 7).all() and (slots == 7).all()
    assert call(p(v), len(v), p(f), len(f), C.byref(info), p(nodes), 1, None, 0) == 0           # either buffer alone
    assert call(p(v), len(v), p(f), len(f), C.byref(info), None, 0, p(slots), 5) == 0
    assert sorted(slots) == [0, 1, 2, 3, 4] and not nodes["pad"].any()


def _faces_beneath(nodes, slot_face, ref, memo):
    return R._faces_beneath(nodes, slot_face, ref, memo)


@pytest.mark.parametrize("name", NAMES)
def test_structure(name):
    v, f = lbvh_ref.meshes()[name]
    info, nodes, slot_face = _mirror(name)
    nf = len(f)
    assert info.n_slots == nf and sorted(slot_face) == list(range(nf))                         # a permutation
    if nf <= 4:
        assert info.n_nodes == 0 and info.root_ref == lbvh_ref.leafref(0, nf) and info.stack_need == 0
        return
    assert info.root_ref == 0 and info.n_nodes == len(nodes) > 0
    assert info.stack_need == bvh_walk.exact_stack_need(nodes, info.root_ref)                   # (also: every record reached exactly once)
    unused = np.isnan(nodes["lo"][:, 0, :])
    for k in ("lo", "hi"):
        assert (np.isnan(nodes[k]) == unused[:, None, :]).all()
    assert (nodes["c"][unused] == lbvh_ref.leafref(0, 1)).all() and not nodes["pad"].any()
    assert (~unused).sum(1).min() >= 2 and not unused[:, :2].any()
    # leaves: 1..4 contiguous slots, together every slot once; numbering: the internal refs in (record, child) order are 1, 2, 3, ...
    refs = nodes["c"][~unused]                                                                  # row-major: by record, then child position
    leaf = (refs & lbvh_ref.LEAF) != 0
    first, cnt = (refs[leaf] & 0x0FFFFFFF).astype(np.int64), ((refs[leaf] >> 28) & 7).astype(np.int64) + 1
    assert cnt.max() <= 4 and cnt.sum() == nf
    covered = np.zeros(nf, np.int64)
    for a, c in zip(first, cnt):
        covered[a:a + c] += 1
    assert (covered == 1).all()
    assert refs[~leaf].tolist() == list(range(1, len(nodes)))                                   # breadth-first, every record referenced once
    # leaves are maximal: the faces beneath an internal child are more than four
    memo = {}
    for i in range(len(nodes)):
        for ch in np.nonzero(~unused[i])[0]:
            ref = int(nodes["c"][i][ch])
            faces = _faces_beneath(nodes, slot_face, ref, memo)
            assert (len(faces) > 4) == (not ref & lbvh_ref.LEAF), (i, ch)
            p = v[f[faces]].reshape(-1, 3)
            assert (nodes["lo"][i][:, ch] == p.min(0)).all() and (nodes["hi"][i][:, ch] == p.max(0)).all(), (i, ch)


@pytest.mark.parametrize("name", NAMES)
def test_mirror_is_the_independent_transcription(name):
    v, f = lbvh_ref.meshes()[name]
    info, nodes, slot_face = _mirror(name)
    want_nodes, want_slots, root_ref, need, level_off = lbvh_ref.build(v, f)
    lbvh_ref.same_tree(nodes, slot_face, want_nodes, want_slots, name)
    assert (info.root_ref, info.stack_need, info.n_nodes) == (root_ref, need, len(want_nodes))


def test_deformed_meshes_too():
    """the vertices the GPU tests build from"""
    for name in R.MESHES:
        v, f = R._deformed(name), R._mesh(name)[1]
        info, nodes, slot_face = capi.device_lbvh_build(v, f)
        want = lbvh_ref.build(v, f)
        lbvh_ref.same_tree(nodes, slot_face, want[0], want[1], name)
        assert (info.root_ref, info.stack_need) == want[2:4]


@pytest.mark.parametrize("name", R.MESHES)
def test_hits_through_the_mirrors_tree(name):
    """bvh_walk.walk over the mirror's tree of the deformed mesh ends, for both triangle models, on the face and at the distance a
    float32 brute force over all triangles gives (tests/test_mesh_refit.py's qualification: rays with two triangles at a bit-equal
    closest t are left out, at most 1 % of the seeded rays); for the two-sided model the float64 Moeller-Trumbore of
    bvh_walk.brute_force agrees: a face that must be hit is, and the face hit may be."""
    v, f = R._deformed(name), R._mesh(name)[1]
    info, nodes, slot_face = capi.device_lbvh_build(v, f)
    root_box = np.concatenate([v[f].reshape(-1, 3).min(0), v[f].reshape(-1, 3).max(0)])
    for model in (capi.SHADE_FIN, capi.SHADE_P13):
        ties, face, t, p, d = R._qualified(name, model)
        ok = ties <= 1
        assert (~ok).sum() * 100 <= len(ok), (name, model, int((~ok).sum()))
        rays = np.concatenate([p, d], 1)
        _, got_face, got_t = bvh_walk.walk(v, f, nodes, slot_face, info.root_ref, root_box, rays, model=0 if model == capi.SHADE_FIN else 1)
        assert (got_face[ok] == face[ok]).all(), (name, model)
        hit = ok & (face >= 0)
        assert hit.sum() >= len(ok) // 4 and (got_t[hit] == t[hit]).all(), (name, model)
        if model == capi.SHADE_FIN:
            sub = np.nonzero(ok)[0][:512]
            may, must = bvh_walk.brute_force(v, f, rays[sub])
            g = got_face[sub]
            assert (g[np.isfinite(must).any(1)] >= 0).all()
            assert np.isfinite(may[np.nonzero(g >= 0)[0], g[g >= 0]]).all()


def test_mirror_under_sanitizers(tmp_path):
    """tests/lbvh_mirror_driver.cpp: csrc/rt_lbvh.h compiled alone by g++ with -fsanitize=address,undefined (no HIP, no library,
    nothing preloaded) and run as a program of its own over the awkward meshes, the coincident triangles and the root leaf: clean,
    and the library's record count, stack_need and bytes"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "lbvh_mirror_driver")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", exe, os.path.join(root, "tests", "lbvh_mirror_driver.cpp")], check=True)
    for name in [n for n in NAMES if n.startswith("awkward_")] + ["coincident64", "tri3", "strip5"]:
        v, f = lbvh_ref.meshes()[name]
        path = tmp_path / (name + ".bin")
        with open(path, "wb") as o:
            o.write(np.array([len(v), len(f)], np.uint32).tobytes() + np.ascontiguousarray(v, F).tobytes() + np.ascontiguousarray(f, np.uint32).tobytes())
        out = subprocess.run([exe, str(path), str(tmp_path / (name + ".out"))], capture_output=True, text=True)
        assert out.returncode == 0 and out.stderr == "", (name, out.stderr[-2000:])
        info, nodes, slot_face = _mirror(name)
        assert out.stdout.split() == [str(info.n_nodes), str(info.root_ref), str(info.stack_need)], (name, out.stdout)
        assert open(tmp_path / (name + ".out"), "rb").read() == nodes.tobytes() + slot_face.tobytes(), name


def test_lbvh_cost_against_the_host_tree():
    """the figure DESIGN.md section 3 records: the SAH cost of the mirror's tree over the cost of the host's binned-SAH tree, on the
    teapot.  An LBVH is the worse tree; how much worse is printed, and bounded only by reason: not better than 0.9 of the SAH
    tree's cost (binned SAH is a greedy heuristic, not an optimum) and not 3 times worse (Morton order is spatially coherent)."""
    v, f = lbvh_ref.meshes()["teapot"]
    info, nodes, _ = _mirror("teapot")
    s = R._scene("teapot")
    hn, _, hinfo = s.mesh_device_bvh(0)
    lb, sah = capi.device_bvh_cost(nodes, info.root_ref)[0], capi.device_bvh_cost(hn, hinfo.root_ref)[0]
    print(f"[lbvh] teapot: LBVH cost {lb:.3f}, SAH cost {sah:.3f}, ratio {lb / sah:.3f}; stack_need {info.stack_need} against {hinfo.stack_need}")
    assert 0.9 < lb / sah < 3.0
