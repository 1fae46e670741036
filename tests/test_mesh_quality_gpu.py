"""Mesh tree quality on the GPU (include/rt_mi355x.h, "mesh tree quality"): k_bvh_cost in csrc/rt_refit.hip through
Scene.mesh_quality, and the update that acts on it, Scene.update_mesh_vertices(..., max_ratio=) (rt_scene_update_mesh_vertices_auto).

Two references.  The host mirror capi.device_bvh_cost on the records read back from the device must give the GPU's cost BIT FOR
BIT: the definition fixes the order of every addition for exactly that.  The yardstick of tests/bvh_cost_ref.py (float32 terms,
math.fsum) is independent of both and holds at 1e-9 relative.  What the update leaves on the device is held against a second scene
given the same vertices through the old call, byte for byte, and the hits against a fresh scene's.

Meshes, deformation and rays are those of tests/test_mesh_refit.py (the rays are the first 256 of its 4096 per mesh, which its CPU
part qualifies: no two triangles at a bit-equal closest distance).  tests/test_bvh_cost_host.py checks without a GPU that the
deformation loosens every tree by more than 5 %; the policy test asserts it again on the device's own refit."""
import ctypes as C
import struct

import numpy as np
import pytest

from raytracing_folder_amd import capi
from tests import bvh_cost_ref
from tests import test_mesh_refit as refit_meshes

MESHES = refit_meshes.MESHES
L = capi.lib
_mesh, _scene, _deformed = refit_meshes._mesh, refit_meshes._scene, refit_meshes._deformed
N_RAYS = 256

pytestmark = pytest.mark.gpu


def _bits(x):
    return struct.pack("<d", x)


def _mirror(read):
    cost, degenerate = capi.device_bvh_cost(read["nodes"], read["info"].root_ref)
    assert not degenerate
    return cost


def _yardstick(read):
    return bvh_cost_ref.sah_cost(read["nodes"], read["info"].root_ref)


def _close(got, want):
    assert want is not None and abs(got - want) <= bvh_cost_ref.RTOL * want, (got, want)


def _plain(q):
    assert not (q["degenerate"] or q["rebuilt"] or q["not_on_device"]), q


def _levels(name):
    """the number of levels of the tree the host builds for the mesh (a node's index is above its parent's)"""
    nodes, _, info = _scene(name).mesh_device_bvh(0)
    if info.root_ref & capi.DEVBVH_LEAF:
        return 0
    depth = {int(info.root_ref): 0}
    for i in range(len(nodes)):
        for c in nodes["c"][i][~np.isnan(nodes["lo"][i][0])]:
            if not int(c) & capi.DEVBVH_LEAF:
                depth[int(c)] = depth[i] + 1
    return max(depth.values()) + 1


@pytest.mark.parametrize("name", MESHES)
def test_gpu_cost_is_the_host_mirror_bit_for_bit(name):
    s = _scene(name)
    q = s.mesh_quality(0)
    read = s.mesh_device_read(0)
    print(f"[quality] {name}: cost {q['cost']!r}, mirror {_mirror(read)!r}, yardstick {_yardstick(read)!r}, {q['measure_ms']:.4f} ms")
    _plain(q)
    assert _bits(q["cost"]) == _bits(_mirror(read))
    _close(q["cost"], _yardstick(read))
    assert q["ratio"] == 1.0 and _bits(q["built_cost"]) == _bits(q["cost"])
    assert q["measure_ms"] >= 0.0
    if name == "tri3":
        assert q["cost"] == 4.0


@pytest.mark.parametrize("name", MESHES)
def test_an_update_that_moves_nothing(name):
    v = _mesh(name)[0]
    s = _scene(name)
    before = s.mesh_device_read(0)
    q = s.update_mesh_vertices(0, v, max_ratio=1e9)
    _plain(q)
    assert q["ratio"] == 1.0 and _bits(q["cost"]) == _bits(q["built_cost"]) == _bits(_mirror(before))
    assert s.mesh_device_read(0)["nodes"].tobytes() == before["nodes"].tobytes()


@pytest.mark.parametrize("name", MESHES)
def test_cost_after_a_deformation(name):
    dv = _deformed(name)
    s = _scene(name)
    built = s.mesh_quality(0)["built_cost"]
    before = s.mesh_device_read(0)["nodes"]
    q = s.update_mesh_vertices(0, dv, max_ratio=1e9)
    read = s.mesh_device_read(0)
    print(f"[quality] {name}: refitted cost {q['cost']!r}, built {q['built_cost']!r}, ratio {q['ratio']!r}, {q['measure_ms']:.4f} ms")
    _plain(q)
    assert _bits(q["cost"]) == _bits(_mirror(read))
    _close(q["cost"], _yardstick(read))
    assert _bits(q["built_cost"]) == _bits(built)
    assert _bits(q["ratio"]) == _bits(q["cost"] / q["built_cost"])
    again = s.mesh_quality(0)                                        # a second launch on the same records: the same bytes
    _plain(again)
    for k in ("cost", "built_cost", "ratio"):
        assert _bits(again[k]) == _bits(q[k]), k
    old = _scene(name)                                               # the same update through the old call
    old.mesh_device_read(0)
    assert old.update_mesh_vertices(0, dv) is None
    refit_meshes._same(read, old.mesh_device_read(0), name)
    if name != "tri3":
        assert q["ratio"] > 1.0 and read["nodes"].tobytes() != before.tobytes()
    else:
        assert q["ratio"] == 1.0 and q["cost"] == 4.0


@pytest.mark.parametrize("name", MESHES)
def test_the_policy(name):
    """the deformation is 0.3 of the extent at phase 0.3 for every mesh: each tree but tri3's loosens by far more than 5 % (the
    teapot to 2.85, strip5 to 1.47, the tower to 6.07 of its built cost), so no mesh needs a larger amplitude.

    That an update below max_ratio did NOT build the tree again shows in three ways: the nodes are byte for byte the old call's
    refit; a following mesh_quality() still has the old built_cost and the measured ratio (after a rebuild: a new built_cost, ratio
    1); and the nodes differ from a fresh build's for the new vertices.  The last holds for the teapot and the tower only: strip5
    is ONE node whose two leaves a fresh build of the deformed strip forms again, so its refitted record IS the fresh build's, byte
    for byte, and cannot differ from it (measured: identical)."""
    dv = _deformed(name)
    old = _scene(name)
    built_nodes = old.mesh_device_read(0)
    old.update_mesh_vertices(0, dv)
    refitted = old.mesh_device_read(0)
    if name == "tri3":                                               # one leaf: 1 + 3 whatever the vertices
        s = _scene(name)
        s.mesh_device_read(0)
        q = s.update_mesh_vertices(0, dv, max_ratio=1.0)
        _plain(q)
        assert q["ratio"] == 1.0 and q["cost"] == q["built_cost"] == 4.0
        refit_meshes._same(s.mesh_device_read(0), refitted, name)
        return
    measured = _yardstick(refitted) / _yardstick(built_nodes)
    print(f"[quality] {name}: yardstick ratio of the refit {measured:.6f}")
    assert measured > 1.05, measured

    s = _scene(name)                                                 # max_ratio 1.0: rebuilt
    built = s.mesh_quality(0)["built_cost"]
    q = s.update_mesh_vertices(0, dv, max_ratio=1.0)
    assert q["rebuilt"] and not q["degenerate"] and not q["not_on_device"]
    assert _bits(q["cost"]) == _bits(_mirror(refitted)) and _bits(q["built_cost"]) == _bits(built)       # the refitted tree's cost, the one that triggered it
    _close(q["ratio"], measured)
    fresh_nodes, _, fresh_info = s.mesh_device_bvh(0)
    assert s.mesh_device_read(0)["nodes"].tobytes() == fresh_nodes.tobytes()
    after = s.mesh_quality(0)
    _plain(after)
    assert after["ratio"] == 1.0 and _bits(after["built_cost"]) == _bits(after["cost"]) == _bits(capi.device_bvh_cost(fresh_nodes, fresh_info.root_ref)[0])
    assert after["built_cost"] != built

    s = _scene(name)                                                 # just above the measured ratio: the refitted tree stays
    s.mesh_device_read(0)
    q = s.update_mesh_vertices(0, dv, max_ratio=measured * 1.01)
    _plain(q)
    _close(q["ratio"], measured)
    got = s.mesh_device_read(0)
    assert got["nodes"].tobytes() == refitted["nodes"].tobytes()
    after = s.mesh_quality(0)
    _plain(after)
    assert _bits(after["built_cost"]) == _bits(q["built_cost"]) and _bits(after["ratio"]) == _bits(q["ratio"]) and after["ratio"] > 1.05
    same_as_fresh = got["nodes"].tobytes() == s.mesh_device_bvh(0)[0].tobytes()
    print(f"[quality] {name}: refitted nodes equal a fresh build's: {same_as_fresh}")
    assert same_as_fresh == (name == "strip5")


@pytest.mark.parametrize("name", MESHES)
def test_hits_after_an_auto_update_are_the_fresh_scenes(name):
    dv, rays = _deformed(name), refit_meshes._rays(name)[:N_RAYS]
    fresh = _scene(name, dv)
    want = {model: fresh.trace_rays(rays, model) for model in (capi.SHADE_FIN, capi.SHADE_P13)}
    assert want[capi.SHADE_FIN]["hit"].sum() >= N_RAYS // 4
    for max_ratio, rebuilt in ((1.0, name != "tri3"), (1e9, False)):
        s = _scene(name)
        s.mesh_device_read(0)
        q = s.update_mesh_vertices(0, dv, max_ratio=max_ratio)
        assert q["rebuilt"] == rebuilt and not q["not_on_device"], (max_ratio, q)
        for model, b in want.items():
            a = s.trace_rays(rays, model)
            for k in ("hit", "z", "p", "N", "node", "front"):
                assert a[k].tobytes() == b[k].tobytes(), (max_ratio, model, k)


def test_argument_errors_change_nothing_on_the_device():
    v, f, vn, fn = _mesh("strip5")
    dv = _deformed("strip5")
    s = _scene("strip5")
    before = s.mesh_device_read(0)
    p, auto, quality = capi._p, L().rt_scene_update_mesh_vertices_auto, L().rt_scene_mesh_quality
    q = capi.MeshQuality(struct_size=C.sizeof(capi.MeshQuality) + 8)
    assert quality(s._h, 0, 0, C.byref(q)) == -1
    assert L().rt_last_error() == b"rt_scene_mesh_quality: rt_mesh_quality.struct_size is 48, this library's is 40"
    assert auto(s._h, 0, p(dv), len(dv), None, 0, 2.0, C.byref(q)) == -1
    assert L().rt_last_error() == b"rt_scene_update_mesh_vertices_auto: rt_mesh_quality.struct_size is 48, this library's is 40"
    q = capi.MeshQuality(struct_size=C.sizeof(capi.MeshQuality))
    assert quality(s._h, 0, 7, C.byref(q)) == -1                      # a mesh never set
    assert L().rt_last_error() == b"rt_scene_mesh_quality: mesh 7 was never set"
    assert auto(s._h, 7, p(dv), len(dv), None, 0, 2.0, C.byref(q)) == -1
    assert L().rt_last_error() == b"rt_scene_update_mesh_vertices_auto: mesh 7 was never set"
    for bad in (float("nan"), 0.5, float("inf")):
        assert auto(s._h, 0, p(dv), len(dv), None, 0, bad, C.byref(q)) == -1
        assert L().rt_last_error().startswith(b"rt_scene_update_mesh_vertices_auto: max_ratio is ")
    assert quality(None, 0, 0, C.byref(q)) == -1                      # a NULL scene, a NULL result
    assert L().rt_last_error() == b"rt_scene_mesh_quality: NULL argument"
    assert quality(s._h, 0, 0, None) == -1
    assert auto(None, 0, p(dv), len(dv), None, 0, 2.0, C.byref(q)) == -1
    assert L().rt_last_error() == b"rt_scene_update_mesh_vertices_auto: scene is NULL"
    for nv in (len(dv) - 1, len(dv) + 1):                             # nv mismatch
        assert auto(s._h, 0, p(dv), nv, None, 0, 2.0, C.byref(q)) == -1
        assert L().rt_last_error().startswith(b"rt_scene_update_mesh_vertices_auto: nv is ")
    assert auto(s._h, 0, p(dv), len(dv), p(vn), len(vn) - 1, 2.0, C.byref(q)) == -1
    assert L().rt_last_error().startswith(b"rt_scene_update_mesh_vertices_auto: nvn is ")
    refit_meshes._same(s.mesh_device_read(0), before, "strip5")
    assert s.export()["meshes"][0]["v"].tobytes() == v.tobytes()
    good = s.mesh_quality(0)
    _plain(good)
    assert good["ratio"] == 1.0


@pytest.mark.parametrize("name", MESHES)
def test_the_old_call_is_the_old_call(name):
    dv = _deformed(name)
    s = _scene(name)
    s.mesh_device_read(0)
    assert s.update_mesh_vertices(0, dv) is None
    assert s.mesh_update_ms()["level_launches"] == _levels(name)
    q = s.update_mesh_vertices(0, dv, max_ratio=1e9)                  # the new entry point refits with the same launches
    _plain(q)
    assert s.mesh_update_ms()["level_launches"] == _levels(name)
