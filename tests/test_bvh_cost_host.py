"""rt_device_bvh_cost, the host mirror of k_bvh_cost (include/rt_mi355x.h, "mesh tree quality"), against the yardstick of
tests/bvh_cost_ref.py -- float32 terms in the stated order, summed exactly by math.fsum, which is not the library's fixed order --
at 1e-9 relative (the bound is derived there).  No GPU: the records are those Scene.mesh_device_bvh builds on the host.

Meshes: the four of tests/test_mesh_refit.py.  tri3's root is a leaf; strip5 is one node; the tower ("deep") has nine levels but
only 15 node records, 60 terms: ONE block of 256.  More than one block, and a short last one, is what the teapot covers (918
records, 3672 terms: 14 blocks and 88 terms), and the clustered soup of tests/deep_meshes.py beside it (435 records whose areas
span 2^80: the sum's worst case for a fixed order)."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from raytracing_folder_amd import capi, workloads
from tests import bvh_cost_ref, deep_meshes
from tests import test_mesh_refit as refit_meshes

MESHES = refit_meshes.MESHES
L = capi.lib

_cache = {}


def _tree(name):
    if name not in _cache:
        if name == "soup":
            s, _ = deep_meshes.mesh_scene(*deep_meshes.clustered_soup(3000))
        else:
            s = refit_meshes._scene(name)
        nodes, slot_face, info = s.mesh_device_bvh(0)
        _cache[name] = nodes, slot_face, int(info.root_ref)
    return _cache[name]


def _close(got, want):
    assert want is not None and abs(got - want) <= bvh_cost_ref.RTOL * want, (got, want)


def test_symbols_are_exported():
    for name in ("rt_device_bvh_cost", "rt_scene_mesh_quality", "rt_scene_update_mesh_vertices_auto"):
        assert hasattr(L(), name) and name in capi.SYMBOLS, name
    assert C.sizeof(capi.MeshQuality) == 40


@pytest.mark.parametrize("name", MESHES + ("soup",))
def test_host_mirror_matches_the_yardstick(name):
    nodes, _, root_ref = _tree(name)
    cost, degenerate = capi.device_bvh_cost(nodes, root_ref)
    want = bvh_cost_ref.sah_cost(nodes, root_ref)
    print(f"[bvh cost] {name}: {len(nodes)} records, mirror {cost!r}, yardstick {want!r}")
    assert not degenerate
    _close(cost, want)
    if name == "tri3":
        assert len(nodes) == 0 and cost == 1.0 + 3.0
    if name in ("teapot", "soup"):
        assert 4 * len(nodes) > 256 and (4 * len(nodes)) % 256 != 0          # several blocks, the last one short


@pytest.mark.parametrize("name", [n for n in MESHES if n != "tri3"])
def test_host_mirror_on_a_refitted_tree(name):
    """the deformation of the GPU tests, refitted on the host: the mirror follows the yardstick there too, and the tree has
    loosened by more than 5 % -- what tests/test_mesh_quality_gpu.py's policy cases rely on"""
    nodes, slot_face, root_ref = _tree(name)
    v, f = refit_meshes._mesh(name)[:2]
    moved = bvh_cost_ref.refit(nodes, slot_face, refit_meshes._deformed(name), f)
    cost, degenerate = capi.device_bvh_cost(moved, root_ref)
    assert not degenerate
    _close(cost, bvh_cost_ref.sah_cost(moved, root_ref))
    ratio = bvh_cost_ref.sah_cost(moved, root_ref) / bvh_cost_ref.sah_cost(nodes, root_ref)
    print(f"[bvh cost] {name}: refitted at 0.3 of the extent, ratio {ratio:.4f}")
    assert ratio > 1.05, ratio


def test_a_nan_child_drops_exactly_its_term():
    nodes, _, root_ref = _tree("strip5")
    t = bvh_cost_ref.terms(nodes).astype(np.float64)
    used = np.nonzero(~np.isnan(nodes["lo"][0][0]))[0]
    assert len(used) == 2 and (t[0][used] > 0).all()
    HR = float(bvh_cost_ref.root_half_area(nodes, root_ref))
    full, _ = capi.device_bvh_cost(nodes, root_ref)
    _close(full, 1.0 + (t[0][used[0]] + t[0][used[1]]) / HR)
    for drop, keep in ((used[0], used[1]), (used[1], used[0])):
        cut = nodes.copy()
        cut["lo"][0][:, drop] = np.nan
        cut["hi"][0][:, drop] = np.nan
        cost, degenerate = capi.device_bvh_cost(cut, root_ref)
        # the root box is now the kept child's alone: S is its one term, H_R its own half area (its weight is the leaf's count)
        HR = float(bvh_cost_ref.root_half_area(cut, root_ref))
        assert not degenerate and cost == 1.0 + t[0][keep] / HR
        _close(cost, bvh_cost_ref.sah_cost(cut, root_ref))


def test_a_root_box_without_extent_is_degenerate():
    nodes, _, root_ref = _tree("strip5")
    flat = nodes.copy()
    used = ~np.isnan(nodes["lo"][0][0])
    flat["lo"][0][:, used] = 1.5
    flat["hi"][0][:, used] = 1.5
    assert capi.device_bvh_cost(flat, root_ref) == (0.0, True)
    assert bvh_cost_ref.sah_cost(flat, root_ref) is None
    huge = nodes.copy()                                   # areas beyond float32: S and H_R are infinite
    huge["hi"][0][:, used] = 3.0e38
    huge["lo"][0][:, used] = -3.0e38
    assert capi.device_bvh_cost(huge, root_ref) == (0.0, True)
    none = nodes.copy()                                   # a root without a used child has no box
    none["lo"][0][:], none["hi"][0][:] = np.nan, np.nan
    assert capi.device_bvh_cost(none, root_ref) == (0.0, True)


def test_abi_errors():
    nodes, _, root_ref = _tree("strip5")
    cost, flags = C.c_double(-1.0), C.c_uint32(77)
    p = capi._p
    assert L().rt_device_bvh_cost(p(nodes), len(nodes), root_ref, None, C.byref(flags)) == -1
    assert L().rt_last_error() == b"rt_device_bvh_cost: NULL argument"
    assert L().rt_device_bvh_cost(p(nodes), len(nodes), root_ref, C.byref(cost), None) == -1
    assert L().rt_device_bvh_cost(None, len(nodes), root_ref, C.byref(cost), C.byref(flags)) == -1
    assert L().rt_last_error() == b"rt_device_bvh_cost: nodes is NULL"
    assert L().rt_device_bvh_cost(p(nodes), len(nodes), len(nodes), C.byref(cost), C.byref(flags)) == -1      # the first index past the records
    assert L().rt_last_error() == b"rt_device_bvh_cost: root_ref names node 1 of 1"
    assert L().rt_device_bvh_cost(p(nodes), 0, 0, C.byref(cost), C.byref(flags)) == -1
    assert (cost.value, flags.value) == (-1.0, 77)        # a refused call writes nothing
    leaf = capi.DEVBVH_LEAF | (2 << 28) | 5               # a leaf ref needs no records at all
    assert L().rt_device_bvh_cost(None, 0, leaf, C.byref(cost), C.byref(flags)) == 0 and (cost.value, flags.value) == (4.0, 0)


def test_mirror_arithmetic_compiled_alone(tmp_path):
    """tests/bvh_cost_mirror.cpp: csrc/rt_bvh_cost.h compiled alone by g++ (no HIP, no library) and run as a program of its own on
    the records of every mesh, written to a file: another compiler, the library's eight bytes.  (The same program is what a
    host-only run under -fsanitize=address,undefined uses: add the flag to this line.)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "bvh_cost_mirror")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-o", exe, os.path.join(root, "tests", "bvh_cost_mirror.cpp")], check=True)
    for name in MESHES + ("soup",):
        nodes, _, root_ref = _tree(name)
        records = tmp_path / (name + ".bin")
        records.write_bytes(nodes.tobytes())
        out = subprocess.run([exe, str(records), str(root_ref)], capture_output=True, text=True)
        assert out.returncode == 0 and out.stderr == "", (name, out.stderr)
        cost, degenerate = capi.device_bvh_cost(nodes, root_ref)
        assert out.stdout.split() == [struct.pack(">d", cost).hex(), "1" if degenerate else "0"], (name, out.stdout)
    out = subprocess.run([exe, str(tmp_path / "strip5.bin"), "1"], capture_output=True, text=True)      # a root past the records
    assert out.returncode == 0 and out.stderr == "" and out.stdout.strip() == "bad root"


def test_update_with_max_ratio_on_a_scene_never_lowered():
    """no device holds the scene: nothing to refit or measure, the store has the new vertices, and the arguments are checked"""
    v, f, vn, fn = refit_meshes._mesh("strip5")
    dv = refit_meshes._deformed("strip5")
    s = refit_meshes._scene("strip5")
    q = s.update_mesh_vertices(0, dv, max_ratio=1.5)
    assert q == dict(cost=0.0, built_cost=0.0, ratio=1.0, measure_ms=0.0, degenerate=False, rebuilt=False, not_on_device=True)
    assert s.export()["meshes"][0]["v"].tobytes() == dv.tobytes()
    assert s.update_mesh_vertices(0, v) is None
    with pytest.raises(ValueError):
        s.update_mesh_vertices(0, dv, rebuild=True, max_ratio=1.5)
    before = s.export()["meshes"][0]
    p, auto = capi._p, L().rt_scene_update_mesh_vertices_auto
    for bad in (float("nan"), 0.5, float("inf"), -1.0):
        assert auto(s._h, 0, p(dv), len(dv), None, 0, bad, None) == -1
        assert L().rt_last_error().startswith(b"rt_scene_update_mesh_vertices_auto: max_ratio is ")
    q = capi.MeshQuality(struct_size=C.sizeof(capi.MeshQuality) + 8)
    assert auto(s._h, 0, p(dv), len(dv), None, 0, 2.0, C.byref(q)) == -1
    assert L().rt_last_error() == b"rt_scene_update_mesh_vertices_auto: rt_mesh_quality.struct_size is 48, this library's is 40"
    assert auto(s._h, 0, p(dv), len(dv) - 1, None, 0, 2.0, None) == -1
    assert L().rt_last_error().startswith(b"rt_scene_update_mesh_vertices_auto: nv is 7")
    assert auto(s._h, 0, p(dv), len(dv), p(vn), len(vn) + 1, 2.0, None) == -1
    assert auto(s._h, 5, p(dv), len(dv), None, 0, 2.0, None) == -1
    assert L().rt_last_error() == b"rt_scene_update_mesh_vertices_auto: mesh 5 was never set"
    assert auto(s._h, 0, None, len(dv), None, 0, 2.0, None) == -1
    assert auto(None, 0, p(dv), len(dv), None, 0, 2.0, None) == -1
    assert L().rt_last_error() == b"rt_scene_update_mesh_vertices_auto: scene is NULL"
    after = s.export()["meshes"][0]
    for k in ("v", "f", "vn", "fn", "nodes", "elements"):
        assert before[k].tobytes() == after[k].tobytes(), k
    assert auto(s._h, 0, p(dv), len(dv), None, 0, 1.0, None) == 0                 # out may be NULL
    assert s.export()["meshes"][0]["v"].tobytes() == dv.tobytes()
