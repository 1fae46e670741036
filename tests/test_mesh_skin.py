"""Mesh skinning on the device (include/rt_mi355x.h, "mesh skinning": k_mesh_pose in csrc/rt_mesh_pose.hip behind the four
rt_scene_pose_mesh* entry points).  Two yardsticks, neither of them the code under test: the host mirror's positions (which
tests/test_mesh_skin_host.py holds against an independent transcription of the definition) given to a FRESH scene through set_mesh
-- with capi.mesh_smooth_normals of them where the mode is SMOOTH -- and the same positions driven through update_mesh_vertices
with the same arguments.  Every comparison is byte equality.

Meshes, rigs and poses are tests/test_mesh_skin_host.py's; the scene is tests/test_mesh_normals.py's.  Rays with two triangles at
a bit-equal closest t (the one thing that may depend on the tree: a refitted tree against a fresh one) are left out, as in
tests/test_mesh_refit.py."""
import numpy as np
import pytest

from raytracing_folder_amd import capi
from tests import test_mesh_normals as nrm
from tests import test_mesh_refit as refit
from tests import test_mesh_skin_host as host

F = np.float32
N_RAYS = 1024
READ = ("nodes", "slot_face", "tris", "nrm", "root_box")
FRAME_PLANES = ("normal", "albedo", "object_id")
_cache = {}


def _skinned(name, rig_name, mode="stored", lower=True):
    s = nrm._scene(name)
    idx, w, n = host.rig(name, rig_name)
    s.set_mesh_skin(0, idx, w, n)
    s.set_mesh_normals(0, mode)
    if lower:
        s.mesh_device_read(0)
    return s, n


def _fresh(name, v, mode):
    _, f, vn, fn = nrm._mesh(name)
    return nrm._scene(name, v, capi.mesh_smooth_normals(v, f, fn, vn) if mode == "smooth" else vn)


def _same_read(a, b, what, keys=READ):
    for k in keys:
        assert a[k].tobytes() == b[k].tobytes(), (what, k)


def _rays(name, key, v):
    """1024 seeded rays at the mesh with positions v, and which of them are qualified (tests/test_mesh_normals.py's recipe)"""
    if ("rays", name, key) not in _cache:
        dv, f = v.astype(np.float64), nrm._mesh(name)[1]
        rng = np.random.default_rng(11)
        pick = rng.integers(0, len(f), N_RAYS)
        w = rng.uniform(0.08, 1.0, (N_RAYS, 3))
        w /= w.sum(1, keepdims=True)
        tgt = refit._to_world((dv[f][pick] * w[:, :, None]).sum(1))
        centre, ext = refit._to_world(dv.mean(0)[None])[0], nrm._extent(dv)
        tgt[::8] += rng.normal(size=(len(tgt[::8]), 3)) * ext
        d = rng.normal(size=(N_RAYS, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        o = centre + 3.0 * ext * d
        rays = np.concatenate([o, (tgt - o) * rng.uniform(1.2, 2.0, (N_RAYS, 1))], 1).astype(F)
        p, dd = refit._to_mesh(rays, nrm._scene(name).get_nodes())
        ok = np.ones(N_RAYS, bool)
        for model in (capi.SHADE_FIN, capi.SHADE_P13):
            ok &= refit._closest(v, f, p, dd, model)[0] <= 1
        _cache["rays", name, key] = rays, ok
    return _cache["rays", name, key]


def _frame(s, name):
    """64 x 48 at 4 samples a pixel, reproducible, looking at mesh 0 from 1.6 extents away"""
    v = nrm._mesh(name)[0].astype(np.float64)
    centre, ext = refit._to_world(v.mean(0)[None])[0], nrm._extent(v)
    pos = centre + 1.6 * ext * np.array([0.3, 0.2, 0.93])
    d = (centre - pos) / np.linalg.norm(centre - pos)
    cam = capi.Camera()
    cam.pos[:], cam.dir[:], cam.up[:] = tuple(pos), tuple(d), (0.0, 1.0, 0.0)
    cam.fov, cam.focaldist, cam.dof, cam.width, cam.height = 40.0, 1.0, 0.0, 64, 48
    s.set_render_flags(capi.RENDER_REPRODUCIBLE)
    return s.render_outputs(cam, capi.default_params(min_sample=4, max_sample=4, threshold=-1.0), FRAME_PLANES)


def _same_frame(a, b, what):
    for k in ("rgb", "z", "count") + FRAME_PLANES:
        assert a[k].tobytes() == b[k].tobytes(), (what, k)


# ---- a pose against the fresh scene ----------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", ("stored", "smooth"))
@pytest.mark.parametrize("rig_name", ("chain3", "chain65"))
@pytest.mark.parametrize("name", ("sheet3", "teapot"))
def test_a_pose_is_the_fresh_scene(name, rig_name, mode):
    """after pose_mesh: slots, normals and root box are the fresh scene's (per face: the trees differ, one refitted, one built),
    the hits of 1024 rays and a frame with its planes too"""
    s, n = _skinned(name, rig_name, mode)
    with pytest.raises(capi.RtError) as e:
        s.mesh_skin_ms()
    assert e.value.status == -2
    assert s.pose_mesh(0, host.pose(name, n, "bend")) is None
    assert s.mesh_skin_ms() > 0.0 and s.mesh_skin(0)["store_current"] == 0
    posed = host.mirror(name, rig_name, "bend")
    fresh = _fresh(name, posed, mode)
    got, want = s.mesh_device_read(0), fresh.mesh_device_read(0)
    assert got["root_box"].tobytes() == want["root_box"].tobytes()
    ga, gb = nrm._by_face(got), nrm._by_face(want)
    assert ga[0].tobytes() == gb[0].tobytes() and ga[1].tobytes() == gb[1].tobytes()
    assert s.mesh_skin(0)["store_current"] == 0                       # reading the device asked the store for nothing
    rays, ok = _rays(name, rig_name, posed)
    assert ok.sum() >= N_RAYS * 3 // 4
    for model in (capi.SHADE_FIN, capi.SHADE_P13):
        a, b = s.trace_rays(rays, model), fresh.trace_rays(rays, model)
        assert b["hit"][ok].sum() >= N_RAYS // 4
        for k in ("hit", "z", "p", "N", "node", "front"):
            assert a[k][ok].tobytes() == b[k][ok].tobytes(), (model, k)
    fa, fb = _frame(s, name), _frame(fresh, name)
    assert (fb["object_id"] >= 0).sum() >= 64 * 48 // 16
    _same_frame(fa, fb, (name, rig_name, mode))
    m = nrm._get_mesh(s)                                              # ... and the store, once asked, agrees
    assert m["v"].tobytes() == posed.tobytes() and m["vn"].tobytes() == nrm._get_mesh(fresh)["vn"].tobytes()


# ---- every form of the pose against the same form of update_mesh_vertices ---------------------------------------------------
FORMS = {
    "plain": dict(),
    "rebuild": dict(rebuild=True),
    "auto_rebuilds": dict(max_ratio=1.0),
    "auto_keeps": dict(max_ratio=1.0e9),
    "device": dict(rebuild="device"),
    "device_auto": dict(rebuild="device", max_ratio=1.0),
    "device_fallback": dict(rebuild="device"),
    "keep_previous": dict(keep_previous=True),
}
FLAGS = ("rebuilt", "on_device", "fell_back", "not_on_device", "degenerate")


@pytest.mark.gpu
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name,rig_name,pose_name,mode", [("tri3", "half2", "shear", "smooth"), ("strip5", "loose", "shear", "stored"),
                                                          ("sheet3", "chain3", "bend", "smooth"), ("teapot", "chain1024", "bend", "smooth"),
                                                          ("teapot", "one", "shear", "stored")])
def test_every_form_leaves_what_the_update_leaves(name, rig_name, pose_name, mode, form, monkeypatch):
    """device state byte for byte (the trees are the same trees: the same refit, the same build), the same dict keys and flags"""
    if form == "device_fallback":
        monkeypatch.setenv("RT_LBVH_STACK_CAP", "0")
    s, n = _skinned(name, rig_name, mode)
    ref, _ = _skinned(name, rig_name, mode)
    posed = host.mirror(name, rig_name, pose_name)
    out = s.pose_mesh(0, host.pose(name, n, pose_name), **FORMS[form])
    want = ref.update_mesh_vertices(0, posed, **FORMS[form])
    if want is None:
        assert out is None
    else:
        assert set(out) == set(want) and {k: out[k] for k in FLAGS if k in out} == {k: want[k] for k in FLAGS if k in want}, (out, want)
        if "build" in want:
            assert {k: out["build"][k] for k in FLAGS if k in out["build"]} == {k: want["build"][k] for k in FLAGS if k in want["build"]}
        if "ratio" in want:
            assert out["ratio"] == want["ratio"] and out["cost"] == want["cost"]
    if form == "device_fallback":
        assert out["fell_back"] or len(nrm._mesh(name)[1]) <= 4, out
    _same_read(s.mesh_device_read(0), ref.mesh_device_read(0), (name, form))
    if form in ("device", "device_auto") and len(nrm._mesh(name)[1]) > 4:
        lbvh = capi.device_lbvh_build(posed, nrm._mesh(name)[1])
        got = s.mesh_device_read(0)
        assert got["nodes"].tobytes() == lbvh[1].tobytes() and got["slot_face"].tobytes() == lbvh[2].tobytes()
    a, b = s.mesh_device_previous(0), ref.mesh_device_previous(0)
    assert (a is None) == (b is None) == (form != "keep_previous") and (a is None or a.tobytes() == b.tobytes())
    assert nrm._get_mesh(s)["v"].tobytes() == posed.tobytes()


# ---- the bone cap ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_the_bone_cap_on_one_partial_workgroup():
    """strip5 -- eight vertices, one workgroup most of whose lanes only stage -- under a rig of 1024 bones, the cap: 48 KB of LDS
    staged for a pose with no morph target.  Every vertex blends bones 0, 1, 1022 and 1023 (the rest are unused); the device holds
    what update_mesh_vertices with the mirror's positions leaves, and the kernel did run (the store was asked for nothing)"""
    name, n = "strip5", capi.MESH_SKIN_MAX_BONES
    v = nrm._mesh(name)[0]
    i = np.arange(len(v))
    idx = np.tile(np.array([0, 1, n - 2, n - 1], np.uint16), (len(v), 1))
    w = np.stack([0.1 + 0.05 * (i % 3), 0.4 - 0.03 * i, 0.2 + 0.02 * i, 0.3 - 0.05 * (i % 3) + 0.01 * i], 1).astype(F)
    assert n == 1024 and (w > 0).all() and len(v) < 256
    bones = host.pose(name, n, "shear")
    posed = capi.mesh_skin(v, idx, w, bones)
    assert (posed != v).any()
    s, ref = nrm._scene(name), nrm._scene(name)
    s.set_mesh_skin(0, idx, w, n)
    for x in (s, ref):
        x.mesh_device_read(0)
    assert s.pose_mesh(0, bones) is None
    assert s.mesh_skin_ms() > 0.0 and s.mesh_skin(0)["store_current"] == 0
    ref.update_mesh_vertices(0, posed)
    _same_read(s.mesh_device_read(0), ref.mesh_device_read(0), name)
    assert s.mesh_skin(0)["store_current"] == 0
    assert nrm._get_mesh(s)["v"].tobytes() == posed.tobytes()


# ---- previous positions ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ("sheet3", "teapot"))
def test_keep_previous_swaps_and_the_motion_plane_follows(name):
    """two flagged poses: the device's previous positions are the first pose's mirror positions and the motion plane is the one
    update_mesh_vertices(keep_previous=True) with the two mirrors' positions gives; the store is asked for nothing on the way; a
    third pose without the flag releases them"""
    rig_name, mode = "chain65", "smooth"
    s, n = _skinned(name, rig_name, mode)
    ref, _ = _skinned(name, rig_name, mode)
    first, second = host.mirror(name, rig_name, "shear"), host.mirror(name, rig_name, "bend")
    for pose_name, posed in (("shear", first), ("bend", second)):
        s.pose_mesh(0, host.pose(name, n, pose_name), keep_previous=True)
        assert s.mesh_skin(0)["store_current"] == 0 and s.previous_positions() == 1
        ref.update_mesh_vertices(0, posed, keep_previous=True)
    assert s.mesh_device_previous(0).tobytes() == first.tobytes()
    _same_read(s.mesh_device_read(0), ref.mesh_device_read(0), name)
    fa = _frame(s, name)
    w, h = 64, 48
    v = nrm._mesh(name)[0].astype(np.float64)
    centre, ext = refit._to_world(v.mean(0)[None])[0], nrm._extent(v)
    pos = centre + 1.6 * ext * np.array([0.3, 0.2, 0.93])
    cam = capi.Camera()
    cam.pos[:], cam.dir[:], cam.up[:] = tuple(pos), tuple((centre - pos) / np.linalg.norm(centre - pos)), (0.0, 1.0, 0.0)
    cam.fov, cam.focaldist, cam.dof, cam.width, cam.height = 40.0, 1.0, 0.0, w, h
    got = s.motion(cam, cam, None, fa["z"], fa["object_id"])
    want = ref.motion(cam, cam, None, fa["z"], fa["object_id"])
    assert got.tobytes() == want.tobytes()
    Y, X = np.mgrid[0:h, 0:w]
    assert (np.abs(got[..., 0] - X) + np.abs(got[..., 1] - Y)).max() > 0.5          # the mesh's pixels did move
    assert s.mesh_skin(0)["store_current"] == 0
    s.pose_mesh(0, host.pose(name, n, "identity"))
    assert s.mesh_device_previous(0) is None and s.previous_positions() == 0
    # the store, asked now, has what the devices had: a flagged pose later on hands the device's positions on
    s.pose_mesh(0, host.pose(name, n, "shear"), keep_previous=True)
    assert s.mesh_device_previous(0).tobytes() == host.mirror(name, rig_name, "identity").tobytes()


# ---- sequences -----------------------------------------------------------------------------------------------------------
def _same_boxes(a, b, what):
    """the same tree with the same bounds; the sign of a zero bound is the refit's to keep from the tree's history (csrc/rt_refit.hip:
    a bound that compares equal to the stored one is left alone), so bounds are compared as numbers, NaN (an unused child) as NaN"""
    assert a["nodes"]["c"].tobytes() == b["nodes"]["c"].tobytes() and a["slot_face"].tobytes() == b["slot_face"].tobytes(), what
    for k in ("lo", "hi"):
        assert np.array_equal(a["nodes"][k], b["nodes"][k], equal_nan=True), (what, k)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ("stored", "smooth"))
def test_rest_moved_rest_ends_at_the_untouched_scene(mode):
    """three poses in a row, rest -> moved -> rest, with one bone at weight 1 on the sheet (no -0.0 coordinate, no zero bound of
    mixed sign: the identity pose gives the rest bytes): device state and frame end byte-identical to the untouched scene's"""
    name, rig_name = "sheet3", "one"
    s, n = _skinned(name, rig_name, mode)
    untouched = nrm._scene(name)
    rest = host.pose(name, n, "identity")
    assert host.mirror(name, rig_name, "identity").tobytes() == nrm._mesh(name)[0].tobytes()
    s.pose_mesh(0, rest)
    s.pose_mesh(0, host.pose(name, n, "shear"))
    assert s.mesh_device_read(0)["tris"].tobytes() != untouched.mesh_device_read(0)["tris"].tobytes()
    s.pose_mesh(0, rest)
    if mode == "smooth":                                                # (the untouched scene holds the stored normals: give it the mode's)
        v, f, vn, fn = nrm._mesh(name)
        untouched = nrm._scene(name, v, capi.mesh_smooth_normals(v, f, fn, vn))
    _same_read(s.mesh_device_read(0), untouched.mesh_device_read(0), mode)
    _same_frame(_frame(s, name), _frame(untouched, name), mode)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ("stored", "smooth"))
def test_rest_bent_rest_ends_where_it_began(mode):
    """the same on the teapot under a blending rig, whose identity pose rounds (and whose OBJ has -0.0 coordinates): slots, normals,
    root box and frame after rest -> bent -> rest are byte for byte those after the first rest pose, and those of an untouched scene
    given the mirror's rest positions; the tree's bounds are the same numbers"""
    name, rig_name = "teapot", "chain3"
    s, n = _skinned(name, rig_name, mode)
    rest = host.pose(name, n, "identity")
    s.pose_mesh(0, rest)
    a, fa = s.mesh_device_read(0), _frame(s, name)
    s.pose_mesh(0, host.pose(name, n, "bend"))
    assert s.mesh_device_read(0)["tris"].tobytes() != a["tris"].tobytes()
    s.pose_mesh(0, rest)
    b = s.mesh_device_read(0)
    _same_read(b, a, mode, ("slot_face", "tris", "nrm", "root_box"))
    _same_boxes(b, a, mode)
    _same_frame(_frame(s, name), fa, mode)
    t, _ = _skinned(name, rig_name, mode)
    t.update_mesh_vertices(0, host.mirror(name, rig_name, "identity"))
    _same_read(t.mesh_device_read(0), a, mode)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ("stored", "smooth"))
def test_a_scene_lowered_after_the_pose_gives_the_same_frame(mode):
    """the store resolves the pose at the lowering: the frame is the one of a scene lowered before the pose"""
    name, rig_name = "teapot", "chain65"
    early, n = _skinned(name, rig_name, mode)
    late, _ = _skinned(name, rig_name, mode, lower=False)
    bones = host.pose(name, n, "bend")
    early.pose_mesh(0, bones)
    late.pose_mesh(0, bones)
    assert late.mesh_skin(0)["store_current"] == 0
    fl = _frame(late, name)
    assert late.mesh_skin(0)["store_current"] == 1
    _same_frame(_frame(early, name), fl, mode)
    a, b = nrm._by_face(early.mesh_device_read(0)), nrm._by_face(late.mesh_device_read(0))
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    # a plain update of the skinned mesh is what it was, and the next pose starts from the rest pose again
    dv = nrm._deformed(name)
    early.update_mesh_vertices(0, dv)
    plain = nrm._scene(name)
    plain.mesh_device_read(0)
    plain.set_mesh_normals(0, mode)
    plain.update_mesh_vertices(0, dv)
    _same_read(early.mesh_device_read(0), plain.mesh_device_read(0), "plain update")
    early.pose_mesh(0, bones)
    a = nrm._by_face(early.mesh_device_read(0))
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
