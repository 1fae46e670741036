"""Morph targets on the device (include/rt_mi355x.h, "morph targets": k_mesh_pose in csrc/rt_mesh_pose.hip behind the four
rt_scene_morph_mesh* entry points).  The yardsticks are tests/test_mesh_skin.py's, neither of them the code under test: the host
mirrors' positions (which tests/test_mesh_morph_host.py and tests/test_mesh_skin_host.py hold against independent transcriptions
of the definitions) given to a FRESH scene through set_mesh -- with capi.mesh_smooth_normals of them where the mode is SMOOTH --
and the same positions driven through update_mesh_vertices with the same arguments.  Every comparison is byte equality.

Meshes and sets are tests/test_mesh_morph_host.py's, rigs and bone poses tests/test_mesh_skin_host.py's, scene, rays and frame
tests/test_mesh_skin.py's.  The pose of the fresh-scene test has 12 of 256 targets active: one full batch of k_mesh_pose's loads
and a tail of four."""
import numpy as np
import pytest

from raytracing_folder_amd import capi
from tests import test_mesh_morph_host as host
from tests import test_mesh_normals as nrm
from tests import test_mesh_refit as refit
from tests import test_mesh_skin as skin_gpu
from tests import test_mesh_skin_host as skin

F = np.float32
N_RAYS = skin_gpu.N_RAYS
RIGS = (None, "chain3", "chain65")
ACTIVE = (3, 17, 40, 41, 77, 100, 128, 150, 199, 200, 230, 255)
_cache = {}


def _pose_weights():
    """12 of 256 non-zero, both signs, between 0.4 and 1.2 in size"""
    w = np.zeros(256, F)
    for k, t in enumerate(ACTIVE):
        w[t] = (0.4 + 0.07 * k) * (-1.0 if k % 3 == 2 else 1.0)
    return w


def _posed(name, set_name, w, rig_name=None, pose_name="bend"):
    """the mirrors' positions of a morph pose: rt_mesh_morph, then rt_mesh_skin over the result if a rig is named"""
    key = (name, set_name, w.tobytes(), rig_name, pose_name)
    if key not in _cache:
        v = capi.mesh_morph(nrm._mesh(name)[0], host.morph_set(name, set_name), w)
        if rig_name:
            idx, sw, n = skin.rig(name, rig_name)
            v = capi.mesh_skin(v, idx, sw, skin.pose(name, n, pose_name))
        _cache[key] = v
    return _cache[key]


def _bones(name, rig_name, pose_name="bend"):
    return None if rig_name is None else skin.pose(name, skin.rig(name, rig_name)[2], pose_name)


def _scene(name, set_name, rig_name=None, mode="stored", lower=True):
    s = host._morph_scene(name, set_name, rig_name)
    s.set_mesh_normals(0, mode)
    if lower:
        s.mesh_device_read(0)
    return s


# ---- the conditions of the fresh-scene test, on the CPU --------------------------------------------------------------------
@pytest.mark.parametrize("rig_name", RIGS)
@pytest.mark.parametrize("name", ("sheet3", "teapot"))
def test_the_pose_qualifies_its_rays(name, rig_name):
    """the weights of test_a_morph_pose_is_the_fresh_scene are chosen so that the posed mesh alone meets that test's conditions:
    at least 3/4 of the 1024 rays qualified and at least 1/4 hitting, by the brute-force float32 triangle tests (no GPU)"""
    posed = _posed(name, "full", _pose_weights(), rig_name)
    assert (posed != nrm._mesh(name)[0]).any()
    rays, ok = skin_gpu._rays(name, ("morph", rig_name), posed)
    assert ok.sum() >= N_RAYS * 3 // 4
    p, d = refit._to_mesh(rays, nrm._scene(name).get_nodes())
    for model in (capi.SHADE_FIN, capi.SHADE_P13):
        face = refit._closest(posed, nrm._mesh(name)[1], p, d, model)[1]
        assert ((face >= 0) & ok).sum() >= N_RAYS // 4, model


# ---- a pose against the fresh scene ----------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", ("stored", "smooth"))
@pytest.mark.parametrize("rig_name", RIGS)
@pytest.mark.parametrize("name", ("sheet3", "teapot"))
def test_a_morph_pose_is_the_fresh_scene(name, rig_name, mode):
    """after pose_mesh(morph_weights=...): slots, normals and root box are the fresh scene's (per face: the trees differ, one
    refitted, one built), the hits of 1024 rays and a frame with its planes too; mesh_morph_ms raises before the first pose"""
    s = _scene(name, "full", rig_name, mode)
    with pytest.raises(capi.RtError) as e:
        s.mesh_morph_ms()
    assert e.value.status == -2
    w = _pose_weights()
    assert s.pose_mesh(0, _bones(name, rig_name), morph_weights=w) is None
    assert s.mesh_morph_ms() > 0.0 and s.mesh_morphs(0)["store_current"] == 0
    posed = _posed(name, "full", w, rig_name)
    fresh = skin_gpu._fresh(name, posed, mode)
    got, want = s.mesh_device_read(0), fresh.mesh_device_read(0)
    assert got["root_box"].tobytes() == want["root_box"].tobytes()
    ga, gb = nrm._by_face(got), nrm._by_face(want)
    assert ga[0].tobytes() == gb[0].tobytes() and ga[1].tobytes() == gb[1].tobytes()
    assert s.mesh_morphs(0)["store_current"] == 0                     # reading the device asked the store for nothing
    rays, ok = skin_gpu._rays(name, ("morph", rig_name), posed)
    assert ok.sum() >= N_RAYS * 3 // 4
    for model in (capi.SHADE_FIN, capi.SHADE_P13):
        a, b = s.trace_rays(rays, model), fresh.trace_rays(rays, model)
        assert b["hit"][ok].sum() >= N_RAYS // 4
        for k in ("hit", "z", "p", "N", "node", "front"):
            assert a[k][ok].tobytes() == b[k][ok].tobytes(), (model, k)
    fa, fb = skin_gpu._frame(s, name), skin_gpu._frame(fresh, name)
    assert (fb["object_id"] >= 0).sum() >= 64 * 48 // 16
    skin_gpu._same_frame(fa, fb, (name, rig_name, mode))
    m = nrm._get_mesh(s)                                              # ... and the store, once asked, agrees
    assert m["v"].tobytes() == posed.tobytes() and m["vn"].tobytes() == nrm._get_mesh(fresh)["vn"].tobytes()


# ---- the active list's edges -----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("weights_name", host.WEIGHTS)
def test_active_list_edges(weights_name):
    """sheet3 with 256 targets bound: none active (the device's vertices are the base's bytes), target 0 alone, target 255 alone,
    every other one, all 256 -- the device holds what update_mesh_vertices with the mirror's positions leaves, and its positions,
    handed on as previous ones by a flagged pose, are the mirror's bytes"""
    name = "sheet3"
    s, ref = _scene(name, "full"), _scene(name, "full")
    w = host.weights(256, weights_name)
    want = host.mirror(name, "full", weights_name)
    assert (want.tobytes() == nrm._mesh(name)[0].tobytes()) == (weights_name == "zero")
    s.pose_mesh(0, morph_weights=w)
    ref.update_mesh_vertices(0, want)
    skin_gpu._same_read(s.mesh_device_read(0), ref.mesh_device_read(0), weights_name)
    s.pose_mesh(0, morph_weights=host.weights(256, "zero"), keep_previous=True)
    assert s.mesh_device_previous(0).tobytes() == want.tobytes()      # the vertices k_mesh_pose wrote, where it wrote them
    assert s.mesh_morphs(0)["store_current"] == 0


# ---- every form of the pose against the same form of update_mesh_vertices ---------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("form", list(skin_gpu.FORMS))
@pytest.mark.parametrize("name,set_name,weights_name,rig_name,mode", [("tri3", "five", "all", "half2", "smooth"), ("strip5", "lift", "all", None, "stored"),
                                                                      ("sheet3", "full", "alternating", "chain3", "smooth"),
                                                                      ("teapot", "full", "all", None, "smooth"), ("teapot", "five", "last", "chain1024", "stored")])
def test_every_form_leaves_what_the_update_leaves(name, set_name, weights_name, rig_name, mode, form, monkeypatch):
    """device state byte for byte (the trees are the same trees: the same refit, the same build), the same dict keys and flags;
    tri3 is a single leaf: the store resolves the pose and the call goes the way of an update (strip5, five faces, has a root
    record: the kernel runs)"""
    if form == "device_fallback":
        monkeypatch.setenv("RT_LBVH_STACK_CAP", "0")
    FORMS, FLAGS = skin_gpu.FORMS, skin_gpu.FLAGS
    s, ref = _scene(name, set_name, rig_name, mode), _scene(name, set_name, rig_name, mode)
    w = host.weights(len(host.morph_set(name, set_name)), weights_name)
    posed = _posed(name, set_name, w, rig_name, "shear")
    out = s.pose_mesh(0, _bones(name, rig_name, "shear"), morph_weights=w, **FORMS[form])
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
    skin_gpu._same_read(s.mesh_device_read(0), ref.mesh_device_read(0), (name, form))
    a, b = s.mesh_device_previous(0), ref.mesh_device_previous(0)
    assert (a is None) == (b is None) == (form != "keep_previous") and (a is None or a.tobytes() == b.tobytes())
    assert nrm._get_mesh(s)["v"].tobytes() == posed.tobytes()


# ---- previous positions ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("rig_name", (None, "chain65"))
@pytest.mark.parametrize("name", ("sheet3", "teapot"))
def test_keep_previous_swaps_and_the_motion_plane_follows(name, rig_name):
    """two flagged poses: the device's previous positions are the first pose's mirror positions and the motion plane is the one
    update_mesh_vertices(keep_previous=True) with the two mirrors' positions gives; the store is asked for nothing on the way -- no
    vertices went up; a third pose without the flag releases them"""
    mode = "smooth"
    s, ref = _scene(name, "full", rig_name, mode), _scene(name, "full", rig_name, mode)
    poses = ((host.weights(256, "alternating") * F(0.05), "shear"), (_pose_weights(), "bend"))
    first, second = (_posed(name, "full", w, rig_name, pose_name) for w, pose_name in poses)
    for (w, pose_name), posed in zip(poses, (first, second)):
        s.pose_mesh(0, _bones(name, rig_name, pose_name), morph_weights=w, keep_previous=True)
        # (store_current == 0 shows that the store never computed the positions, so none of THIS pose's can have gone up; it would
        # not show an upload of older store bytes that the kernel then overwrites -- the byte comparisons below hold the result)
        assert s.mesh_morphs(0)["store_current"] == 0 and s.previous_positions() == 1
        ref.update_mesh_vertices(0, posed, keep_previous=True)
    assert s.mesh_device_previous(0).tobytes() == first.tobytes()
    skin_gpu._same_read(s.mesh_device_read(0), ref.mesh_device_read(0), name)
    fa = skin_gpu._frame(s, name)
    w_, h_ = 64, 48
    v = nrm._mesh(name)[0].astype(np.float64)
    centre, ext = refit._to_world(v.mean(0)[None])[0], nrm._extent(v)
    pos = centre + 1.6 * ext * np.array([0.3, 0.2, 0.93])
    cam = capi.Camera()
    cam.pos[:], cam.dir[:], cam.up[:] = tuple(pos), tuple((centre - pos) / np.linalg.norm(centre - pos)), (0.0, 1.0, 0.0)
    cam.fov, cam.focaldist, cam.dof, cam.width, cam.height = 40.0, 1.0, 0.0, w_, h_
    got = s.motion(cam, cam, None, fa["z"], fa["object_id"])
    want = ref.motion(cam, cam, None, fa["z"], fa["object_id"])
    assert got.tobytes() == want.tobytes()
    Y, X = np.mgrid[0:h_, 0:w_]
    assert (np.abs(got[..., 0] - X) + np.abs(got[..., 1] - Y)).max() > 0.5          # the mesh's pixels did move
    assert s.mesh_morphs(0)["store_current"] == 0
    s.pose_mesh(0, morph_weights=host.weights(256, "zero"))
    assert s.mesh_device_previous(0) is None and s.previous_positions() == 0
    # the store, asked now, has what the devices had: a flagged pose later on hands the device's positions on
    s.pose_mesh(0, morph_weights=_pose_weights(), keep_previous=True)
    assert s.mesh_device_previous(0).tobytes() == nrm._mesh(name)[0].tobytes()


@pytest.mark.gpu
def test_two_owed_poses_hand_the_first_on():
    """tests/test_mesh_morph_host.py's sequences on a scene no device holds -- two flagged poses, nothing read between them -- and
    then the first lowering: the device's previous positions are the first pose's, its positions the second's"""
    name = "strip5"
    for first, second, want in host.keep_previous_sequences(name):
        s = _scene(name, "five", "chain3", lower=False)
        s.pose_mesh(0, keep_previous=True, **first)
        s.pose_mesh(0, keep_previous=True, **second)
        assert s.mesh_device_previous(0).tobytes() == want[0].tobytes()
        assert nrm._get_mesh(s)["v"].tobytes() == want[1].tobytes()
        fresh = nrm._scene(name, want[1])
        a, b = nrm._by_face(s.mesh_device_read(0)), nrm._by_face(fresh.mesh_device_read(0))
        assert a[0].tobytes() == b[0].tobytes()


# ---- the kinds of pose alternating ------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_kinds_alternate():
    """sheet3 with rig chain3 and the 256-target set bound: a bone pose, then flagged a morph pose without bones, a bone pose and a
    morph pose with bones.  After each step the device's previous positions are the mirror's of the step before (none after the
    first, which is not flagged) and its state is a reference scene's, driven through update_mesh_vertices with the same flag and
    the mirror's positions.  The two timers stay apart: mesh_morph_ms raises RT_ERR_STATE until the first morph pose and keeps its
    value across the bone pose behind it; mesh_skin_ms keeps its value across either morph pose"""
    name, rig_name = "sheet3", "chain3"
    s, ref = _scene(name, "full", rig_name), _scene(name, "full", rig_name)
    w2, w4 = host.weights(256, "alternating"), _pose_weights()
    steps = ((dict(bones=_bones(name, rig_name, "bend")), skin.mirror(name, rig_name, "bend")),
             (dict(morph_weights=w2), _posed(name, "full", w2)),
             (dict(bones=_bones(name, rig_name, "shear")), skin.mirror(name, rig_name, "shear")),
             (dict(bones=_bones(name, rig_name, "bend"), morph_weights=w4), _posed(name, "full", w4, rig_name, "bend")))
    skin_ms = morph_ms = before = None
    for k, (args, posed) in enumerate(steps):
        if morph_ms is None:
            with pytest.raises(capi.RtError) as e:
                s.mesh_morph_ms()
            assert e.value.status == -2
        s.pose_mesh(0, args.get("bones"), morph_weights=args.get("morph_weights"), keep_previous=k > 0)
        ref.update_mesh_vertices(0, posed, keep_previous=k > 0)
        prev = s.mesh_device_previous(0)
        assert (prev is None) if k == 0 else (prev.tobytes() == before.tobytes()), k
        skin_gpu._same_read(s.mesh_device_read(0), ref.mesh_device_read(0), k)
        if "morph_weights" in args:
            assert s.mesh_skin_ms() == skin_ms, k
            morph_ms = s.mesh_morph_ms()
            assert morph_ms > 0.0
        else:
            assert morph_ms is None or s.mesh_morph_ms() == morph_ms, k
            skin_ms = s.mesh_skin_ms()
            assert skin_ms > 0.0
        before = posed
    assert s.mesh_morphs(0)["store_current"] == 0


# ---- sequences -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", ("stored", "smooth"))
@pytest.mark.parametrize("name", ("sheet3", "teapot"))
def test_weights_up_and_back_end_at_the_untouched_scene(name, mode):
    """weights up and then back to all-zero: zero weights give the base's bytes -- the teapot's -0.0 coordinates included -- so
    slots, normals, root box and frame are byte for byte the untouched scene's (given the mode's normals); the tree's bounds are
    the same numbers (the refit keeps a zero bound's sign)"""
    s = _scene(name, "full", None, mode)
    v, f, vn, fn = nrm._mesh(name)
    untouched = nrm._scene(name, v, capi.mesh_smooth_normals(v, f, fn, vn)) if mode == "smooth" else nrm._scene(name)
    a = untouched.mesh_device_read(0)
    s.pose_mesh(0, morph_weights=_pose_weights())
    assert s.mesh_device_read(0)["tris"].tobytes() != a["tris"].tobytes()
    s.pose_mesh(0, morph_weights=host.weights(256, "zero"))
    b = s.mesh_device_read(0)
    skin_gpu._same_read(b, a, (name, mode), ("slot_face", "tris", "nrm"))
    assert np.array_equal(b["root_box"], a["root_box"])
    skin_gpu._same_boxes(b, a, (name, mode))
    skin_gpu._same_frame(skin_gpu._frame(s, name), skin_gpu._frame(untouched, name), (name, mode))
    assert nrm._get_mesh(s)["v"].tobytes() == v.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ("stored", "smooth"))
def test_a_scene_lowered_after_the_pose_gives_the_same_frame(mode):
    """the store resolves the pose at the lowering -- morph, then skin: the frame is the one of a scene lowered before the pose"""
    name, rig_name = "teapot", "chain65"
    early, late = _scene(name, "full", rig_name, mode), _scene(name, "full", rig_name, mode, lower=False)
    w, bones = _pose_weights(), _bones(name, rig_name)
    early.pose_mesh(0, bones, morph_weights=w)
    late.pose_mesh(0, bones, morph_weights=w)
    assert late.mesh_morphs(0)["store_current"] == 0
    fl = skin_gpu._frame(late, name)
    assert late.mesh_morphs(0)["store_current"] == 1
    skin_gpu._same_frame(skin_gpu._frame(early, name), fl, mode)
    a, b = nrm._by_face(early.mesh_device_read(0)), nrm._by_face(late.mesh_device_read(0))
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    # a plain bone pose on the mesh with morphs bound is what it is without them, and the next morph starts from the base again
    early.pose_mesh(0, bones)
    plain, _ = skin_gpu._skinned(name, rig_name, mode)
    plain.pose_mesh(0, bones)
    skin_gpu._same_read(early.mesh_device_read(0), plain.mesh_device_read(0), "plain pose", ("slot_face", "tris", "nrm", "root_box"))
    early.pose_mesh(0, bones, morph_weights=w)
    a = nrm._by_face(early.mesh_device_read(0))
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
