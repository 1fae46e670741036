"""Motion vectors for deforming meshes (rt_scene_motion, rt_scene_motion_device, k_motion_mesh; RT_MESH_UPDATE_KEEP_PREVIOUS;
Scene.motion, Scene.update_mesh_vertices(keep_previous=True), Scene.render_temporal(moving=True)).  The reference has no
counterpart: the yardstick is tests/motion_mesh_exact.py, a float64 transcription of the header's section with a brute-force ray
test, checked on the CPU through properties that do not depend on the transcription.  The z and object_id planes of the plane
tests are synthetic (the depth of a jittered sample's ray, from the same brute-force test); the tests that need real frames
render them."""
import ctypes as C

import numpy as np
import pytest

from raytracing_folder_amd import capi, workloads
from tests import deep_meshes, scenes
from tests import motion_mesh_exact as mx
from tests.test_motion import make_nodes, ref_motion, rot_z, set_node
from tests.stage_support import BIG, F
from tests.test_temporal import MAX_LEFT_OUT, make_cam

MESH = 1                                # the mesh's node in every scene here
SIZES = ((37, 23), (64, 48))
EXTENT = 16.0                           # a sheet of this extent at z = 0 overfills the frustum of the cameras below (fov 40 from z = 10)
SHIFT = np.array([0.375, -0.25, 0.125])    # exact in float32, like the sheets' vertices and the camera's position


TEAPOT_CAM = (0.125, 0.0625, 4.5)      # moved in until the teapot's left-out share is under the cap: 37 x 23 from z = 10 left out 4 of 76 pixels


def _cam(w, h, pos=(0.125, 0.0625, 10.0), yaw=0.0):
    """off the axis, so that no pixel centre's ray runs through a vertex or along a diagonal of the sheets"""
    return make_cam(w, h, pos=pos, yaw=yaw)


def _nodes(tm=np.eye(3), pos=(0.0, 0.0, 0.0), extra=0):
    nodes = make_nodes(2 + extra)
    set_node(nodes, MESH, tm, pos)
    nodes[MESH]["obj_type"], nodes[MESH]["mesh"], nodes[MESH]["material"] = capi.OBJ_MESH, 0, 0
    return nodes


def _chain_nodes(turn, pos):
    """root, a group turned and moved, and under it the mesh's node (node 2 here)"""
    nodes = make_nodes(3)
    set_node(nodes, 1, rot_z(turn), pos)
    set_node(nodes, 2, pos=(0.1, -0.2, 0.05), parent=1)
    nodes[2]["obj_type"], nodes[2]["mesh"], nodes[2]["material"] = capi.OBJ_MESH, 0, 0
    return nodes


def _teapot():
    m = scenes.load_cornell()[0].export()["meshes"][0]
    v = m["v"].astype(np.float64)
    c, e = 0.5 * (v.max(0) + v.min(0)), float((v.max(0) - v.min(0)).max())
    return ((v - c) * (5.0 / e)).astype(F), m["f"].astype(np.uint32)       # centred, 5 units across


_cases = {}


def case(name, w, h):
    """(cam, prev_cam, nodes, prev_nodes, v, v_prev, f, jitter) of one input of the plane tests"""
    if (name, w, h) in _cases:
        return _cases[name, w, h]
    cam = prev_cam = _cam(w, h)
    nodes, prev_nodes, jitter = _nodes(), None, (0.0, 0.0)
    if name.startswith("sheet"):
        n = int(name.split(":")[0][5:])
        v0, f = workloads.sheet(n, EXTENT)
        kind = name.split(":")[1]
        if kind == "rest":
            v = v_prev = v0
        elif kind == "shift":
            v_prev, v = v0, (v0 + SHIFT).astype(F)
        elif kind == "wave0.05":        # both shapes waved: slopes below 1, no fold, the boundary stays outside the frustum
            v_prev, v = workloads.deform_wave(v0, 0.3, 0.05 * EXTENT), workloads.deform_wave(v0, 0.9, 0.05 * EXTENT)
        elif kind == "wave0.3":         # a wave this high folds the sheet over: it is the PREVIOUS shape, the current one is flat
            v_prev, v = workloads.deform_wave(v0, 0.3, 0.3 * EXTENT), v0
        else:                           # the sheet under a moved parent node and a moved camera together
            assert kind == "parent"
            v_prev, v = workloads.deform_wave(v0, 0.3, 0.05 * EXTENT), workloads.deform_wave(v0, 0.9, 0.05 * EXTENT)
            nodes, prev_nodes = _chain_nodes(4.0, (0.3, 0.1, -0.2)), _chain_nodes(0.0, (0.0, 0.0, 0.0))
            prev_cam = _cam(w, h, pos=(0.43, -0.12, 10.3), yaw=1.5)
    elif name == "teapot":
        v0, f = _teapot()
        v_prev, v = workloads.deform_wave(v0, 0.3, 0.25), workloads.deform_wave(v0, 0.9, 0.25)
        nodes = _nodes(rot_z(20.0) @ np.array([[1.0, 0, 0], [0, 0.0, -1.0], [0, 1.0, 0.0]]), (0.2, -0.3, 0.0))
        jitter = (0.3, -0.2)            # z belongs to a jittered sample: at the silhouettes the gate decides
        cam = prev_cam = _cam(w, h, pos=TEAPOT_CAM)
    else:
        assert name == "tower"          # stack_need 39 > RT_BVH_STACK: seen from below, up its axis, the walk spills
        v0, f = deep_meshes.tower(60, 2)
        v_prev, v = (v0 + F([0.05, -0.03, 0.0])).astype(F), v0
        nodes = _nodes(np.diag([1.0, -1.0, -1.0]), (0.0, 0.0, 0.0))       # turned over: the camera looks up the axis
    mesh_node = 2 if name.endswith("parent") else MESH
    z, ids = mx.synthetic_planes(cam, nodes, mesh_node, v, f, jitter)
    _cases[name, w, h] = dict(cam=cam, prev_cam=prev_cam, nodes=nodes, prev_nodes=prev_nodes, v=v, v_prev=v_prev, f=f, z=z, ids=ids, node=mesh_node)
    return _cases[name, w, h]


GPU_CASES = [("sheet1:wave0.05", 37, 23), ("sheet2:wave0.05", 37, 23), ("sheet16:wave0.05", 37, 23), ("sheet16:wave0.05", 64, 48),
             ("sheet16:wave0.3", 37, 23), ("sheet16:wave0.3", 64, 48), ("teapot", 37, 23), ("tower", 37, 23), ("sheet16:parent", 37, 23),
             ("sheet16:shift", 37, 23)]
_refs = {}


def reference(name, w, h):
    if (name, w, h) not in _refs:
        c = case(name, w, h)
        _refs[name, w, h] = mx.ref_motion_mesh(c["cam"], c["prev_cam"], c["nodes"], c["prev_nodes"], {c["node"]: (c["v"], c["v_prev"], c["f"])}, c["z"], c["ids"])
    return _refs[name, w, h]


def scene_of(c, flagged=True):
    """the case's mesh as mesh 0 of a scene with the case's nodes: set with its previous shape, then updated to the current one"""
    s = capi.Scene()
    s.set_nodes(c["nodes"])
    deep_meshes.add_mesh(s, 0, c["v_prev"] if flagged else c["v"], c["f"])
    s.set_materials(np.zeros(1, capi.BLINN))
    if flagged:
        s.update_mesh_vertices(0, c["v"], keep_previous=True)
    return s


# ---- CPU: the ABI -------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("rt_scene_motion_device", "rt_scene_motion", "rt_scene_update_mesh_vertices_flags", "rt_scene_update_mesh_vertices_auto_flags",
               "rt_scene_previous_positions", "rt_scene_mesh_device_previous")


def test_new_symbols_and_struct_sizes():
    L = capi.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name) and name in capi.SYMBOLS, name
    assert L.rt_abi_version() == 4 and capi.MESH_UPDATE_KEEP_PREVIOUS == 2 and capi.MESH_UPDATE_REBUILD == 1
    # both structs of the update calls and the planes struct are what they were
    assert C.sizeof(capi.MotionPlanes) == 32 and C.sizeof(capi.MeshQuality) == 40 and C.sizeof(capi.MeshUpdateMs) == 20
    v, f = workloads.sheet(3, 2.0)
    assert v.shape == (16, 3) and f.shape == (18, 3) and v.dtype == np.float32 and f.dtype == np.uint32
    n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    assert (n[:, 2] > 0).all() and np.isclose(0.5 * n[:, 2].sum(), 4.0) and np.abs(v[:, :2]).max() == 1.0


def test_argument_checks_come_before_any_gpu_call():
    """every refusal is RT_ERR_ARG and names its reason, with or without a GPU; the store keeps previous positions without one"""
    L = capi.lib()
    c = case("sheet2:shift", 37, 23)
    s = scene_of(c, flagged=False)
    cam, ptr = c["cam"], np.zeros(37 * 23 * 3, F).ctypes.data
    full = lambda **kw: capi.MotionPlanes(**{**dict(z=ptr, object_id=ptr, motion=ptr), **kw})

    def both(scene, cm, pc, pn, count, tol, pl, model=capi.SHADE_FIN):
        a = (scene._h if scene else None, model, 0)
        b = (C.byref(cm) if cm else None, C.byref(pc) if pc else None, pn.ctypes.data if pn is not None else None, count, C.c_float(tol), C.byref(pl) if pl else None)
        return (L.rt_scene_motion(*a, *b), L.rt_scene_motion_device(*a, None, *b, 1)), L.rt_last_error()

    broken = c["nodes"].copy()
    broken[1]["parent"] = 1
    pl_bad = full()
    pl_bad.struct_size = 24
    cases = [(b"scene is NULL", (None, cam, cam, None, 2, 0.05, full())), (b"NULL", (s, None, cam, None, 2, 0.05, full())),
             (b"NULL", (s, cam, None, None, 2, 0.05, full())), (b"NULL", (s, cam, cam, None, 2, 0.05, None)),
             (b"struct_size", (s, cam, cam, None, 2, 0.05, pl_bad)), (b"required", (s, cam, cam, None, 2, 0.05, full(motion=None))),
             (b"the scene has 2 nodes", (s, cam, cam, None, 3, 0.05, full())), (b"the scene has 2 nodes", (s, cam, cam, None, 0, 0.05, full())),
             (b"parent", (s, cam, cam, broken, 2, 0.05, full())), (b"previous one", (s, cam, _cam(36, 23), None, 2, 0.05, full())),
             (b"depth_tol", (s, cam, cam, None, 2, 0.0, full())), (b"depth_tol", (s, cam, cam, None, 2, -1.0, full())),
             (b"depth_tol", (s, cam, cam, None, 2, float("nan"), full())), (b"depth_tol", (s, cam, cam, None, 2, float("inf"), full()))]
    for what, args in cases:
        sts, err = both(*args)
        assert sts == (-1, -1) and what in err, (what, sts, err)
    for model in (-1, 5):
        sts, err = both(s, cam, cam, None, 2, 0.05, full(), model=model)
        assert sts == (-1, -1) and b"shading model" in err, (model, sts, err)
    # the flags
    v = c["v"]
    upd = lambda flags: L.rt_scene_update_mesh_vertices_flags(s._h, 0, v.ctypes.data, len(v), None, 0, flags)
    # the call that came before the flag takes the bits it always took
    assert L.rt_scene_update_mesh_vertices(s._h, 0, v.ctypes.data, len(v), None, 0, 2) == -1 and b"unknown flag" in L.rt_last_error()
    auto = lambda flags: L.rt_scene_update_mesh_vertices_auto_flags(s._h, 0, v.ctypes.data, len(v), None, 0, C.c_double(2.0), flags, None)
    assert upd(4) == -1 and b"unknown flag" in L.rt_last_error() and auto(1) == -1 and auto(3) == -1 and s.previous_positions() == 0
    if capi.device_count() == 0:        # (with a device these calls would refit: the GPU tests make them)
        assert upd(2) == 0 and s.previous_positions() == 1 and upd(0) == 0 and s.previous_positions() == 0
        assert upd(3) == 0 and s.previous_positions() == 1 and auto(0) == 0 and s.previous_positions() == 0
        assert auto(2) == 0 and s.previous_positions() == 1
        deep_meshes.add_mesh(s, 0, c["v"], c["f"])
        assert s.previous_positions() == 0
        sts, _ = both(s, cam, cam, None, 2, 0.05, full())
        assert sts == (-3, -3)


# ---- CPU: the reference alone -------------------------------------------------------------------------------------
def test_reference_of_a_sheet_at_rest_is_the_pixel_itself():
    for w, h in SIZES:
        c = case("sheet16:rest", w, h)
        got, found, near = reference("sheet16:rest", w, h)
        Y, X = np.mgrid[0:h, 0:w]
        assert found.all() and not near.any()
        tol = mx.motion_mesh_px(c["cam"], c["cam"], c["nodes"], None, MESH, c["v"], c["v_prev"], c["f"], float(c["z"].min()))
        assert (np.abs(got[..., 0] - X) + np.abs(got[..., 1] - Y)).max() <= tol       # (float64 against exact: far inside the float32 bound)
        assert np.abs(got[..., 2] - c["z"]).max() <= 2e-5 * c["z"].max()              # (t itself: z is its float32)


def test_reference_of_a_shifted_sheet_is_ref_motion_of_a_translated_node():
    """all vertices shifted by d under a fixed node = the same sheet under a node translated by d: test_motion's reference, which
    knows nothing of triangles, gives the plane"""
    for w, h in SIZES:
        c = case("sheet16:shift", w, h)
        got, found, near = reference("sheet16:shift", w, h)
        moved, before = _nodes(pos=SHIFT), _nodes()
        want, wfound, _ = ref_motion(c["cam"], c["cam"], moved, before, c["z"], c["ids"])
        assert found.all() and wfound.all() and not near.any()
        assert np.abs(got[..., :2] - want[..., :2]).max() < 1e-4 and np.abs(got[..., 2] - want[..., 2]).max() < 1e-4      # (z is float32(t): 1e-6 of 10)
        assert np.abs(got[..., 0] - np.mgrid[0:h, 0:w][1]).min() > 0.5                # and it is a motion of about a pixel and more


def test_few_pixels_are_left_out_of_the_gpu_comparisons():
    """at most MAX_LEFT_OUT of the valid pixels of every input of the GPU tests; the sheets overfill the frustum and leave out none"""
    for name, w, h in GPU_CASES:
        c = case(name, w, h)
        _, found, near = reference(name, w, h)
        valid = c["ids"] >= 0
        share = near.sum() / max(1, valid.sum())
        print(f"{name} {w}x{h}: {valid.sum()} valid pixels, {found.sum()} with a previous position, left out {near.sum()} ({share:.4f})")
        assert share <= MAX_LEFT_OUT, (name, w, h, share)
        if name.startswith("sheet"):
            assert valid.all() and not near.any(), name
        else:
            assert 8 <= valid.sum() < valid.size and found.sum() >= 8, name
    c = case("teapot", 37, 23)
    _, found, _ = reference("teapot", 37, 23)
    assert ((c["ids"] >= 0) & ~found).sum() >= 3        # the gate (or a centre ray's miss) takes pixels of the jittered silhouette


# ---- GPU ------------------------------------------------------------------------------------------------------------
def _check_mesh_plane(got, name, w, h, scale=1.0):
    """got against the reference: fx + fy within scale * motion_mesh_px on the pixels kept, z_exp within 2e-5 |want| + 1e-6, (x, y, 0)
    exactly where there is no previous position; returns the worst error over bound"""
    c = case(name, w, h)
    want, found, near = reference(name, w, h)
    keep, mesh = ~near, c["ids"] == c["node"]
    assert got.shape == want.shape and got.dtype == np.float32
    none = keep & ~found
    assert got[none].tobytes() == want[none].astype(F).tobytes(), name
    on = keep & found & mesh
    assert on.sum() >= 8
    z_min = float(min(c["z"][on].min(), want[..., 2][on].min()))
    tol = scale * mx.motion_mesh_px(c["cam"], c["prev_cam"], c["nodes"], c["prev_nodes"], c["node"], c["v"], c["v_prev"], c["f"], z_min)
    err = (np.abs(got[..., 0] - want[..., 0]) + np.abs(got[..., 1] - want[..., 1]))[on]
    zerr, ztol = np.abs(got[..., 2] - want[..., 2])[on], (2e-5 * np.abs(want[..., 2]) + 1e-6)[on]
    worst = max(float(err.max() / tol), float((zerr / ztol).max()))
    print(f"motion mesh {name} {w}x{h}: {on.sum()} pixels, max |fx|+|fy| error {err.max():.3e} px (bound {tol:.3e}: {err.max() / tol:.4f}), "
          f"z_exp worst err/tolerance {(zerr / ztol).max():.4f}")
    assert (err <= tol).all() and (zerr <= ztol).all(), (name, worst)
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("name,w,h", GPU_CASES[:-1])
def test_motion_plane_against_the_reference(name, w, h):
    """sheet(1): the root is a leaf, no node record; sheet(2): one node of leaves; sheet(16) waved by 0.05 and 0.3 of its extent;
    the teapot (silhouettes: the gate and the marker); the tower (stack_need 39: the spill path); a moved parent and camera.
    Measured on the MI355X: DESIGN 3."""
    c = case(name, w, h)
    s = scene_of(c)
    if name == "tower":
        assert s.mesh_device_bvh(0)[2].stack_need > s.mesh_device_bvh(0)[2].bvh_stack
    got = s.motion(c["cam"], c["prev_cam"], c["prev_nodes"], c["z"], c["ids"])
    _check_mesh_plane(got, name, w, h)
    assert s.motion(c["cam"], c["prev_cam"], c["prev_nodes"], c["z"], c["ids"]).tobytes() == got.tobytes()


def _random_planes(w, h, n_nodes, seed):
    rng = np.random.default_rng(seed)
    z = rng.uniform(5.0, 15.0, (h, w)).astype(F)
    ids = rng.integers(-1, n_nodes + 1, (h, w)).astype(np.int32)          # (one id beyond the table as well)
    z[rng.random((h, w)) < 0.05] = BIG
    z.reshape(-1)[:3] = (np.nan, np.inf, -np.inf)
    return z, ids


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", SIZES)
def test_rigid_pixels_are_k_motions_to_the_byte(w, h):
    """a sphere, the wall plane and an unflagged mesh: with nodes and camera moved, at rest, and with prev_nodes NULL, the scene's
    plane is capi.motion's on the same planes"""
    v, f = workloads.sheet(4, 2.0)
    nodes = make_nodes(4)
    for i, (obj, mesh) in enumerate(((capi.OBJ_SPHERE, -1), (capi.OBJ_PLANE, -1), (capi.OBJ_MESH, 0)), 1):
        set_node(nodes, i, rot_z(10.0 * i), (i - 2.0, 0.5 * i, 0.2 * i))
        nodes[i]["obj_type"], nodes[i]["mesh"], nodes[i]["material"] = obj, mesh, 0
    prev = nodes.copy()
    for i in (1, 2, 3):
        set_node(prev, i, rot_z(10.0 * i - 3.0), (i - 2.2, 0.5 * i + 0.1, 0.2 * i))
    s = capi.Scene()
    s.set_nodes(nodes)
    deep_meshes.add_mesh(s, 0, v, f)
    s.set_materials(np.zeros(1, capi.BLINN))
    s.update_mesh_vertices(0, v)        # an update without the flag: still rigid
    z, ids = _random_planes(w, h, 4, 5)
    cam, cam2 = _cam(w, h), _cam(w, h, pos=(0.5, -0.2, 10.4), yaw=2.0)
    for pc, pn in ((cam2, prev), (cam, prev), (cam, nodes.copy()), (cam, None), (cam2, None)):
        assert s.motion(cam, pc, pn, z, ids).tobytes() == capi.motion(cam, pc, nodes, pn, z, ids).tobytes()


@pytest.mark.gpu
def test_shifted_vertices_move_like_a_translated_node():
    """the sheet with all vertices shifted by d, flagged, under a fixed node, against the same sheet under a node translated by d,
    both through Scene.motion: within twice the bound; the z and object_id planes of the two renders are byte-identical"""
    w, h = 37, 23
    c = case("sheet16:shift", w, h)
    a = scene_of(c)
    b = capi.Scene()
    b.set_nodes(_nodes(pos=SHIFT))
    deep_meshes.add_mesh(b, 0, c["v_prev"], c["f"])
    b.set_materials(np.zeros(1, capi.BLINN))
    p = capi.default_params(min_sample=1, max_sample=1, threshold=-1.0)
    planes = []
    for s in (a, b):
        s.set_render_flags(capi.RENDER_REPRODUCIBLE)
        planes.append(s.render_outputs(c["cam"], p, ("object_id",)))
    assert (planes[0]["object_id"] == MESH).all()
    print(f"shifted vertices against translated node: max |z difference| of the two renders {np.abs(planes[0]['z'] - planes[1]['z']).max():.3e}")
    assert planes[0]["object_id"].tobytes() == planes[1]["object_id"].tobytes() and planes[0]["z"].tobytes() == planes[1]["z"].tobytes()
    got_a = a.motion(c["cam"], c["cam"], None, c["z"], c["ids"])
    got_b = b.motion(c["cam"], c["cam"], _nodes(), c["z"], c["ids"])
    _check_mesh_plane(got_a, "sheet16:shift", w, h)
    tol = 2 * mx.motion_mesh_px(c["cam"], c["cam"], c["nodes"], None, MESH, c["v"], c["v_prev"], c["f"], float(c["z"].min()))
    err = np.abs(got_a[..., 0] - got_b[..., 0]) + np.abs(got_a[..., 1] - got_b[..., 1])
    print(f"vertices shifted against node translated: max |fx|+|fy| difference {err.max():.3e} px (bound {tol:.3e})")
    assert (got_a[..., 2] > 0).all() and (got_b[..., 2] > 0).all() and err.max() <= tol
    assert np.abs(got_a[..., 2] - got_b[..., 2]).max() <= 2 * (2e-5 * got_b[..., 2].max() + 1e-6)


@pytest.mark.gpu
def test_previous_positions_follow_the_updates():
    w, h = 37, 23
    c = case("sheet16:wave0.05", w, h)
    s = scene_of(c, flagged=False)
    deep_meshes.add_mesh(s, 0, c["v_prev"], c["f"])
    args = (c["cam"], c["cam"], None, c["z"], c["ids"])
    rigid = s.motion(*args)
    assert s.mesh_device_previous(0) is None and s.previous_positions() == 0
    assert rigid.tobytes() == capi.motion(c["cam"], c["cam"], c["nodes"], None, c["z"], c["ids"]).tobytes()
    s.update_mesh_vertices(0, c["v"], keep_previous=True)
    assert s.mesh_device_previous(0).tobytes() == c["v_prev"].tobytes() and s.previous_positions() == 1
    refit = s.motion(*args)
    _check_mesh_plane(refit, "sheet16:wave0.05", w, h)
    assert refit.tobytes() != rigid.tobytes()
    # a rebuild keeps them (per vertex, not per slot), and the plane is the refit's
    for kw in (dict(rebuild=True), dict(max_ratio=1.0)):
        t = scene_of(c, flagged=False)
        deep_meshes.add_mesh(t, 0, c["v_prev"], c["f"])
        t.motion(*args)                 # lowered, so that max_ratio has a tree to measure
        q = t.update_mesh_vertices(0, c["v"], keep_previous=True, **kw)
        assert q is None or q["rebuilt"], q
        assert t.motion(*args).tobytes() == refit.tobytes(), kw
        assert t.mesh_device_previous(0).tobytes() == c["v_prev"].tobytes()
        assert t.mesh_device_read(0)["nodes"].tobytes() == t.mesh_device_bvh(0)[0].tobytes()       # built again, not refitted
    # an update without the flag, or set_mesh: rigid again
    s.update_mesh_vertices(0, c["v"])
    assert s.mesh_device_previous(0) is None and s.previous_positions() == 0 and s.motion(*args).tobytes() == rigid.tobytes()
    s.update_mesh_vertices(0, c["v"], keep_previous=True)
    assert s.mesh_device_previous(0).tobytes() == c["v"].tobytes()
    deep_meshes.add_mesh(s, 0, c["v"], c["f"])
    assert s.mesh_device_previous(0) is None and s.motion(*args).tobytes() == rigid.tobytes()


def _lit_sheet_scene(v, f):
    """the sheet under a point light close above it, so that its colour varies across the image (a blur along x changes it)"""
    s = capi.Scene()
    s.set_nodes(_nodes())
    deep_meshes.add_mesh(s, 0, v, f)
    m = np.zeros(1, capi.BLINN)
    m["diffuse"], m["ior"] = (0.8, 0.5, 0.3), 1.0
    s.set_materials(m)
    l = np.zeros(1, capi.LIGHT)
    l["type"], l["intensity"], l["position"] = capi.LIGHT_POINT, (1.0, 1.0, 1.0), (3.0, 2.0, 2.5)
    s.set_lights(l)
    s.set_render_flags(capi.RENDER_REPRODUCIBLE)
    return s


@pytest.mark.gpu
def test_render_temporal_follows_a_sliding_sheet_only_with_the_flag():
    """64 x 48, 4 spp, reproducible: a sheet slides in its own plane by about three pixels a frame under a fixed camera, three
    frames of render_temporal(moving=True).  With the flag the motion plane is the float64 reference's on the rendered z and id
    planes, within motion_mesh_px -- a shift of three pixels -- and the history grows; without it the same sequence reports
    fx == x -- the ghosting input.  motion_blur= then changes the sliding sheet, and leaves a sheet at rest under flagged updates
    byte-identical (and what the run without it gives)."""
    w, h = 64, 48
    cam = _cam(w, h)
    v0, f = workloads.sheet(16, 2 * EXTENT)
    step = np.array([3.0 * 2 * 10.0 * np.tan(np.radians(20.0)) / h, 0.0, 0.0])        # three pixels at distance 10
    p = lambda seed: capi.default_params(min_sample=4, max_sample=4, threshold=-1.0, seed=seed)
    X = np.mgrid[0:h, 0:w][1]
    shape = lambda k: (v0 + k * step).astype(F)
    for flagged in (True, False):
        s = _lit_sheet_scene(v0, f)
        with capi.History(0, w, h) as hst, capi.MotionBlur(0, w, h) as mb:
            for k in range(3):
                if k:
                    s.update_mesh_vertices(0, shape(k), keep_previous=flagged)
                out = s.render_temporal(hst, cam, p(20 + k), denoise=False, moving=True, motion_blur=mb)
                assert (out["object_id"] == MESH).all()
                assert np.ptp(out["accumulated"][..., 0]) > 0.05          # the light varies across the image
                got = out["motion"]
                dx = got[..., 0] - X
                if k == 0 or not flagged:
                    assert (dx == 0).all() and (got[..., 2] == out["z"]).all()
                    assert out["motion_blurred"].tobytes() == out["accumulated"].tobytes()      # no velocity: nothing to blur
                    continue
                want, found, near = mx.ref_motion_mesh(cam, cam, _nodes(), None, {MESH: (shape(k), shape(k - 1), f)}, out["z"], out["object_id"])
                assert found.all() and not near.any()
                tol = mx.motion_mesh_px(cam, cam, _nodes(), None, MESH, shape(k), shape(k - 1), f, float(min(out["z"].min(), want[..., 2].min())))
                err = np.abs(got[..., 0] - want[..., 0]) + np.abs(got[..., 1] - want[..., 1])
                zerr, ztol = np.abs(got[..., 2] - want[..., 2]), 2e-5 * np.abs(want[..., 2]) + 1e-6
                print(f"sliding sheet, frame {k}: max |fx|+|fy| error {err.max():.3e} px (bound {tol:.3e}), shift {dx.min():.4f} .. {dx.max():.4f} px, "
                      f"z_exp worst err/tolerance {(zerr / ztol).max():.4f}")
                assert (err <= tol).all() and (zerr <= ztol).all()
                assert np.abs(want[..., 0] - X + 3.0).max() < 0.05        # the reference's shift is the three pixels the sheet was moved by
                # the pixels whose surface point has been inside the image (all four taps) in every frame so far: its position
                # k frames ago was x - 3 k.  (The history length is interpolated like the colour: whole to rounding.)
                inside = (X >= 3 * k + 1) & (X < w - 1)
                assert np.abs(out["history"][inside] - (k + 1)).max() < 1e-3
                changed = (out["motion_blurred"] != out["accumulated"]).any(-1)
                assert changed.mean() > 0.5, changed.mean()                # three pixels of velocity: the blur changes the frame
    # a sheet at rest under flagged updates: the mesh pixels run the steps (fx = x to rounding, not exactly), the blur's early out
    # returns the frame bit for bit, and the run without motion_blur= gives the same planes
    runs = []
    for with_mb in (True, False):
        s = _lit_sheet_scene(v0, f)
        with capi.History(0, w, h) as hst, capi.MotionBlur(0, w, h) as mb:
            for k in range(3):
                if k:
                    s.update_mesh_vertices(0, v0, keep_previous=True)
                out = s.render_temporal(hst, cam, p(20 + k), denoise=False, moving=True, motion_blur=mb if with_mb else None)
            assert s.previous_positions() == 1 and np.abs(out["motion"][..., 0] - X).max() < 1e-3
            if with_mb:
                assert out["motion_blurred"].tobytes() == out["accumulated"].tobytes()
            runs.append(out)
    assert "motion_blurred" not in runs[1] and runs[0]["motion_blurred"].tobytes() == runs[1]["accumulated"].tobytes()
    assert runs[0]["motion"].tobytes() == runs[1]["motion"].tobytes()


@pytest.mark.gpu
def test_identical_inputs_on_two_streams_give_identical_bytes():
    import torch
    w, h = 64, 48
    c = case("sheet16:wave0.3", w, h)
    s = scene_of(c)
    z, ids = torch.from_numpy(c["z"]).cuda(), torch.from_numpy(c["ids"]).cuda()
    outs = [torch.full((h, w, 3), -7.0, dtype=torch.float32, device="cuda") for _ in range(2)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for o, st in zip(outs, streams):
        s.motion_device(0, st.cuda_stream, c["cam"], c["prev_cam"], c["prev_nodes"], z_ptr=z.data_ptr(), object_id_ptr=ids.data_ptr(),
                        motion_ptr=o.data_ptr(), sync=False)
    torch.cuda.synchronize()
    a, b = outs[0].cpu().numpy(), outs[1].cpu().numpy()
    assert a.tobytes() == b.tobytes() and a.tobytes() == s.motion(c["cam"], c["prev_cam"], c["prev_nodes"], c["z"], c["ids"]).tobytes()
    _check_mesh_plane(a, "sheet16:wave0.3", w, h)
