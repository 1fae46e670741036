"""Smooth normals of a deforming mesh (include/rt_mi355x.h, "smooth normals": k_mesh_normals in csrc/rt_mesh_normals.hip, the host
mirror rt_mesh_smooth_normals, the per-mesh mode rt_scene_set_mesh_normals_mode).  Three yardsticks, none of them the code under
test: tests/normals_ref.py, an independent float32 transcription of the definition (the mirror must equal it byte for byte); the
scene loader's ComputeNormals on an OBJ without normals; and a FRESH scene given the deformed vertices and the mirror's normals
through set_mesh (the device must hold, hit for hit and pixel for pixel, what that scene holds).  No tolerance anywhere.

Meshes: tri3, strip5, the tower and the teapot (fn != f) as tests/test_mesh_refit.py builds them; workloads.sheet(3, 2.0); a
sphere whose poles have valence 70, more than one wave of lanes; and one hand-made mesh with an unreferenced normal, a triangle
without area and a normal whose incident face normals cancel exactly.  Each undeformed and under deform_wave at 0.3 of its extent."""
import numpy as np
import pytest

from raytracing_folder_amd import capi, workloads
from tests import deep_meshes, normals_ref, scenes
from tests import test_mesh_refit as refit

F = np.float32
L = capi.lib
CPU_MESHES = ("tri3", "strip5", "deep", "sheet3", "teapot", "sphere70", "odd")
GPU_MESHES = ("tri3", "strip5", "sheet3", "teapot", "sphere70")
CLEAN = ("tri3", "strip5", "deep", "sheet3", "teapot", "sphere70")      # no degenerate input: ComputeNormals is defined on them
N_RAYS = 1024

_cache = {}


# ---- inputs -------------------------------------------------------------------------------------------------------------
def _stored_normals(v):
    """a unit normal per vertex, all different, none of them a smooth normal of the mesh (test_mesh_refit.py's recipe)"""
    d = v.astype(np.float64) - v.mean(0) + np.array([0.3, 0.2, 1.0]) * (v.max(0) - v.min(0) + 1.0)
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)


def _odd():
    """faces 0 and 1 are one triangle wound both ways and share normal 0 only: its two face normals are exact negatives, S_0 is
    exactly 0 and normal 0 keeps its stored value.  Face 2 has no area (three points of a line whose cross product is exactly
    0 undeformed): normals 6 and 7 see nothing else and keep theirs; normal 5 is shared with face 3, which gives it a direction.
    Normal 10 is named by no corner.  Faces 3 and 4 are ordinary."""
    v = np.array([[0, 0, 0], [1, 0.25, 0], [0.25, 1, 0.5], [2, 2, 2], [3, 3, 3], [4, 4, 4], [2.5, 0.5, 1], [0.5, 2.5, 1.5], [3, 0, 0.5]], F)
    f = np.array([[0, 1, 2], [0, 2, 1], [3, 4, 5], [3, 6, 7], [6, 8, 7]], np.uint32)
    fn = np.array([[0, 1, 2], [0, 3, 4], [5, 6, 7], [5, 8, 9], [8, 8, 9]], np.uint32)
    vn = _stored_normals(np.concatenate([v, v[:2] + F(0.5)]))
    return v, f, vn, fn


def _mesh(name):
    """(v, f, vn, fn) of a test mesh, undeformed; vn are the STORED normals"""
    if name not in _cache:
        if name in ("tri3", "strip5", "deep", "teapot"):
            out = refit._mesh(name)
        elif name == "odd":
            out = _odd()
        else:
            v, f = workloads.sheet(3, 2.0) if name == "sheet3" else workloads.uv_sphere(70, 5, (0.0, 0.0, 0.0), 1.0)
            v, f = v.astype(F), f.astype(np.uint32)
            out = v, f, _stored_normals(v), f.copy()
        _cache[name] = tuple(np.ascontiguousarray(a) for a in out)
    return _cache[name]


def _extent(v):
    return float((v.max(0) - v.min(0)).max())


def _deformed(name, phase=0.3):
    v = _mesh(name)[0]
    return workloads.deform_wave(v, phase, 0.3 * _extent(v))


def _shapes(name):
    return (("rest", _mesh(name)[0]), ("waved", _deformed(name)))


def _mirror(name, v):
    """the host mirror's normals of mesh `name` at positions v, over the mesh's stored normals: computed once per (mesh, shape)"""
    key = ("mirror", name, v.tobytes())
    if key not in _cache:
        _, f, vn, fn = _mesh(name)
        _cache[key] = capi.mesh_smooth_normals(v, f, fn, vn)
    return _cache[key]


def _scene(name, v=None, vn=None):
    """test_mesh_refit.py's scene: the mesh (vertices v, normals vn: default its own) as mesh 0 under the two-node chain that
    rotates and translates, the other mesh as mesh 1 beside it"""
    v0, f, vn0, fn = _mesh(name)
    v, vn = v0 if v is None else v, vn0 if vn is None else vn
    s = capi.Scene()
    s.set_nodes(np.concatenate([scenes.identity_node(), refit._node(0, *refit.CHAIN[0]),
                                refit._node(1, *refit.CHAIN[1], obj=capi.OBJ_MESH, material=0, mesh=0),
                                scenes.identity_node(0, capi.OBJ_MESH, 0, 1, pos=(0.0, 0.0, -4.0 * _extent(v0)))]))
    s.set_mesh(0, v, f, vn, fn, *capi.bvh_build(v, f))
    ov, of = refit._other_mesh()
    deep_meshes.add_mesh(s, 1, ov, of)
    s.set_materials(np.zeros(1, capi.BLINN))
    return s


def _get_mesh(s, index=0):
    return s.export()["meshes"][index]


# ---- CPU ----------------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_and_declared():
    for name in ("rt_mesh_smooth_normals", "rt_scene_set_mesh_normals_mode", "rt_scene_get_mesh_normals_mode", "rt_scene_mesh_normals_ms"):
        assert hasattr(L(), name) and name in capi.SYMBOLS and name in capi.SIGNATURES, name
    assert (capi.MESH_NORMALS_STORED, capi.MESH_NORMALS_SMOOTH) == (0, 1)


def test_odd_mesh_is_what_it_stands_for():
    v, f, vn, fn = _mesh("odd")
    assert 10 not in fn and len(vn) == 11
    for _, vv in _shapes("odd"):
        n = np.array([normals_ref._face_normal(vv, t) for t in f], F)
        assert (n[0] == -n[1]).all() and n[0].any()                  # exact negatives: S_0 = N + (-N) = 0
    n = np.array([normals_ref._face_normal(v, t) for t in f], F)
    assert not n[2].any() and n[3].any()                              # no area at rest; the wave gives it some


def test_argument_errors_change_nothing():
    s = _scene("strip5")
    v, f, vn, fn = _mesh("strip5")
    before = _get_mesh(s)
    p = capi._p
    assert L().rt_scene_set_mesh_normals_mode(s._h, 0, 2) == -1                     # unknown mode
    assert L().rt_last_error() == b"rt_scene_set_mesh_normals_mode: unknown mode 2"
    assert L().rt_scene_set_mesh_normals_mode(s._h, 5, 1) == -1                     # mesh never set
    assert L().rt_scene_set_mesh_normals_mode(s._h, -1, 1) == -1
    assert L().rt_scene_set_mesh_normals_mode(None, 0, 1) == -1
    mode = capi.C.c_uint32(7)
    assert L().rt_scene_get_mesh_normals_mode(s._h, 5, capi.C.byref(mode)) == -1 and mode.value == 7
    assert L().rt_scene_get_mesh_normals_mode(s._h, 0, None) == -1
    with pytest.raises(ValueError):
        s.set_mesh_normals(0, "flat")
    assert s.mesh_normals(0) == "stored"
    out = vn.copy()
    bad = f.copy()
    bad[-1, 2] = len(v)
    assert L().rt_mesh_smooth_normals(p(v), len(v), p(bad), None, len(f), p(out), len(out)) == -1       # face index >= nv
    bad = fn.copy()
    bad[0, 0] = len(vn)
    assert L().rt_mesh_smooth_normals(p(v), len(v), p(f), p(bad), len(f), p(out), len(out)) == -1       # normal index >= nvn
    assert L().rt_mesh_smooth_normals(p(v), len(v), p(f), None, len(f), p(out), len(out) - 1) == -1     # fn = f does not fit nvn
    assert L().rt_mesh_smooth_normals(None, len(v), p(f), None, len(f), p(out), len(out)) == -1
    assert L().rt_mesh_smooth_normals(p(v), len(v), p(f), None, len(f), None, len(out)) == -1
    assert L().rt_mesh_smooth_normals(p(v), len(v), p(f), None, 0, p(out), len(out)) == -1
    assert out.tobytes() == vn.tobytes()
    ms = capi.C.c_float(-1.0)
    assert L().rt_scene_mesh_normals_ms(s._h, 0, capi.C.byref(ms)) == -2 and ms.value == -1.0       # RT_ERR_STATE: nothing ran
    assert L().rt_scene_mesh_normals_ms(s._h, 0, None) == -1
    after = _get_mesh(s)
    for k in ("v", "f", "vn", "fn", "nodes", "elements"):
        assert before[k].tobytes() == after[k].tobytes(), k


@pytest.mark.parametrize("name", CPU_MESHES)
def test_mirror_is_the_transcription(name):
    """byte for byte, on both shapes; the normals that are kept are the stored bytes; fn = None stands for f and vn = None for zeros"""
    v0, f, vn, fn = _mesh(name)
    for shape, v in _shapes(name):
        want = normals_ref.smooth_normals(v, f, fn, vn)
        got = _mirror(name, v)
        assert got.dtype == F and got.tobytes() == want.tobytes(), (name, shape)
        named = np.zeros(len(vn), bool)
        named[fn.ravel()] = True
        assert got[~named].tobytes() == vn[~named].tobytes(), (name, shape)
        changed = (got != vn).any(1)
        print(f"[normals] {name} {shape}: {len(vn)} normals, {int((~named).sum())} unnamed, {int((named & ~changed).sum())} named and kept")
        assert changed[named].any()
    if name == "odd":
        rest, waved = _mirror(name, v0), _mirror(name, _deformed(name))
        for kept in (0, 6, 7, 10):
            assert rest[kept].tobytes() == vn[kept].tobytes(), kept
        for kept in (0, 10):                                          # the wave gives face 2 an area, not normal 0 a direction
            assert waved[kept].tobytes() == vn[kept].tobytes(), kept
        assert (rest[5] != vn[5]).any() and (waved[6] != vn[6]).any()
    if (fn == f).all():
        assert capi.mesh_smooth_normals(v0, f).tobytes() == normals_ref.smooth_normals(v0, f).tobytes()


def test_clean_meshes_are_clean():
    """what "no degenerate input" means for the comparison with ComputeNormals below: every vertex is named by a face, no face
    normal is zero and no vertex's sum is, on both shapes -- so ComputeNormals divides by no zero"""
    for name in CLEAN:
        f = _mesh(name)[1]
        for shape, v in _shapes(name):
            assert len(np.unique(f)) == len(v), (name, shape)
            n = normals_ref.smooth_normals(v, f)
            assert np.isfinite(n).all() and n.any(1).all(), (name, shape)


@pytest.mark.parametrize("name", CLEAN)
def test_mirror_is_the_loaders_compute_normals(name, tmp_path):
    """an OBJ written without normals and loaded through the scene loader gets ComputeNormals' normals: the mirror's, byte for byte"""
    f = _mesh(name)[1]
    for shape, v in _shapes(name):
        workloads.write_obj(str(tmp_path / f"{shape}.obj"), v, f)
        xml = tmp_path / f"{shape}.xml"
        xml.write_text(f'<xml><scene><object type="obj" name="{shape}.obj" material="m"/>'
                       '<material type="blinn" name="m"/></scene><camera/></xml>')
        s = capi.Scene()
        s.load_xml(str(xml))
        m = _get_mesh(s)
        assert m["v"].tobytes() == v.tobytes() and m["f"].tobytes() == f.tobytes() and m["fn"].tobytes() == f.tobytes(), (name, shape)
        assert m["vn"].tobytes() == capi.mesh_smooth_normals(v, f).tobytes(), (name, shape)


@pytest.mark.parametrize("name", CPU_MESHES)
def test_smooth_update_of_a_scene_never_lowered(name):
    """the store: set the mode, update without normals, and get_mesh gives the mirror's normals of the new vertices; with normals
    it gives those; the mode survives updates and set_mesh resets it.  (Fails without the feature: there is no mode to set.)"""
    v, f, vn, fn = _mesh(name)
    dv = _deformed(name)
    s = _scene(name)
    assert s.mesh_normals(0) == "stored"
    s.set_mesh_normals(0, "smooth")
    assert s.mesh_normals(0) == "smooth" and s.mesh_normals(1) == "stored"
    assert _get_mesh(s)["vn"].tobytes() == vn.tobytes()               # setting the mode touches no normal
    s.update_mesh_vertices(0, dv)
    m = _get_mesh(s)
    assert m["v"].tobytes() == dv.tobytes() and m["vn"].tobytes() == _mirror(name, dv).tobytes()
    assert m["nodes"].tobytes() == capi.bvh_build(dv, f)[0].tobytes()
    vn2 = np.ascontiguousarray(vn[::-1])
    s.update_mesh_vertices(0, v, vn2)                                 # an explicit vn wins for that call
    assert _get_mesh(s)["vn"].tobytes() == vn2.tobytes() and s.mesh_normals(0) == "smooth"
    s.update_mesh_vertices(0, dv, rebuild=True)                       # ... and the next update without one recomputes, over vn2
    held = capi.mesh_smooth_normals(dv, f, fn, vn2)
    assert _get_mesh(s)["vn"].tobytes() == held.tobytes()
    # two updates between reads: the normals are those of the LAST vertices, over what the store held at the last read
    s.update_mesh_vertices(0, v, keep_previous=True)
    s.update_mesh_vertices(0, dv, keep_previous=True)
    assert _get_mesh(s)["vn"].tobytes() == capi.mesh_smooth_normals(dv, f, fn, held).tobytes()
    # back to stored: the normals stay those of the last SMOOTH update, whatever the vertices do afterwards
    s.update_mesh_vertices(0, v)
    s.set_mesh_normals(0, "stored")
    s.update_mesh_vertices(0, dv)
    assert _get_mesh(s)["vn"].tobytes() == capi.mesh_smooth_normals(v, f, fn, held).tobytes()
    s.set_mesh_normals(0, "smooth")
    s.set_mesh(0, v, f, vn, fn, *capi.bvh_build(v, f))
    assert s.mesh_normals(0) == "stored"
    s.update_mesh_vertices(0, dv)
    assert _get_mesh(s)["vn"].tobytes() == vn.tobytes()


def test_stored_mode_is_untouched():
    """a mesh whose mode was never set, and one set back to STORED: updates keep the stored normals"""
    v, f, vn, fn = _mesh("strip5")
    dv = _deformed("strip5")
    s = _scene("strip5")
    s.update_mesh_vertices(0, dv)
    assert _get_mesh(s)["vn"].tobytes() == vn.tobytes()
    s.set_mesh_normals(0, "smooth")
    s.set_mesh_normals(0, "stored")
    s.update_mesh_vertices(0, v)
    assert _get_mesh(s)["vn"].tobytes() == vn.tobytes()


# ---- GPU ----------------------------------------------------------------------------------------------------------------
FORMS = {
    "plain": dict(),
    "auto_rebuilds": dict(max_ratio=1.0),
    "auto_keeps": dict(max_ratio=1.0e9),
    "rebuild": dict(rebuild=True),
    "device": dict(rebuild="device"),
    "device_auto": dict(rebuild="device", max_ratio=1.0),
    "device_fallback": dict(rebuild="device"),
    "keep_previous": dict(keep_previous=True),
}


def _by_face(read):
    order = np.argsort(read["slot_face"])
    return read["tris"][order], read["nrm"][order]


@pytest.mark.gpu
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", GPU_MESHES)
def test_slots_hold_the_mirrors_normals(name, form, monkeypatch):
    """after a SMOOTH update of a lowered scene, in every form of the update: nrm is the mirror's normals gathered through fn per
    slot, tris what a STORED update with the same vertices leaves; the store agrees; the mesh beside it is untouched"""
    v, f, vn, fn = _mesh(name)
    dv = _deformed(name)
    want = _mirror(name, dv)
    if form == "device_fallback":
        monkeypatch.setenv("RT_LBVH_STACK_CAP", "0")
    s, stored = _scene(name), _scene(name)
    other = s.mesh_device_read(1)
    stored.mesh_device_read(0)
    s.set_mesh_normals(0, "smooth")
    with pytest.raises(capi.RtError) as e:
        s.mesh_normals_ms()
    assert e.value.status == -2
    out = s.update_mesh_vertices(0, dv, **FORMS[form])
    stored.update_mesh_vertices(0, dv, **FORMS[form])
    if form == "device_fallback":
        assert out["fell_back"] or len(f) <= 4, out
    got, ref = s.mesh_device_read(0), stored.mesh_device_read(0)
    assert got["slot_face"].tobytes() == ref["slot_face"].tobytes() and got["nodes"].tobytes() == ref["nodes"].tobytes()
    assert got["tris"].tobytes() == ref["tris"].tobytes() and got["root_box"].tobytes() == ref["root_box"].tobytes()
    gathered = want[fn[got["slot_face"]]].reshape(-1, 9)
    assert got["nrm"].tobytes() == gathered.tobytes(), (name, form)
    assert ref["nrm"].tobytes() == vn[fn[ref["slot_face"]]].reshape(-1, 9).tobytes()
    assert _get_mesh(s)["vn"].tobytes() == want.tobytes()
    again = s.mesh_device_read(1)
    for k in ("nodes", "slot_face", "tris", "nrm", "root_box"):
        assert again[k].tobytes() == other[k].tobytes(), k
    if form in ("plain", "auto_keeps", "keep_previous", "device"):
        assert s.mesh_normals_ms() >= 0.0
    with pytest.raises(capi.RtError) as e:
        stored.mesh_normals_ms()                                      # STORED mode launches nothing
    assert e.value.status == -2


def _rays(name, phase):
    """1024 seeded rays of test_mesh_refit.py's kind at the mesh deformed at `phase`, and which of them are qualified as that file
    qualifies its rays: no two triangles accepted at a bit-equal closest t, under either triangle test"""
    if ("rays", name, phase) not in _cache:
        dv, f = _deformed(name, phase).astype(np.float64), _mesh(name)[1]
        rng = np.random.default_rng(11)
        pick = rng.integers(0, len(f), N_RAYS)
        w = rng.uniform(0.08, 1.0, (N_RAYS, 3))
        w /= w.sum(1, keepdims=True)
        tgt = refit._to_world((dv[f][pick] * w[:, :, None]).sum(1))
        centre, ext = refit._to_world(dv.mean(0)[None])[0], _extent(dv)
        tgt[::8] += rng.normal(size=(len(tgt[::8]), 3)) * ext
        d = rng.normal(size=(N_RAYS, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        o = centre + 3.0 * ext * d
        rays = np.concatenate([o, (tgt - o) * rng.uniform(1.2, 2.0, (N_RAYS, 1))], 1).astype(F)
        p, dd = refit._to_mesh(rays, _scene(name).get_nodes())
        ok = np.ones(N_RAYS, bool)
        for model in (capi.SHADE_FIN, capi.SHADE_P13):
            ok &= refit._closest(_deformed(name, phase), f, p, dd, model)[0] <= 1
        _cache["rays", name, phase] = rays, ok
    return _cache["rays", name, phase]


@pytest.mark.gpu
@pytest.mark.parametrize("name", GPU_MESHES)
def test_hits_are_the_fresh_scenes(name):
    """three successive SMOOTH updates at different phases; after each, and with a device build in between, every qualified ray
    gives the hit record a fresh scene with the mirror's normals gives"""
    s = _scene(name)
    s.mesh_device_read(0)
    s.set_mesh_normals(0, "smooth")
    for phase, form in ((0.9, {}), (0.6, dict(rebuild="device")), (0.3, {})):
        dv = _deformed(name, phase)
        s.update_mesh_vertices(0, dv, **form)
        fresh = _scene(name, dv, _mirror(name, dv))
        rays, ok = _rays(name, phase)
        assert ok.sum() >= N_RAYS * 3 // 4
        for model in (capi.SHADE_FIN, capi.SHADE_P13):
            a, b = s.trace_rays(rays, model), fresh.trace_rays(rays, model)
            assert b["hit"][ok].sum() >= N_RAYS // 4
            for k in ("hit", "z", "p", "N", "node", "front"):
                assert a[k][ok].tobytes() == b[k][ok].tobytes(), (phase, model, k)
        ga, gb = _by_face(s.mesh_device_read(0)), _by_face(fresh.mesh_device_read(0))
        assert ga[0].tobytes() == gb[0].tobytes() and ga[1].tobytes() == gb[1].tobytes(), phase


FRAME_PLANES = ("normal", "albedo", "object_id")


@pytest.mark.gpu
def test_frames_are_the_fresh_scenes():
    """the Cornell box with the teapot waved, 64 x 48, reproducible: after each of three SMOOTH updates the frame and its normal,
    albedo and object_id planes are byte for byte those of a fresh scene given the mirror's normals"""
    p = capi.default_params(min_sample=8, max_sample=8, threshold=-1.0)
    s, cam = refit._cornell_with(None)
    m = _get_mesh(s)
    first = s.render_outputs(cam, p, FRAME_PLANES)
    s.set_mesh_normals(0, "smooth")
    for phase in (0.3, 0.6, 0.9):
        v = workloads.deform_wave(m["v"], phase, 0.3 * _extent(m["v"]))
        s.update_mesh_vertices(0, v)
        fresh, _ = refit._cornell_with(None)
        fresh.set_mesh(0, v, m["f"], capi.mesh_smooth_normals(v, m["f"], m["fn"], m["vn"]), m["fn"], *capi.bvh_build(v, m["f"]), m["vt"], m["ft"])
        got, want = s.render_outputs(cam, p, FRAME_PLANES), fresh.render_outputs(cam, p, FRAME_PLANES)
        for k in ("rgb", "z", "count") + FRAME_PLANES:
            assert got[k].tobytes() == want[k].tobytes(), (phase, k)
        stale, _ = refit._cornell_with(v)                             # the same shape under the normals it was loaded with
        assert got["normal"].tobytes() != stale.render_outputs(cam, p, FRAME_PLANES)["normal"].tobytes()
        assert got["rgb"].tobytes() != first["rgb"].tobytes()


def _sheet_scene(v, f, vn):
    s = capi.Scene()
    s.set_nodes(np.concatenate([scenes.identity_node(), scenes.identity_node(0, capi.OBJ_MESH, 0, 0)]))
    s.set_mesh(0, v, f, vn, f, *capi.bvh_build(v, f))
    mat = np.zeros(1, capi.BLINN)
    mat["diffuse"] = 0.7
    s.set_materials(mat)
    s.set_render_flags(capi.RENDER_REPRODUCIBLE)
    cam = capi.Camera()
    cam.pos[:], cam.dir[:], cam.up[:] = (0.0, 0.0, 5.0), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0)
    cam.fov, cam.focaldist, cam.dof, cam.width, cam.height = 40.0, 1.0, 0.0, 48, 48
    return s, cam


@pytest.mark.gpu
def test_the_feature_shows():
    """sheet(8, 2.0) seen from +z, every stored normal (0, 0, 1), waved by 0.1 of its extent (the wave moves x and y by less than
    a cell's width against its neighbours: the sheet does not fold, every face still looks at the camera).  STORED: the sheet is
    lit as if flat -- the normal plane is k_resolve's average of (0, 0, 1) over the pixel's h hit samples, computed the way
    tests/test_feature_planes.py computes it (c += N * (1 / h) in sample order, float32) and compared exactly: an interpolated
    (0, 0, z) normalises to (0, 0, 1) exactly; the node is the identity, so there is no rotation to apply.  SMOOTH: most mesh pixels differ from that, and the plane is byte for byte that of a fresh scene given
    the mirror's normals.  (Fails without the feature: there is no mode to set.)"""
    v0, f = workloads.sheet(8, 2.0)
    flat = np.tile(np.array([[0, 0, 1]], F), (len(v0), 1))
    v = workloads.deform_wave(v0, 0.3, 0.1 * _extent(v0))
    assert (np.array([normals_ref._face_normal(v, t) for t in f], F)[:, 2] > 0).all()
    p = capi.default_params(min_sample=8, max_sample=8, threshold=-1.0)
    planes = ("normal", "alpha", "object_id")
    out = {}
    for mode in ("stored", "smooth"):
        s, cam = _sheet_scene(v0, f, flat)
        s.render_outputs(cam, p, planes)
        s.set_mesh_normals(0, mode)
        s.update_mesh_vertices(0, v)
        out[mode] = s.render_outputs(cam, p, planes)
    on = out["stored"]["object_id"] == 1
    assert on.sum() >= 48 * 48 // 8 and (out["smooth"]["object_id"] == out["stored"]["object_id"]).all()
    n, alpha = out["stored"]["normal"], out["stored"]["alpha"]
    flat_z = np.zeros(p.max_sample + 1, F)                              # k_resolve's average of h ones: c += 1 * (1 / h), h times, in float32
    for h in range(1, p.max_sample + 1):
        for _ in range(h):
            flat_z[h] = F(flat_z[h] + F(1) * (F(1) / F(h)))
    hits = np.rint(alpha[on] * p.max_sample).astype(int)
    assert (hits >= 1).all() and (alpha[on] == hits.astype(F) / F(p.max_sample)).all()
    assert (n[on][:, 0] == 0).all() and (n[on][:, 1] == 0).all() and (n[on][:, 2] == flat_z[hits]).all()
    differ = (out["smooth"]["normal"][on] != n[on]).any(1)
    print(f"[normals] sheet: {int(on.sum())} mesh pixels, {int(differ.sum())} differ in SMOOTH mode")
    assert 2 * differ.sum() > on.sum()
    fresh, cam = _sheet_scene(v, f, capi.mesh_smooth_normals(v, f, None, flat))
    want = fresh.render_outputs(cam, p, planes)
    for k in ("rgb", "z", "count") + planes:
        assert out["smooth"][k].tobytes() == want[k].tobytes(), k


@pytest.mark.gpu
def test_explicit_normals_win_for_their_call_and_runs_repeat():
    """SMOOTH mode on the device: an update that brings vn leaves exactly those in the slots, the next one without recomputes;
    the same sequence run twice leaves the same bytes"""
    name = "sphere70"
    v, f, vn, fn = _mesh(name)
    vn2 = np.ascontiguousarray(vn[::-1])
    runs = []
    for _ in range(2):
        s = _scene(name)
        s.mesh_device_read(0)
        s.set_mesh_normals(0, "smooth")
        got = []
        s.update_mesh_vertices(0, _deformed(name, 0.6))
        got.append(s.mesh_device_read(0))
        s.update_mesh_vertices(0, _deformed(name, 0.9), vn2)
        got.append(s.mesh_device_read(0))
        s.update_mesh_vertices(0, _deformed(name, 0.3))
        got.append(s.mesh_device_read(0))
        runs.append(got)
    a = runs[0]
    assert a[0]["nrm"].tobytes() == _mirror(name, _deformed(name, 0.6))[fn[a[0]["slot_face"]]].reshape(-1, 9).tobytes()
    assert a[1]["nrm"].tobytes() == vn2[fn[a[1]["slot_face"]]].reshape(-1, 9).tobytes()
    assert a[2]["nrm"].tobytes() == capi.mesh_smooth_normals(_deformed(name, 0.3), f, fn, vn2)[fn[a[2]["slot_face"]]].reshape(-1, 9).tobytes()
    for x, y in zip(*runs):
        for k in ("nodes", "slot_face", "tris", "nrm", "root_box"):
            assert x[k].tobytes() == y[k].tobytes(), k


@pytest.mark.gpu
def test_a_device_that_lowers_later_holds_the_same_normals():
    """SMOOTH updates of a scene nobody has lowered, then the first lowering: the store ran the mirror, and the device holds what
    a device updated in place holds"""
    name = "teapot"
    v, f, vn, fn = _mesh(name)
    dv = _deformed(name)
    s = _scene(name)
    s.set_mesh_normals(0, "smooth")
    s.update_mesh_vertices(0, _deformed(name, 0.9))
    s.update_mesh_vertices(0, dv)
    late = s.mesh_device_read(0)
    t = _scene(name)
    t.mesh_device_read(0)
    t.set_mesh_normals(0, "smooth")
    t.update_mesh_vertices(0, dv)
    a, b = _by_face(late), _by_face(t.mesh_device_read(0))
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    assert late["nrm"].tobytes() == _mirror(name, dv)[fn[late["slot_face"]]].reshape(-1, 9).tobytes()
