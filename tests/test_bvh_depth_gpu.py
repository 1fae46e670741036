"""Every tracing kernel at the depth of traversal stack it is built for (csrc/rt_trace.h: bvh_push / bvh_pop; the LDS part, then
the per-thread spill part in HBM), against the CPU oracle at the suite's existing bars: closest hits bit-exact, linear colours
2e-5, frames through _frame_gate.

Two fixture meshes of the tower family (tests/deep_meshes.py):
  A  T = 60, m = 2: 120 triangles, stack_need 39 of the 40 the kernels provide; a ray up its axis holds 37 entries.
  B  T = 100, m = 4: 400 triangles; binned SAH alone would need 73 entries, the builder's rebuild brings it to 40, and a ray up
     its axis then holds 34 (FIN) or 36 (P13 family, whose culled back faces never shorten the ray).
Before a test touches the GPU it proves with tests/bvh_walk.py that its rays get that deep (limits from rt_device_bvh_info, not
literals) and prints the peaks it measured."""
import numpy as np
import pytest

from oracle import orc
from raytracing_folder_amd import capi
from tests import bvh_walk, deep_meshes, scenes
from tests.test_gpu_parity import _close, _frame_gate

pytestmark = pytest.mark.gpu

MESH = {"A": (60, 2), "B": (100, 4)}
TOWER_POS = (0.0, 0.0, 12.0)          # where the frames and the photon pass put the tower: the middle of the Cornell box


class Tower:
    """a tower mesh under an identity node: scene, tree, the oracle's scene, and its 777 rays with the oracle's hits"""

    def __init__(self, which, axis, facing_down=False):
        self.T, self.m = MESH[which]
        self.axis = axis
        self.v, self.f = deep_meshes.tower(self.T, self.m, axis)
        if facing_down:                                 # the other winding: the same boxes and the same tree, front faces towards the rays that come up the axis
            self.f = np.ascontiguousarray(self.f[:, [0, 2, 1]])
        self.s, self.box = deep_meshes.mesh_scene(self.v, self.f)
        self.nodes, self.slot_face, self.info = self.s.mesh_device_bvh(0)
        self.osc = scenes.oracle_scene(self.s.export())
        self.rays = deep_meshes.axis_rays(self.T, axis)
        self.ref = {}

    def peaks(self, rays, model=capi.SHADE_FIN, positions=((0, 0, 0), (0, 0, 0)), scales=None, **kw):
        return bvh_walk.walk(self.v, self.f, self.nodes, self.slot_face, self.info.root_ref, self.box,
                             bvh_walk.through_identity_nodes(rays, positions, scales), model, **kw)[0]

    def oracle(self, model):
        if model not in self.ref:
            self.ref[model] = orc.trace(self.osc, model, self.rays)
        return self.ref[model]


_towers = {}


def _tower(which, axis=2, facing_down=False):
    if (which, axis, facing_down) not in _towers:
        _towers[which, axis, facing_down] = Tower(which, axis, facing_down)
    return _towers[which, axis, facing_down]


def _qualify(tag, peak, info, above_stack=64, near_need=3, most_above_lds=True):
    """the depth conditions of a deep test: at least `above_stack` rays hold more entries than the per-level kernels' LDS stack
    (so their spill part runs), most hold more than k_wavefront's LDS part, and the deepest is within `near_need` of what the
    tree can need at all"""
    n_stack, n_lds = int((peak > info.bvh_stack).sum()), int((peak > info.bvh_lds).sum())
    print(f"[bvh depth] {tag}: {len(peak)} rays, peak max {peak.max()} of stack_need {info.stack_need} "
          f"({n_stack} above RT_BVH_STACK = {info.bvh_stack}, {n_lds} above RT_BVH_LDS = {info.bvh_lds}; spill {info.bvh_spill})")
    assert info.stack_need <= info.bvh_lds + info.bvh_spill
    assert n_stack >= above_stack, tag
    assert not most_above_lds or 2 * n_lds > len(peak), tag
    assert peak.max() >= info.stack_need - near_need, tag
    assert peak.max() <= info.stack_need


@pytest.mark.parametrize("which, axis", [("A", 2), ("A", 0), ("A", 1), ("B", 2), ("B", 0), ("B", 1)])
def test_trace_rays_at_full_stack_depth(which, axis):
    """rt_trace_rays (k_trace: 32 LDS entries + spill), FIN and P13 triangles, 777 rays (a partial last workgroup) up, down and
    around the axis of the tower plus oblique controls.  Mesh A: 432 rays above 32 entries, peak 37 of 39.  Mesh B, the rebuilt
    tree: peak 34 (FIN) / 36 (P13) of 40 -- the cap of 28 .. 0 SAH levels that first fits leaves balanced halves below it, and a
    ray holds at most one entry per level of those, so no ray gets closer than 4 entries to the bound."""
    t = _tower(which, axis)
    for model in (capi.SHADE_FIN, capi.SHADE_P13):
        peak = t.peaks(t.rays, model)
        _qualify(f"trace_rays mesh {which} axis {axis} model {model}", peak, t.info, near_need=3 if which == "A" else 6)
        hit, hits = t.oracle(model)
        assert hit.sum() > (600 if model == capi.SHADE_FIN else 150)        # the P13 triangle is culled from behind: the rays up the axis walk the whole tree and hit nothing
        scenes.assert_hits_equal(t.s.trace_rays(t.rays, model), hit, hits)


def test_trace_rays_with_more_rays_than_the_spill_buffer_has_thread_slots():
    """330 000 rays on mesh A in ONE call: more than RT_SPILL_BLOCKS * RT_BLOCK threads' worth, so the grid-stride loop of
    k_trace takes a second ray on threads whose spill slots the first one filled; the count leaves a partial last workgroup.
    The rays are the 777 of the test above drawn at random (the oracle's answer per ray is computed once and drawn alike)."""
    t = _tower("A")
    slots = t.info.spill_blocks * t.info.block
    n = 330000
    assert n > slots and n % t.info.block != 0
    pick = np.random.default_rng(9).integers(0, len(t.rays), n)
    for model in (capi.SHADE_FIN, capi.SHADE_P13):
        peak = t.peaks(t.rays, model)[pick]
        _qualify(f"trace_rays 330 000 rays model {model}", peak, t.info, above_stack=100000)
        assert (peak[slots:] > t.info.bvh_stack).sum() > 500          # deep rays in the second round of the stride loop, too
        hit, hits = t.oracle(model)
        scenes.assert_hits_equal(t.s.trace_rays(t.rays[pick], model), hit[pick], {k: hits[k][pick] for k in ("node", "front", "z", "p", "N")})


def test_two_meshes_in_one_scene_one_deep_one_within_lds():
    """mesh A beside a mesh of 20 triangles whose tree fits the LDS part of every kernel (stack_need <= RT_BVH_LDS): the deep
    traversal and the shallow one share a launch and a thread's stack; hits bit-exact.  (The small mesh is spread out: where two
    triangles lie at EXACTLY the same float32 distance the P13 hit point is the kept triangle's own, and which one is kept is the
    one thing that may depend on the tree.)"""
    t = _tower("A")
    v2, f2 = deep_meshes.tower(20, 1, axis=0)
    v2[:, 0] *= np.float32(2.0 ** 36)                 # heights 2^-4 .. 2^15: no two of its triangles at one float32 distance from any of these rays
    s = capi.Scene()
    s.set_nodes(np.concatenate([scenes.identity_node(), scenes.identity_node(0, capi.OBJ_MESH, 0, 0), scenes.identity_node(0, capi.OBJ_MESH, 0, 1)]))
    deep_meshes.add_mesh(s, 0, t.v, t.f)
    deep_meshes.add_mesh(s, 1, v2, f2)
    s.set_materials(np.zeros(1, capi.BLINN))
    small = s.mesh_device_bvh(1)[2]
    assert 0 < small.stack_need <= small.bvh_lds and s.mesh_device_bvh(0)[2].stack_need == t.info.stack_need
    rays = np.concatenate([t.rays, deep_meshes.axis_rays(56, 0, seed=5)])
    _qualify("two meshes, the deep one", t.peaks(rays), t.info, most_above_lds=False)
    osc = scenes.oracle_scene(s.export())
    for model in (capi.SHADE_FIN, capi.SHADE_P13):
        hit, hits = orc.trace(osc, model, rays)
        assert len(set(hits["node"][hit.astype(bool)])) == 2
        scenes.assert_hits_equal(s.trace_rays(rays, model), hit, hits)


def test_shade_rays_with_shadow_rays_up_the_whole_tower():
    """rt_shade_rays, FIN: mesh A above a ground plane, a point light over the top of the tower.  Primary rays land on the plane
    and on the lowest triangles; their shadow rays run up the axis, an any-hit traversal that holds 37 entries before it meets
    its occluder (a triangle above 2^10: nearer ones fall under the t > 1e-3 of the triangle test).  A dropped stack entry would
    lose the occluder and light the point: colours against the oracle's at the 2e-5 bar."""
    t = _tower("A")
    top = deep_meshes.tower_top(t.T)
    s = capi.Scene()
    s.set_nodes(np.concatenate([scenes.identity_node(), scenes.identity_node(0, capi.OBJ_MESH, 0, 0),
                                scenes.identity_node(0, capi.OBJ_PLANE, 1, scale=64.0, pos=(0, 0, -1))]))
    deep_meshes.add_mesh(s, 0, t.v, t.f)
    m = np.zeros(2, capi.BLINN)
    m["diffuse"] = [[0.8, 0.6, 0.3], [0.5, 0.7, 0.9]]
    m["specular"], m["glossiness"], m["ior"] = 0.3, 20.0, 1.0
    s.set_materials(m)
    lights = np.zeros(2, capi.LIGHT)
    lights["type"] = [capi.LIGHT_AMBIENT, capi.LIGHT_POINT]
    lights["intensity"] = [[0.25] * 3, [4.0e12] * 3]
    light_pos = np.array([0.05, -0.2, 1.5 * top])
    lights["position"][1] = light_pos
    s.set_lights(lights)
    rng = np.random.default_rng(21)
    n = 900
    tgt = np.concatenate([rng.uniform(-0.9, 0.9, (600, 2)), rng.uniform(-40, 40, (300, 2))])      # on the plane: under the tower, and far from it
    o = np.concatenate([tgt + rng.normal(scale=0.05, size=(n, 2)), np.full((n, 1), -0.5)], 1)
    o[::3, 2] = 6.0                                                                                  # every third ray comes down through the tower
    d = np.concatenate([tgt, np.full((n, 1), -1.0)], 1) - o
    rays = np.concatenate([o, d], 1).astype(np.float32)
    osc = scenes.oracle_scene(s.export())
    p = capi.default_params()
    ohit, orgb, oz = orc.shade_rays(osc, scenes.oracle_params(p), rays)
    hit0, hits0 = orc.trace(osc, capi.SHADE_FIN, rays)
    h = hit0.astype(bool)
    shadow = np.concatenate([hits0["p"][h], light_pos[None, :] - hits0["p"][h]], 1)
    _qualify("shade_rays shadow rays", t.peaks(shadow, z0=np.float32(1.0), any_hit=True), t.info, most_above_lds=False)
    hit, rgb, z = s.shade_rays(p, rays)
    assert (hit == ohit).all() and z.tobytes() == oz.tobytes() and ohit.all()
    lit = orgb.max(1) > 0.25 * 0.9 + 1e-3
    assert 100 < lit.sum() < n - 300                                   # both verdicts occur
    assert _close(rgb, orgb).all(), (~_close(rgb, orgb).all(axis=1)).sum()


GLASS = dict(diffuse=0.1, specular=0.2, reflection=0.2, refraction=0.75, glossiness=20.0, ior=1.0)


def _cornell_with_tower(which, textured=False, glass=False, squashed=False):
    """The Cornell box with a tower along y at its middle.  Returns (scene, camera, tower, export, node index of the tower).
    Plain: a node that only translates, seen from far out on the tower's axis through a very long lens -- the 48 x 36 frame is
    the base triangle and its surroundings, and the primary rays stay inside the tower's column almost to its top (mesh A only:
    no float32 camera is far enough out for mesh B, 2^60 high).
    squashed: the node also scales the tower's axis by 2^-(T - 40), so that it stands one unit high in the box (in the mesh's own
    coordinates every ray is then nearly axial), seen from the Cornell camera's distance.
    glass: the tower gets a material of its own that reflects and refracts with ior 1 -- the refracted ray of every hit goes on up
    the column, the reflected one back down it -- and its triangles are wound the other way, to face the camera (every triangle but
    FIN's is culled from behind).  textured: a checker map on the tower's material."""
    t = _tower(which, 1, facing_down=glass)
    s, cam = scenes.load_cornell(48, 36)
    e = s.export()
    material = int(e["nodes"]["material"][e["nodes"]["obj_type"] == capi.OBJ_MESH][0])
    if glass:
        m = np.zeros(1, capi.BLINN)
        for k, val in GLASS.items():
            m[k] = val
        material = len(e["materials"])
        s.set_materials(np.concatenate([e["materials"], m]))
    node = scenes.identity_node(0, capi.OBJ_MESH, material, 1, pos=TOWER_POS)
    scale = (1.0, 2.0 ** -(t.T - 40) if squashed else 1.0, 1.0)
    node["tm"][0, 4], node["itm"][0, 4] = scale[1], np.float32(1.0) / np.float32(scale[1])
    s.set_nodes(np.concatenate([e["nodes"], node]))
    # vertex normals: the triangles' own, tipped a little -- with the shading normal exactly along the ray the reference's
    # refraction frame is normalize(0) (NaN colours that nobody claims parity on); with ior 1 the refracted ray goes straight on
    # whatever the normal
    normal = np.array([0, -1 if glass else 1, 0.25]) / np.sqrt(1 + 0.25 ** 2)
    deep_meshes.add_mesh(s, 1, t.v, t.f, normal=normal)
    if textured:
        tex = np.zeros(1, capi.TEXTURE)
        tex["type"], tex["color1"], tex["color2"] = capi.TEX_CHECKER, [1.0, 0.9, 0.2], [0.1, 0.2, 0.9]
        s.set_textures(tex, np.zeros(0, np.uint8))
        maps = np.concatenate([capi.identity_map() for _ in range(2 * len(e["materials"]))])
        maps["texture"][2 * material] = 0
        s.set_material_maps(maps)
    dist = 60.0 if squashed else 2.0 ** 18
    pos = (TOWER_POS[0] - 0.3, -dist, TOWER_POS[2])                     # tower triangle (x_t, y_t) = (0, -0.3): z = x_t, x = y_t
    for i in range(3):
        cam.pos[i], cam.dir[i], cam.up[i] = pos[i], (0, 1, 0)[i], (0, 0, 1)[i]
    cam.fov = float(np.degrees(2 * np.arctan(1.1 / dist)))
    t.where = dict(positions=((0, 0, 0), TOWER_POS), scales=((1, 1, 1), scale))
    return s, cam, t, s.export(), len(e["nodes"])


def _primary_rays(cam):
    oc = scenes.oracle_camera(cam)
    return np.stack([orc.primary_ray(oc, x, y, 0) for y in range(cam.height) for x in range(cam.width)])


def _primary_peaks(t, cam, model=capi.SHADE_FIN):
    return t.peaks(_primary_rays(cam), model, **t.where)


def _refracted_peaks(t, cam, e, tower_node, model=capi.SHADE_FIN):
    """the first refracted rays of the frame: from where a primary ray meets the glass tower, on in the same direction (ior 1)"""
    rays = _primary_rays(cam)
    hit, hits = orc.trace(scenes.oracle_scene(e), model, rays)
    on = hit.astype(bool) & (hits["node"] == tower_node)
    return t.peaks(np.concatenate([hits["p"][on], rays[on, 3:]], 1), model, **t.where)


def _frame(s, cam, e, p):
    rgb, z, cnt, st, _ = s.render(cam, p)
    orgb, oz, ocnt = orc.render(scenes.oracle_scene(e), scenes.oracle_camera(cam), scenes.oracle_params(p))
    _frame_gate(rgb, orgb, z, oz, cnt, ocnt)
    assert len(np.unique(orgb.reshape(-1, 3), axis=0)) > 3             # a picture, not one colour
    return rgb, z, cnt, st


P8 = dict(min_sample=8, max_sample=8, threshold=-1.0)


def test_frames_on_the_default_tracer_plain_and_textured():
    """48 x 36, 8 spp, FIN on k_wavefront (8 LDS entries + spill), mesh A: untextured, and with a checker map on the tower's
    material for the textured instantiation's stack.  896 of the 1728 pixels' primary rays hold more than 32 entries, the deepest
    38 of 39."""
    for textured in (False, True):
        s, cam, t, e, _ = _cornell_with_tower("A", textured)
        _qualify(f"frame mesh A textured {textured}", _primary_peaks(t, cam), t.info, most_above_lds=False)
        rgb, z, cnt, st = _frame(s, cam, e, capi.default_params(**P8))
        assert st.rays_shadow > 0


def test_frame_of_the_rebuilt_tree_on_the_default_tracer():
    """mesh B, the tree the builder had to build again, through k_wavefront: squashed to one unit of height by its node, so that
    the Cornell camera's rays run its whole column"""
    s, cam, t, e, _ = _cornell_with_tower("B", squashed=True)
    _qualify("frame mesh B", _primary_peaks(t, cam), t.info, near_need=6, most_above_lds=False)
    rgb, z, cnt, st = _frame(s, cam, e, capi.default_params(**P8))
    assert st.rays_shadow > 0


def test_frames_with_deep_secondary_rays_on_the_per_level_kernels_and_through_the_overflow_queue(monkeypatch):
    """mesh A as glass (reflection + refraction, ior 1): every hit sends a refracted ray on up the column and a reflected one back
    down, eight levels deep.  With the P6 model k_primary and k_bounce (32 LDS entries + spill) trace them.  With FIN and the LDS
    ray stacks of k_wavefront held to 300 entries (RT_WF_LDS_RAYS) a round of 256 primary rays pushes 512 children: the stacks
    overflow, and the queue pass of k_wavefront and the per-level launches behind it trace deep rays too."""
    s, cam, t, e, tower_node = _cornell_with_tower("A", glass=True)
    assert t.info.stack_need == _tower("A", 1).info.stack_need and t.nodes.tobytes() == _tower("A", 1).nodes.tobytes()
    for model in (capi.SHADE_P6, capi.SHADE_FIN):
        _qualify(f"glass frame, primary rays, model {model}", _primary_peaks(t, cam, model), t.info, most_above_lds=False)
        _qualify(f"glass frame, first refracted rays, model {model}", _refracted_peaks(t, cam, e, tower_node, model), t.info, most_above_lds=False)
    dim = e["lights"].copy()                                           # that model's point light has no fall-off: the Cornell lamp would burn the frame white
    dim["intensity"][dim["type"] == capi.LIGHT_POINT] = 0.6
    s.set_lights(dim)
    st = _frame(s, cam, s.export(), capi.default_params(shade_model=capi.SHADE_P6, gamma=1.0, bounce=5, **P8))[3]
    assert st.rays_refract > st.rays_primary // 4 and st.rays_reflect > 0 and st.peak_rays > 0
    s.set_lights(e["lights"])
    monkeypatch.setenv("RT_WF_LDS_RAYS", "300")
    st = _frame(s, cam, e, capi.default_params(bounce=8, **P8))[3]
    assert st.rays_refract > st.rays_primary // 4 and st.rays_reflect > st.rays_primary // 4
    assert st.peak_rays > 0                                            # rays did go through the global queues


def test_reproducible_frame_in_two_chunks_on_two_streams_equals_the_one_chunk_frame(monkeypatch):
    """reproducible mode: the frame of mesh A rendered in two chunks on two streams -- two working sets, each with a spill buffer
    of its own -- is the one-chunk frame to the byte"""
    s, cam, t, e, _ = _cornell_with_tower("A")
    _qualify("reproducible frame", _primary_peaks(t, cam), t.info, most_above_lds=False)
    s.set_render_flags(capi.RENDER_REPRODUCIBLE)
    p = capi.default_params(**P8)
    one = s.render(cam, p)
    whole = one[:3]
    monkeypatch.setenv("RT_CHUNK_SAMPLES", str(48 * 36 * 8 // 2))
    monkeypatch.setenv("RT_STREAMS", "2")
    two = s.render(cam, p)
    halves = two[:3]
    # the second render did take more than one chunk, two in flight at once: every chunk has primary and resolve launches of its own
    assert one[3].streams == 1 and two[3].streams == 2
    assert two[3].launches_primary > one[3].launches_primary > 0 and two[3].launches_resolve > one[3].launches_resolve > 0
    for a, b, name in zip(whole, halves, ("rgb", "z", "count")):
        assert a.tobytes() == b.tobytes(), name
    orgb, oz, ocnt = orc.render(scenes.oracle_scene(e), scenes.oracle_camera(cam), scenes.oracle_params(p))
    _frame_gate(whole[0], orgb, whole[1], oz, whole[2], ocnt)


def test_photon_pass_up_the_deep_mesh():
    """k_photon_trace (32 LDS entries + spill): the Cornell box with mesh A squashed to one unit of height at its middle and the
    lamp moved onto the tower's axis, 0.4 below its base.  A point light's photons fan out, so only a tower that is wide for its
    height keeps them in its column: a quarter of the lamp's directions enter the base and run the whole column (5298 of 20 000
    hold more than 32 entries, the deepest 38 of 39).  Qualified on 20 000 directions drawn uniformly over the sphere, as the pass
    draws its own (about 7 000 emissions for 20 000 stored photons); then the pass against the oracle's, as
    test_photon_pass_matches_oracle holds them together."""
    s, cam, t, e, tower_node = _cornell_with_tower("A", squashed=True)
    lights = e["lights"].copy()
    lamp = np.array([TOWER_POS[0] - 0.3, -0.4, TOWER_POS[2]], np.float32)
    assert (lights["type"] == capi.LIGHT_POINT).sum() == 1
    lights["position"][lights["type"] == capi.LIGHT_POINT] = lamp
    s.set_lights(lights)
    e = s.export()
    osc = scenes.oracle_scene(e)
    d = np.random.default_rng(12).normal(size=(20000, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.concatenate([np.tile(lamp, (len(d), 1)), d], 1).astype(np.float32)
    hit, hits = orc.trace(osc, capi.SHADE_FIN, rays)
    first = hit.astype(bool) & (hits["node"] == tower_node)
    assert first.sum() > 500
    _qualify("photon pass, lamp directions that enter the tower", t.peaks(rays[first], **t.where), t.info, most_above_lds=False)
    got, att = s.photon_pass(20000, 8, seed=78)
    ref, oatt = orc.photon_pass(osc, 20000, 8, seed=78)
    assert int(att) == int(oatt) > 2000 and len(got) == len(ref)      # thousands of emissions, a quarter of them up the column
    a, b = got[1:], ref[1:]
    dpos = np.abs(a["position"] - b["position"]).max(axis=1)
    assert (dpos < 2e-3).mean() > 0.97 and (dpos < 0.1).mean() > 0.995
    assert (a["position"] == b["position"]).all(axis=1).mean() > 0.3
    assert abs(a["power"].sum() / b["power"].sum() - 1) < 0.02
    on_tower = (np.abs(b["position"][:, 0] - TOWER_POS[0]) < 1) & (b["position"][:, 1] >= 0) & (b["position"][:, 1] <= 1.001) & (np.abs(b["position"][:, 2] - TOWER_POS[2]) < 1)
    assert on_tower.sum() > 20                                         # photons were stored on the tower too (a first hit is not stored: these came back from the walls)
