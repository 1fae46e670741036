"""Material classes (RT_MAT_NO_SPEC_TREE / RT_MAT_NO_SPECULAR, decided once per material where the scene is lowered): FIN shading
leaves out the reflection / refraction set-up and the Blinn lobe for materials whose reflection, refraction or specular colour
is +0, because the left-out terms are exactly +0.  CPU: the class word of every material is what the rule says, bit patterns
compared.  GPU: a render with the classes and one with RT_RENDER_GENERAL_SHADING (all class words clear, the general path for
every hit) are the same bytes in the linear plane, z and the sample count, and the same work counters (see SCHEDULED for the two
that no two renders share) -- inside one library build, in reproducible mode so that accumulation order cannot blur the comparison."""
import numpy as np
import pytest

from raytracing_folder_amd import capi, photons
from tests import scenes

TREE, SPEC = capi.MAT_NO_SPEC_TREE, capi.MAT_NO_SPECULAR


# ---- CPU: the lowering ---------------------------------------------------------------------------------------------------
def _blinn(**kw):
    """one material with the loader's defaults (specular 0.7, glossiness 20, ior 1) and the given fields replaced"""
    m = np.zeros(1, capi.BLINN)
    m["diffuse"], m["specular"], m["glossiness"], m["ior"] = 0.5, 0.7, 20.0, 1.0
    for k, v in kw.items():
        m[k] = v
    return m


def _classes(mats, maps=None):
    s = capi.Scene()
    s.set_materials(mats)
    if maps is not None:
        s.set_material_maps(maps)
    got = s.material_classes()
    s.set_render_flags(capi.RENDER_GENERAL_SHADING)
    assert (s.material_classes() == 0).all() and len(s.material_classes()) == len(mats)      # the hook clears every word
    s.set_render_flags(0)
    assert (s.material_classes() == got).all()
    s.close()
    return got


def test_cornell_material_classes():
    s = capi.Scene()
    s.load_xml(scenes.CORNELL)
    mats, cls = s.export()["materials"], s.material_classes()
    assert len(mats) == 6 and len(cls) == 6

    def index(field, value):
        hit = [i for i in range(len(mats)) if np.allclose(mats[field][i], value)]
        assert len(hit) == 1, (field, value, hit)
        return hit[0]
    wall, red, blue = index("diffuse", [1, 1, 1]), index("diffuse", [1, 0.5, 0.5]), index("diffuse", [0.5, 0.5, 1])
    mtl1, mtl2, mtl3 = index("diffuse", [1, 0.3, 0.3]), index("reflection", [1, 1, 1]), index("refraction", [1, 1, 1])
    for i in (wall, red, blue):                      # specular value="0", no reflection, no refraction
        assert cls[i] == TREE | SPEC
    assert cls[mtl1] == TREE                         # specular 0.7: only the ray tree is known to be empty
    assert cls[mtl2] == 0 and cls[mtl3] == 0         # the mirror and the glass (and the default specular 0.7)
    s.set_render_flags(capi.RENDER_REPRODUCIBLE | capi.RENDER_GENERAL_SHADING)
    assert s.render_flags() == capi.RENDER_REPRODUCIBLE | capi.RENDER_GENERAL_SHADING
    assert (s.material_classes() == 0).all()
    s.close()


def test_hand_made_material_classes():
    neg0 = np.float32(-0.0)
    mats = np.concatenate([
        _blinn(specular=0.0),                                    # 0: ks = +0 -> both (no reflection / refraction either)
        _blinn(specular=[0.0, neg0, 0.0]),                       # 1: ks = -0.0 in one channel
        _blinn(specular=0.0, reflection=[0, 1e-4, 0]),           # 2: a reflection of 1e-4
        _blinn(specular=0.0, glossiness=-1.0),                   # 3
        _blinn(specular=0.0, ior=0.0),                           # 4
        _blinn(specular=0.0, glossiness=0.0),                    # 5: 0^0 = 1 is still in [0, 1]
        _blinn(specular=0.0, refraction=[neg0, 0, 0]),           # 6: -0.0 is not +0.0
        _blinn(specular=[0, 0, np.nan]),                         # 7
        _blinn(specular=0.0, glossiness=np.inf, ior=np.inf),     # 8: neither is finite
        _blinn(specular=0.0, glossiness=np.nan, ior=np.nan),     # 9
        _blinn(specular=0.0, ior=-1.5),                          # 10
        _blinn(specular=0.0, glossiness=2.0 ** 20),              # 11: the largest glossiness whose lobe stays finite for sure
        _blinn(specular=0.0, glossiness=2.0 ** 21),              # 12
        _blinn(),                                                # 13: the loader's defaults
    ])
    want = [TREE | SPEC, TREE, SPEC, TREE, SPEC, TREE | SPEC, SPEC, TREE, 0, 0, SPEC, TREE | SPEC, TREE, TREE]
    assert _classes(mats).tolist() == want
    # a specular texture keeps the lobe (whatever it samples to); a diffuse texture does not matter
    maps = np.concatenate([capi.identity_map() for _ in range(2 * len(mats))])
    assert _classes(mats, maps).tolist() == want                 # maps that are all RT_MAP_NONE
    tex = np.zeros(1, capi.TEXTURE)
    tex["type"], tex["color1"], tex["color2"] = capi.TEX_CHECKER, 0.0, 1.0
    maps["texture"][2 * 0 + 1] = 0                               # material 0: specular map
    maps["texture"][2 * 5 + 0] = 0                               # material 5: diffuse map
    maps["texture"][2 * 11 + 1] = capi.MAP_EMPTY                 # material 11: a specular map that failed to load is a map
    s = capi.Scene()
    s.set_materials(mats)
    s.set_textures(tex, np.zeros(0, np.uint8))
    s.set_material_maps(maps)
    got = s.material_classes().tolist()
    s.close()
    want2 = list(want)
    want2[0], want2[11] = TREE, TREE
    assert got == want2


def test_accessor_arguments():
    s = capi.Scene()
    assert len(s.material_classes()) == 0
    s.set_materials(np.concatenate([_blinn(), _blinn(specular=0.0)]))
    import ctypes as C
    n, out = C.c_int32(), np.full(2, 99, np.uint32)
    assert capi.lib().rt_scene_material_classes(None, None, 0, C.byref(n)) == -1
    assert capi.lib().rt_scene_material_classes(s._h, capi._p(out), 1, C.byref(n)) == -1 and n.value == 2      # too little room
    assert out.tolist() == [99, 99]
    assert capi.lib().rt_scene_material_classes(s._h, capi._p(out), 2, None) == 0 and out.tolist() == [TREE, TREE | SPEC]
    s.close()


# ---- GPU: with the classes and without, the same bytes ---------------------------------------------------------------------
def _render_both_ways(s, cam, p):
    """the frame with the material classes and with RT_RENDER_GENERAL_SHADING, both reproducible: planes and counters of each"""
    out = []
    for flags in (capi.RENDER_REPRODUCIBLE, capi.RENDER_REPRODUCIBLE | capi.RENDER_GENERAL_SHADING, capi.RENDER_REPRODUCIBLE):
        s.set_render_flags(flags)
        rgb, z, cnt, lin, st, progress = s.render_linear(cam, p)
        assert progress == cam.width * cam.height
        ctr = s.render_counters().as_dict()
        out.append((dict(rgb=rgb, linear=lin, z=z, count=cnt), ctr, st))
    return out


# Two of the work counters are not functions of the frame but of how its rays happened to share waves, with or without this change:
# instance_visits counts an object once per WAVE that has any lane reaching its bounds (rt_trace.h: the object loop is wave-uniform,
# and a wave's shadow-ray hint is the occluder of whatever batch it traced before), gather_leaf_reads once per leaf a gather
# workgroup stages for the queries it was handed.  Measured on an MI355X, the Cornell frame below rendered three times in ONE mode:
# instance_visits 90280 / 90169 / 90241, gather_leaf_reads 2034 / 2035 / 2035 (general mode: 90018 / 90280 / 90210, 2036 / 2037 /
# 2038), every other field identical in all six.  Equality is asked of every counter that IS a function of the frame -- the rays of
# every kind, the per-lane traversal counts, the photon queries and the photons they examined -- and these two must stay within
# 2 % (a dropped or added ray shows in its own counter exactly; the run-to-run spread is 0.3 %).
SCHEDULED = ("instance_visits", "gather_leaf_reads")


def _assert_same(a, b):
    for name in ("linear", "z", "count", "rgb"):
        x, y = a[0][name], b[0][name]
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), f"{name}: {(x.view(np.uint8) != y.view(np.uint8)).sum()} bytes differ"
    print({k: (a[1][k], b[1][k]) for k in a[1] if a[1][k] or b[1][k]})
    for k in a[1]:
        if k in SCHEDULED:
            assert abs(a[1][k] - b[1][k]) <= 0.02 * max(a[1][k], b[1][k]), (k, a[1][k], b[1][k])
        else:
            assert a[1][k] == b[1][k], (k, a[1][k], b[1][k])
    for k in ("rays_primary", "rays_shadow", "rays_reflect", "rays_refract", "bvh_nodes_visited", "tris_tested",
              "photon_queries", "photons_visited", "samples", "pixels"):
        assert getattr(a[2], k) == getattr(b[2], k), k


@pytest.mark.gpu
def test_cornell_frame_is_the_same_bytes_without_the_classes():
    s, cam = scenes.load_cornell(64, 48)
    s.set_photons(photons.synth_cornell_photon_map(4000, seed=1))
    assert sorted(s.material_classes().tolist()) == [0, 0, TREE, TREE | SPEC, TREE | SPEC, TREE | SPEC]
    p = capi.default_params(min_sample=4, max_sample=4, threshold=-1.0)
    classed, general, again = _render_both_ways(s, cam, p)
    ctr = classed[1]
    # a real frame: every kind of ray, photon queries from the secondary hits on the walls
    assert ctr["rays_primary"] == 64 * 48 * 4 and ctr["rays_shadow"] > ctr["rays_primary"] // 2
    assert ctr["rays_reflect"] > 0 and ctr["rays_refract"] > 0 and ctr["photon_queries"] > 0
    assert np.isfinite(classed[0]["linear"]).all() and (classed[0]["linear"] > 0).any(axis=2).mean() > 0.9
    _assert_same(classed, general)
    _assert_same(again, general)                     # and back: the flag lowers the scene again both ways
    s.close()


def _camera(pos, target, w=32, h=32, fov=40.0):
    pos, target = np.asarray(pos, np.float64), np.asarray(target, np.float64)
    d = (target - pos) / np.linalg.norm(target - pos)
    x = np.cross(d, [0.0, 0.0, 1.0])
    up = np.cross(x / np.linalg.norm(x), d)
    cam = capi.Camera()
    for i in range(3):
        cam.pos[i], cam.dir[i], cam.up[i] = pos[i], d[i], up[i]
    cam.fov, cam.focaldist, cam.dof, cam.width, cam.height = fov, 1.0, 0.0, w, h
    return cam


def _light(kind, intensity, position=(0, 0, 0), direction=(0, 0, -1)):
    l = np.zeros(1, capi.LIGHT)
    l["type"], l["intensity"], l["position"], l["direction"] = kind, intensity, position, direction
    return l


AMBIENT = _light(capi.LIGHT_AMBIENT, 0.15)
KEY = _light(capi.LIGHT_POINT, 45.0, position=(3, -4, 6))
# in the plane z = 0 of the wall: N.L is 0 there -- a point light beside it, and a direct light along it
GRAZING_POINT = _light(capi.LIGHT_POINT, 30.0, position=(9.5, 0.5, 0))
GRAZING_DIRECT = _light(capi.LIGHT_DIRECT, 0.8, direction=(-1, 0, 0))
SHINY = _blinn(diffuse=[0.3, 0.5, 0.8], specular=0.6, glossiness=30.0)                                  # class 0 next to the classed wall
GLASS = _blinn(diffuse=0.0, specular=0.7, glossiness=80.0, refraction=0.9, ior=1.5, absorption=[0.02, 0.1, 0.05])

# (wall material, sphere material, lights, shell): one plane at z = 0 (scale 8) and one sphere of radius 1 on it; shell = a
# sphere of radius 14 of the WALL's material around all of it, camera and lights included, which is only ever hit from inside
BOUNDARY_CASES = {
    "gloss0": (_blinn(diffuse=[0.7, 0.6, 0.5], specular=0.0, glossiness=0.0), SHINY, [AMBIENT, KEY], False),
    "grazing": (_blinn(diffuse=0.8, specular=0.0), SHINY, [AMBIENT, KEY, GRAZING_POINT, GRAZING_DIRECT], False),
    "black": (_blinn(diffuse=0.0, specular=0.0), SHINY, [AMBIENT, KEY], False),
    "glass": (_blinn(diffuse=[0.8, 0.7, 0.6], specular=0.0), GLASS, [AMBIENT, KEY], True),
    "negative_kd": (_blinn(diffuse=[-0.3, 0.5, 0.0], specular=0.0), SHINY, [AMBIENT, KEY, GRAZING_POINT, GRAZING_DIRECT], False),
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(BOUNDARY_CASES))
def test_class_boundaries_are_the_same_bytes_without_the_classes(case):
    wall, ball, lights, shell = BOUNDARY_CASES[case]
    s = capi.Scene()
    nodes = [scenes.identity_node(), scenes.identity_node(0, capi.OBJ_PLANE, 0, scale=8.0),
             scenes.identity_node(0, capi.OBJ_SPHERE, 1, scale=1.0, pos=(0, 0, 1))]
    if shell:
        nodes.append(scenes.identity_node(0, capi.OBJ_SPHERE, 0, scale=14.0))
    s.set_nodes(np.concatenate(nodes))
    s.set_materials(np.concatenate([wall, ball]))
    s.set_lights(np.concatenate(lights))
    cls = s.material_classes().tolist()
    assert cls[0] == TREE | SPEC and cls[1] == (0 if shell else TREE)        # both classes in the frame, mixed inside a wave
    cam = _camera((0.5, -7.0, 3.0), (0.0, 0.0, 0.7))
    p = capi.default_params(min_sample=4, max_sample=4, threshold=-1.0)
    classed, general, again = _render_both_ways(s, cam, p)
    ctr, lin = classed[1], classed[0]["linear"]
    assert ctr["rays_primary"] == 32 * 32 * 4 and ctr["rays_shadow"] > 0
    hit_wall, hit_ball = classed[0]["z"][-1, :], classed[0]["z"][16, 16]
    assert (hit_wall > 4).all() and (hit_wall < 6).all() and 6 < hit_ball < 7     # the bottom row sees the wall, the centre the sphere
    if case == "glass":
        assert ctr["rays_refract"] > 0 and ctr["rays_reflect"] > 0
        assert (classed[0]["z"] < 30).all() and (classed[0]["z"][0, :] > 12).all()     # the shell closes the frame: the top row hits it from inside
    else:
        assert (classed[0]["z"][0, :] > 1e29).all()                         # the top row looks past the wall
    if case == "black":
        assert (lin[-1, :] == 0).all()                                      # nothing but zeros on the wall
    if case == "negative_kd":
        assert (lin[-1, :, 0] < 0).all() and (lin[-1, :, 1] > 0).all()      # the additions are kept: a negative channel stays negative
    _assert_same(classed, general)
    _assert_same(again, general)
    s.close()
