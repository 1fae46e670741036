"""Texture lookups of the kernels, one ray per lookup, at the coordinates where a lookup goes wrong and a random ray never lands:
texture_sample / tile_clamp / textured_color (csrc/rt_trace.h), environment_color / material_colors (rt_shade.h), the background
lookup of k_resolve, and the coordinates the sphere, the plane and the PROJ13 triangle hand to them.

The probe: one object under an identity node, material diffuse = 1 with a diffuse map and specular = 0, one ambient light of
intensity 1, bounce = 0 -- the rgb Scene.shade_rays returns is then the texture's colour and nothing else.  A ray from (x, y, 1)
along -z hits the unit plane at exactly (x, y, 0); tests/texture_ref.py chooses x, y and a power-of-two map so that the lookup
coordinate is a chosen float (test_texture_ref_host.py checks that every named edge is reached, and holds the oracle against
texture_ref on the same set, on the CPU).

Acceptance, for EVERY lookup (no share is left out): hit and z are the oracle's to the byte; rgb is within 2e-6 absolute of the
oracle's (on the plane's exact lookups: the oracle's bytes, as measured) and of texture_ref's (seven float32 roundings on values in [0, 1] are about 5e-7; neighbouring texels differ by at
least 0.125).  The sphere's tolerance adds max(width, height) * 2^-24: one float32 ulp of a coordinate in [0.5, 1], which the
device's and glibc's double atan2 / asin may differ by after rounding, times the steepest slope of a bilinear lookup."""
import numpy as np
import pytest

from oracle import orc
from raytracing_folder_amd import capi
from tests import graph_scenes as G, scenes, texture_ref as R
from tests.stage_support import encode_rgb8

pytestmark = pytest.mark.gpu
F = np.float32
TOL = 2e-6
NAMES = ("1x1", "2x2", "1x4", "4x1", "3x5", "4x4", "golden52x37", "checker")


def _close(a, b, rel=5e-5, abs_=2e-6):
    return np.abs(a - b) <= rel * np.maximum(np.abs(a), np.abs(b)) + abs_


def _material(**kw):
    m = np.zeros(1, capi.BLINN)
    m["diffuse"], m["glossiness"], m["ior"] = 1.0, 4.0, 1.0
    for k, v in kw.items():
        m[k] = v
    return m


def _light(kind, intensity=1.0, direction=(0, 0, -1)):
    l = np.zeros(1, capi.LIGHT)
    l["type"], l["intensity"], l["direction"] = kind, intensity, direction
    return l


class Probe:
    """the probe scene and its oracle twin over the same arrays; set_map() replaces one map record in both"""

    def __init__(self, nodes, material=None, lights=None, meshes=()):
        self.textures, self.texels, rec = R.edge_store(capi.TEXTURE)
        s = capi.Scene()
        s.set_nodes(nodes)
        for i, m in enumerate(meshes):
            s.set_mesh(i, m["v"], m["f"], m["vn"], m["fn"], m["nodes"], m["elements"], m["vt"], m["ft"])
        s.set_materials(_material() if material is None else material)
        s.set_lights(_light(capi.LIGHT_AMBIENT) if lights is None else lights)
        s.set_textures(rec, self.texels)
        self.maps = np.concatenate([capi.identity_map(), capi.identity_map()])
        s.set_material_maps(self.maps)
        self.s, self.osc = s, scenes.oracle_scene(s.export())

    def set_map(self, record, texture, which=0):
        self.maps[which] = record[0]
        self.maps["texture"][which] = texture
        self.s.set_material_maps(self.maps)
        self.osc.material_maps[:] = self.maps

    def shade(self, rays, p):
        hit, rgb, z = self.s.shade_rays(p, rays)
        ohit, orgb, oz = orc.shade_rays(self.osc, scenes.oracle_params(p), rays)
        assert (hit == ohit).all() and z.tobytes() == oz.tobytes()
        return hit.astype(bool), rgb, orgb

    def close(self):
        self.s.close()


def _plane_nodes():
    return np.concatenate([scenes.identity_node(), scenes.identity_node(0, capi.OBJ_PLANE, 0)])


def _plane_rays(uvw):
    rays = np.zeros((len(uvw), 6), F)
    rays[:, 0], rays[:, 1], rays[:, 2], rays[:, 5] = R.plane_point(uvw[:, 0]), R.plane_point(uvw[:, 1]), 1, -1
    return rays


# ---- the plane: every texture at every edge coordinate ------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(NAMES)), ids=NAMES)
def test_diffuse_map_on_the_plane(index):
    pr = Probe(_plane_nodes())
    tex = pr.textures[index]
    assert tex.name == NAMES[index]
    p = capi.default_params(bounce=0)
    n = worst_o = worst_r = same = 0
    for m, uvw, t in R.edge_lookups(tex, capi.TEXMAP):
        pr.set_map(m, index)
        hit, rgb, orgb = pr.shade(_plane_rays(uvw), p)
        want = R.sample(tex, pr.texels, t)
        assert hit.all()
        worst_o, worst_r = max(worst_o, float(np.abs(rgb - orgb).max())), max(worst_r, float(np.abs(rgb - want).max()))
        same += int((rgb.view(np.uint32) == orgb.view(np.uint32)).all(axis=1).sum()); n += len(t)
        # measured on an MI355X: all 21 776 lookups of this test are the oracle's bytes, so that is what is asked (2e-6 was the bound set)
        assert rgb.tobytes() == orgb.tobytes() and np.abs(rgb - want).max() <= TOL, (tex.name, worst_o, worst_r)
    print(f"{tex.name}: {n} lookups, {same} of them the oracle's bytes; largest difference from the oracle {worst_o:.3g}, from texture_ref {worst_r:.3g}")
    assert n >= 784
    pr.close()


@pytest.mark.parametrize("index", range(len(NAMES)), ids=NAMES)
def test_specular_map_on_the_plane(index):
    """the same lookups through material_colors' second map: specular = 1 under a direct light whose Blinn term is not zero
    (the half vector of a ray along -z and this light is 9 degrees off the normal); the oracle alone is the reference"""
    d = np.array([0.3, 0.2, -1.0]) / np.linalg.norm([0.3, 0.2, -1.0])
    pr = Probe(_plane_nodes(), _material(diffuse=0.25, specular=1.0), _light(capi.LIGHT_DIRECT, 1.0, d))
    tex = pr.textures[index]
    p = capi.default_params(bounce=0)
    lo, hi = np.inf, -np.inf
    for m, uvw, t in R.edge_lookups(tex, capi.TEXMAP):
        pr.set_map(m, index, which=1)
        hit, rgb, orgb = pr.shade(_plane_rays(uvw), p)
        assert hit.all() and _close(rgb, orgb).all(), (tex.name, float(np.abs(rgb - orgb).max()))
        lo, hi = min(lo, float(rgb.min())), max(hi, float(rgb.max()))
    assert tex.width * tex.height == 1 or hi - lo > 0.05         # the diffuse term is one value: the specular term follows the texture
    pr.close()


def test_rotated_map_on_the_plane():
    """a map turned by 30 degrees with a scale of 3.7: the lookup coordinates are whatever the float32 product gives (the same
    operations in the kernel, the oracle and texture_ref.map_transform), so file textures only -- bilinear is continuous"""
    c, s = np.cos(np.pi / 6) * 3.7, np.sin(np.pi / 6) * 3.7
    m = capi.identity_map(0)
    m["itm"][0] = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]]).T.reshape(9)
    m["tm"][0] = np.linalg.inv(m["itm"][0].reshape(3, 3).astype(np.float64)).reshape(9)
    m["pos"][0] = (0.3, -0.2, 0.0)
    rng = np.random.default_rng(9)
    xy = np.concatenate([rng.uniform(-1, 1, (1500, 2)), [[-1, -1], [1, 1], [-1, 1], [1, -1], [0, 0]]]).astype(F)
    rays = np.zeros((len(xy), 6), F); rays[:, :2], rays[:, 2], rays[:, 5] = xy, 1, -1
    uvw = np.zeros((len(xy), 3), F); uvw[:, :2] = ((xy + F(1)).astype(F) / F(2)).astype(F)
    pr = Probe(_plane_nodes())
    p = capi.default_params(bounce=0)
    for index, tex in enumerate(pr.textures):
        if tex.kind != R.FILE:
            continue
        pr.set_map(m, index)
        hit, rgb, orgb = pr.shade(rays, p)
        want = R.sample(tex, pr.texels, R.map_transform(m["itm"][0], m["pos"][0], uvw))
        assert hit.all() and np.abs(rgb - orgb).max() <= TOL and np.abs(rgb - want).max() <= TOL, tex.name
    pr.close()


def test_lookup_that_is_not_finite_is_black():
    """a singular map (an itm entry of 1 / 0) hands texture_sample a NaN or an infinite coordinate: black, like RT_MAP_EMPTY, for
    file textures and the checker alike, and the oracle's bytes -- where a conversion of NaN to int would read some texel"""
    rng = np.random.default_rng(13)
    xy = np.concatenate([rng.uniform(-1, 1, (60, 2)), [[-1, -1], [1, 1], [0, 0], [1, -1]]]).astype(F)
    rays = np.zeros((len(xy), 6), F); rays[:, :2], rays[:, 2], rays[:, 5] = xy, 1, -1
    pr = Probe(_plane_nodes())
    p = capi.default_params(bounce=0)
    nan_map, inf_map = capi.identity_map(0), capi.identity_map(0)
    nan_map["itm"][0, 0], nan_map["itm"][0, 3] = np.inf, -np.inf             # u = inf dx - inf dy
    inf_map["itm"][0, 4] = -np.inf                                           # v = -inf dy
    inf_map["pos"][0] = (0, -0.25, 0)                                         # dy = v + 0.25 > 0 on the whole plane
    uvw = np.zeros((len(xy), 3), F); uvw[:, :2] = ((xy + F(1)).astype(F) / F(2)).astype(F)
    with np.errstate(invalid="ignore"):
        assert np.isnan(R.map_transform(nan_map["itm"][0], nan_map["pos"][0], uvw)[:, 0]).all()
        assert (R.map_transform(inf_map["itm"][0], inf_map["pos"][0], uvw)[:, 1] == -np.inf).all()
    for index in (0, 4, 6, 7):                                    # 1x1, 3x5, the golden image, the checker
        for which in (0, 1):
            pr.set_map(capi.identity_map(), index, which=1 - which)
            pr.maps["texture"][1 - which] = capi.MAP_NONE
            for m in (nan_map, inf_map):
                pr.set_map(m, index, which=which)
                hit, rgb, orgb = pr.shade(rays, p)
                # diffuse map: kd = 0 and the ambient term with it; specular map: ks = 0 under an ambient light adds nothing to kd = 1
                want = 0.0 if which == 0 else 1.0
                assert hit.all() and (rgb == want).all() and rgb.tobytes() == orgb.tobytes(), (pr.textures[index].name, which)
    pr.close()


# ---- the PROJ13 triangle's texture vertices -------------------------------------------------------------------------------
def _square_mesh():
    """the unit square as two triangles whose texture vertices lie outside [0, 1] and on texel boundaries of the 4 x 4 texture"""
    v = np.array([[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0]], F)
    f = np.array([[0, 1, 2], [0, 2, 3]], np.uint32)
    nodes, elements = capi.bvh_build(v, f)
    vt = np.array([[-0.25, -0.5, 0], [1.75, -0.5, 0], [1.75, 1.5, 0], [-0.25, 1.5, 0]], F)
    return dict(v=v, f=f, vn=np.array([[0, 0, 1]], F), fn=np.zeros((2, 3), np.uint32), nodes=nodes, elements=elements, vt=vt, ft=f.copy())


def test_proj13_triangles_read_their_texture_vertices():
    nodes = np.concatenate([scenes.identity_node(), scenes.identity_node(0, capi.OBJ_MESH, 0, 0)])
    pr = Probe(nodes, meshes=[_square_mesh()])
    g = np.arange(-15, 16) / F(16)                                # hit points on multiples of 1/16: uvw on multiples of 1/16 too
    gx, gy = np.meshgrid(g, g)
    rays = np.zeros((gx.size, 6), F); rays[:, 0], rays[:, 1], rays[:, 2], rays[:, 5] = gx.ravel(), gy.ravel(), 1, -1
    for index in (5, 4, 6):                                       # 4x4, 3x5, the golden image
        tex = pr.textures[index]
        pr.set_map(capi.identity_map(), index)
        p13 = capi.default_params(bounce=0, shade_model=capi.SHADE_P13)
        hit, rgb, orgb = pr.shade(rays, p13)
        ohit, ohits = orc.trace(pr.osc, capi.SHADE_P13, rays)
        uvw = ohits["uvw"]
        assert hit.all() and (uvw[:, 0] < 0).any() and (uvw[:, 0] > 1).any() and (uvw[:, 1] < 0).any() and (uvw[:, 1] > 1).any()
        want = R.sample(tex, pr.texels, uvw)
        assert np.abs(rgb - orgb).max() <= TOL and np.abs(rgb - want).max() <= TOL, tex.name
        if index == 5:
            ix, ixp, iy, iyp, fx, fy = R.file_texels(tex, uvw)
            assert ((fx == 0) & (fy == 0)).sum() >= 16              # lookups on texel corners
        # FIN's triangle never writes uvw: every hit looks up the stale (0.5, 0.5, 0.5)
        hit, rgb, orgb = pr.shade(rays, capi.default_params(bounce=0))
        stale = R.sample(tex, pr.texels, np.full((1, 3), 0.5, F))
        assert hit.all() and np.abs(rgb - orgb).max() <= TOL and np.abs(rgb - stale).max() <= TOL, tex.name
    pr.close()


# ---- the sphere -----------------------------------------------------------------------------------------------------------
def _sphere_nodes():
    return np.concatenate([scenes.identity_node(), scenes.identity_node(0, capi.OBJ_SPHERE, 0)])


def _sphere_tol(tex):
    return TOL + (max(tex.width, tex.height) * 2.0 ** -24 if tex.kind == R.FILE else 0.0)


def _sphere_check(pr, index, rays, p):
    """device against the oracle and against texture_ref at the oracle's hit point, every ray"""
    tex = pr.textures[index]
    pr.set_map(capi.identity_map(), index)
    hit, rgb, orgb = pr.shade(rays, p)
    ohit, ohits = orc.trace(pr.osc, p.shade_model, rays)
    want = R.sample(tex, pr.texels, R.sphere_coord(ohits["p"]))
    assert hit.all() and np.isfinite(rgb).all()
    worst = max(float(np.abs(rgb - orgb).max()), float(np.abs(rgb - want).max()))
    assert worst <= _sphere_tol(tex), (tex.name, worst)
    return rgb, ohits


def test_sphere_seam_axes_poles_and_rings():
    pr = Probe(_sphere_nodes())
    p = capi.default_params(bounce=0)
    edge = np.concatenate([R.seam_rays(), R.axis_rays()])
    # both sides of the seam, asked of the rays as the scene traces them (under its two nodes a -0 in the direction is lost)
    ohit, ohits = orc.trace(pr.osc, capi.SHADE_FIN, R.seam_rays())
    u, hp = ohits["uvw"][:, 0], ohits["p"]
    assert ohit.all() and (hp[:, 1] < 0).all() and (np.abs(hp[:, 0]) <= 1e-10).all()
    assert (u == 0).sum() >= 13 and (u == 1).sum() >= 13 and ((u == 0) | (u == 1)).all()
    assert (hp[u == 1, 0] < 0).all() and (hp[u == 0, 0] == 0).all()
    for index in (6, 4, 7):                                       # the golden image, 3x5, and at these points the checker too
        _sphere_check(pr, index, edge, p)
    for index in (6, 4):
        tex = pr.textures[index]
        v = np.arange(tex.height + 1) / tex.height                 # a ring at every v = texel boundary, 24 longitudes off the axes
        phi = (np.arange(24) + 0.37) * (2 * np.pi / 24)
        zz, ph = np.meshgrid(np.sin((v - 0.5) * np.pi), phi)
        r = np.sqrt(np.maximum(0.0, 1 - zz ** 2))
        pt = np.stack([r * np.cos(ph), r * np.sin(ph), zz], -1).reshape(-1, 3)
        _sphere_check(pr, index, np.concatenate([3 * pt, -pt], 1).astype(F), p)
    pr.close()


def test_sphere_next_to_the_poles_is_finite_and_the_poles_row():
    """Hit points whose float32 |z| exceeds 1 (rounding, within 2e-3 of a pole) made asin NaN: a NaN colour from a file texture.
    With asin's argument clamped they have the pole's v, where fy is 0: the colour is row 0's at their u."""
    rays = R.pole_rays()
    hit, hits = orc.sphere_intersect(capi.SHADE_FIN, rays, 1e30)
    z = hits["p"][:, 2]
    north, south = z > 1, z < -1
    assert hit.all() and north.sum() >= 1000 and south.sum() >= 1000
    rays = rays[north | south]
    pr = Probe(_sphere_nodes())
    tex = pr.textures[6]
    pr.set_map(capi.identity_map(), 6)
    got = pr.s.shade_rays(capi.default_params(bounce=0), rays)[1]
    print(f"{len(rays)} rays with |p.z| > 1: {int((~np.isfinite(got)).any(axis=1).sum())} of them not finite on the device")
    assert np.isfinite(got).all()
    rgb, ohits = _sphere_check(pr, 6, rays, capi.default_params(bounce=0))
    # the scene's root node rounds the direction once more ((p + d) - p), so the traced hit point is not sphere_intersect's:
    # the pole's row is asked of the rays whose traced |p.z| exceeds 1, again at least 1000 per pole
    pz = ohits["p"][:, 2]
    assert (pz > 1).sum() >= 1000 and (pz < -1).sum() >= 1000
    over = np.abs(pz) > 1
    u = R.sphere_coord(ohits["p"][over])
    pole = u.copy(); pole[:, 1] = np.where(pz[over] > 0, 1, 0)
    assert (u[:, 1] == pole[:, 1]).all()
    ix, ixp, iy, iyp, fx, fy = R.file_texels(tex, pole)
    assert (iy == 0).all() and (fy == 0).all()
    assert np.abs(rgb[over] - R.sample(tex, pr.texels, pole)).max() <= _sphere_tol(tex)
    pr.close()


def test_frame_over_the_pole_has_no_nan():
    """16 x 16 pixels onto the north pole from (0.4, -0.3, 5), so narrow that the whole frame lies in the cap where |p.z| rounds
    above 1 for a good part of the samples (asked of the oracle's primary rays: a condition on the inputs): the linear plane,
    which the denoiser, the history and the meter read, stays finite"""
    pr = Probe(_sphere_nodes())
    pr.set_map(capi.identity_map(), 6)
    pos = np.array([0.4, -0.3, 5.0])
    d = (np.array([0, 0, 1.0]) - pos) / np.linalg.norm(np.array([0, 0, 1.0]) - pos)
    cam = capi.Camera()
    for i in range(3):
        cam.pos[i], cam.dir[i], cam.up[i] = pos[i], d[i], (0, 1, 0)[i]
    cam.fov, cam.focaldist, cam.dof, cam.width, cam.height = 0.03, 1.0, 0.0, 16, 16
    oc = scenes.oracle_camera(cam)
    rays = np.stack([orc.primary_ray(oc, x, y, j) for y in range(16) for x in range(16) for j in range(4)])
    ohit, ohits = orc.trace(pr.osc, capi.SHADE_FIN, rays)
    over = (ohits["p"][:, 2] > 1).reshape(256, 4).any(axis=1)
    print(f"{int(over.sum())} of 256 pixels have a sample whose hit point lies above z = 1")
    assert ohit.all() and over.sum() >= 64
    rgb, z, cnt, lin, st, progress = pr.s.render_linear(cam, capi.default_params(bounce=0))
    assert progress == 256 and (z < 4.1).all() and (z > 3.9).all()
    print(f"{int(np.isnan(lin).any(axis=2).sum())} of 256 pixels hold a NaN")
    assert np.isfinite(lin).all() and (lin.max(axis=2) > 0).all()
    pr.close()


# ---- background and environment -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", ((8, 8), (7, 5)))
def test_background_lookup_of_the_resolve_kernel(size):
    """no object at all: every pixel misses and takes background.Sample(x / W, y / H, 0) -- on the 4 x 4 texture's texel
    boundaries at 8 x 8.  The linear plane against the oracle's lookup; the 8-bit frame is the host encode of that plane"""
    w, h = size
    textures, texels, rec = R.edge_store(capi.TEXTURE)
    s = capi.Scene()
    s.set_nodes(scenes.identity_node())
    s.set_materials(_material())
    s.set_lights(_light(capi.LIGHT_AMBIENT))
    s.set_textures(rec, texels)
    s.set_environment((1, 1, 1), (1, 1, 1))
    s.set_environment_maps(None, capi.identity_map(5))
    cam = capi.Camera()
    for i in range(3):
        cam.pos[i], cam.dir[i], cam.up[i] = (0, 0, 5)[i], (0, 0, -1)[i], (0, 1, 0)[i]
    cam.fov, cam.focaldist, cam.dof, cam.width, cam.height = 40.0, 1.0, 0.0, w, h
    p = capi.default_params()
    rgb, z, cnt, lin, st, progress = s.render_linear(cam, p)
    assert progress == w * h and (z > 1e29).all()
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    uvw = np.zeros((h * w, 3), F); uvw[:, 0], uvw[:, 1] = x.ravel().astype(F) / F(w), y.ravel().astype(F) / F(h)
    want = orc.texture_sample(R.records(textures, orc.TEXTURE)[5], texels, uvw).reshape(h, w, 3)
    assert np.abs(lin - want).max() <= TOL and np.abs(lin - R.sample(textures[5], texels, uvw).reshape(h, w, 3)).max() <= TOL
    if size == (8, 8):
        ix, ixp, iy, iyp, fx, fy = R.file_texels(textures[5], uvw)
        assert ((fx == 0) & (fy == 0)).sum() == 16 and len(np.unique(lin.reshape(-1, 3), axis=0)) >= 60
    assert rgb.tobytes() == encode_rgb8(lin, p.gamma).tobytes()
    s.close()


def _reflected(d, axis):
    """the direction MtlBlinn::Shade of PROJ13 gives the reflected ray, float32 in its order of operations, for a surface whose
    normal is the unit vector of `axis`: V = -d / |d|, R = N 2 clamp(N.V) - V, R / |R|"""
    def unit(v):
        n2 = ((v[:, 0] * v[:, 0]).astype(F) + (v[:, 1] * v[:, 1]).astype(F)).astype(F)
        return (v / np.sqrt((n2 + (v[:, 2] * v[:, 2]).astype(F)).astype(F))[:, None]).astype(F)
    V = -unit(np.asarray(d, F))
    Rr = -V
    Rr[:, axis] = ((F(2) * np.clip(V[:, axis], F(-1), F(1))).astype(F) - V[:, axis]).astype(F)
    return unit(Rr)


def test_environment_lookup_on_the_axes_and_straight_up():
    """a mirror plane (reflection = 1, nothing else) under PROJ13, whose reflected rays that leave the scene look up the
    environment: the plane's normal is the axis the wanted direction is largest along, the ray comes in as that direction's
    mirror image.  Axes, diagonals, dir.z = 0, straight up and down (0/0 in the reference: the map's centre here) -- asked of
    the reflected direction as the shader computes it (_reflected), not of the direction wanted."""
    dirs = R.environment_directions().astype(np.float64)
    p = capi.default_params(bounce=1, shade_model=capi.SHADE_P13)
    out = []
    for axis in range(3):
        cols = np.eye(3)[:, [(axis + 1) % 3, (axis + 2) % 3, axis]]              # local z -> the world axis
        nodes = np.concatenate([scenes.identity_node(), G.node(cols * 4.0, parent=0, obj=capi.OBJ_PLANE, material=0)])
        pr = Probe(nodes, _material(diffuse=0.0, specular=0.0, reflection=1.0))
        pr.s.set_environment((1, 1, 1), (0, 0, 0))
        pr.s.set_environment_maps(capi.identity_map(6), None)
        pr.osc = scenes.oracle_scene(pr.s.export())
        mine = dirs[np.abs(dirs).argmax(axis=1) == axis]
        d = mine.copy(); d[:, axis] = -d[:, axis]
        at = np.zeros(3); at[(axis + 1) % 3], at[(axis + 2) % 3] = 0.125, -0.25
        rays = np.concatenate([at - 2 * d, d], 1).astype(F)
        hit, rgb, orgb = pr.shade(rays, p)
        assert hit.all() and np.isfinite(rgb).all() and _close(rgb, orgb).all(), (axis, float(np.abs(rgb - orgb).max()))
        r = _reflected(rays[:, 3:], axis)
        assert np.abs(r - mine).max() <= 4 * 2.0 ** -24               # the reflected ray leaves in the direction wanted
        up = (r[:, 0] == 0) & (r[:, 1] == 0)
        if axis == 2:
            centre = R.sample(pr.textures[6], pr.texels, np.array([[0.5, 0.5, 0]], F))
            assert up.sum() == 2 and sorted(r[up, 2].tolist()) == [-1.0, 1.0]
            assert np.abs(rgb[up] - centre).max() <= TOL              # straight up and straight down: the map's centre
        # everywhere else the lookup is texture_ref's at the reflected direction: 8 ulp of the coordinate (float32 throughout
        # against float64) times the image's steepest slope, on top of the blend's 2e-6
        want = R.sample(pr.textures[6], pr.texels, R.environment_coord(r).astype(F))
        assert np.abs(rgb - want).max() <= TOL + 9 * 52 * 2.0 ** -24, float(np.abs(rgb - want).max())
        assert len(np.unique(rgb, axis=0)) > len(rays) // 2
        out.append(r)
        pr.close()
    r = np.concatenate(out)
    assert len(r) == len(dirs)
    assert ((np.abs(r) == 1).sum(axis=1) == 1).sum() == 6             # the six axis directions, exactly
    assert (r[:, 2] == 0).sum() >= 8                                  # the horizon, dir.z == 0: four axes and four diagonals
    assert ((np.abs(r[:, 0]) == np.abs(r[:, 1])) & (r[:, 0] != 0)).sum() >= 12      # the diagonals |x| == |y|
