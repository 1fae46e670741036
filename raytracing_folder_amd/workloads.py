"""Workload inputs of the render path, as the product ships them (bench.py, __graft_entry__.smoke() and the
tests all build their scenes here):

  * the Cornell box of the reference's photon-mapping snapshots (BASELINE config C4): data/cornell.xml +
    data/teapot_tri.obj, loaded through the product's own XML/OBJ loader; data/cornell_gi.xml is the variant
    RayTracingProj12's main() loads (config C3, live path-traced GI);
  * the stand-in for the absent christmas_balls.obj: 128 tessellated spheres
    (102 402 triangles with the ground quad) in two meshes, one of them mirrors, under a PNG sky that is both
    environment and background -- written as OBJ + PNG + XML and loaded the same way.
"""
import os
import tempfile

import numpy as np

from . import capi

DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data")
CORNELL_XML = os.path.join(DATA, "cornell.xml")
CORNELL_GI_XML = os.path.join(DATA, "cornell_gi.xml")


def load_cornell(width=None, height=None):
    """(scene, camera) of the Cornell box; width/height override the file's 800 x 600"""
    s = capi.Scene()
    s.load_xml(CORNELL_XML)
    cam = s.camera()
    if width:
        cam.width, cam.height = int(width), int(height)
    return s, cam


def load_cornell_gi(width=None, height=None):
    """(scene, camera) of BASELINE config C3: the scene RayTracingProj12's main() loads (its scene-2.xml: glass teapot, glossy
    sphere, point light 0.5 -- that snapshot's PointLight has no fall-off, include/lights.h:86-88), for shade model P12"""
    s = capi.Scene()
    s.load_xml(CORNELL_GI_XML)
    cam = s.camera()
    if width:
        cam.width, cam.height = int(width), int(height)
    return s, cam


def uv_sphere(nu, nv, center, radius):
    """nu x nv quads -> 2*nu*(nv-1) triangles (poles are fans)"""
    v = [[0, 0, 1]]
    for j in range(1, nv):
        th = np.pi * j / nv
        for i in range(nu):
            ph = 2 * np.pi * i / nu
            v.append([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)])
    v.append([0, 0, -1])
    v = np.array(v) * radius + np.array(center)
    f = []
    for i in range(nu):
        f.append([0, 1 + i, 1 + (i + 1) % nu])
    for j in range(nv - 2):
        a, b = 1 + j * nu, 1 + (j + 1) * nu
        for i in range(nu):
            i2 = (i + 1) % nu
            f.append([a + i, b + i, b + i2])
            f.append([a + i, b + i2, a + i2])
    last = len(v) - 1
    a = 1 + (nv - 2) * nu
    for i in range(nu):
        f.append([last, a + (i + 1) % nu, a + i])
    return v, np.array(f)


def balls_scene(n_balls=128, nu=20, nv=21, seed=1):
    """n_balls spheres of 2*nu*(nv-1) = 800 triangles each (102 400 for the defaults) + a ground quad"""
    rng = np.random.default_rng(seed)
    vs, fs, off = [], [], 0
    for _ in range(n_balls):
        c = [rng.uniform(-14, 14), rng.uniform(-25, 18), rng.uniform(1.0, 8.0)]
        v, f = uv_sphere(nu, nv, c, rng.uniform(0.6, 1.6))
        vs.append(v); fs.append(f + off); off += len(v)
    g = np.array([[-20, -30, 0], [20, -30, 0], [20, 25, 0], [-20, 25, 0]], float)
    vs.append(g); fs.append(np.array([[0, 1, 2], [0, 2, 3]]) + off)
    return np.concatenate(vs).astype(np.float32), np.concatenate(fs).astype(np.uint32)


def deform_wave(v, phase, amplitude):
    """the vertices of a deforming surface: along every axis a smooth sinusoidal displacement of `amplitude` (in the units of v)
    driven by the other two coordinates, about one wavelength across the mesh's extent; `phase` (radians) moves the wave.
    float32 in, float32 out, the same bytes for the same arguments."""
    v = np.asarray(v, np.float32).reshape(-1, 3).astype(np.float64)
    lo, hi = v.min(0), v.max(0)
    u = (v - lo) / np.where(hi > lo, hi - lo, 1.0)                  # every coordinate in [0, 1]
    d = np.stack([np.sin(2 * np.pi * (u[:, 1] + 0.37 * u[:, 2]) + phase + 0.4),
                  np.sin(2 * np.pi * (u[:, 2] + 0.53 * u[:, 0]) + 1.7 * phase + 1.3),
                  np.sin(2 * np.pi * (u[:, 0] + 0.71 * u[:, 1]) + 0.6 * phase + 2.2)], 1)
    return (v + float(amplitude) * d).astype(np.float32)


def bone_chain(v, n_bones, axis=0):
    """a skin for vertices v (Scene.set_mesh_skin): n_bones bones evenly spaced along `axis` over the mesh's extent, every vertex
    weighted linearly between its two nearest bones, the other two influences weight 0 (on bone 0).  Returns bone_index uint16
    (nv, 4) and weight float32 (nv, 4)."""
    v = np.asarray(v, np.float32).reshape(-1, 3).astype(np.float64)
    n_bones = int(n_bones)
    x = v[:, axis]
    lo, hi = x.min(), x.max()
    t = (x - lo) / (hi - lo if hi > lo else 1.0) * (n_bones - 1)       # the vertex in bone spacings: bone b sits at t = b
    b0 = np.clip(np.floor(t).astype(np.int64), 0, max(n_bones - 2, 0))
    b1 = np.minimum(b0 + 1, n_bones - 1)
    w1 = (t - b0) if n_bones > 1 else np.zeros_like(t)
    index = np.zeros((len(v), 4), np.uint16)
    weight = np.zeros((len(v), 4), np.float32)
    index[:, 0], index[:, 1] = b0, b1
    weight[:, 0], weight[:, 1] = 1.0 - w1, w1
    return index, weight


def chain_pose(n_bones, angle, origin, axis):
    """a pose for bone_chain's skin (Scene.pose_mesh): a cumulative bend of `angle` radians per joint about the direction `axis`
    through `origin` -- bone 0 stays, bone b is bone b - 1's transform followed by one more rotation -- composed in float64 and
    rounded once.  float32 (n_bones, 3, 4), row-major [R | t]."""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    o = np.asarray(origin, np.float64)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)     # Rodrigues
    step = np.eye(4)
    step[:3, :3], step[:3, 3] = R, o - R @ o
    out, M = np.zeros((int(n_bones), 3, 4), np.float64), np.eye(4)
    for b in range(int(n_bones)):
        out[b] = M[:3]
        M = step @ M
    return out.astype(np.float32)


def morph_targets(v, n_targets, amplitude=0.15, seed=0):
    """a morph set for vertices v (Scene.set_mesh_morphs): target t moves the vertices within a seeded radius (0.15 .. 0.45 of the
    mesh's extent, its largest side) of a seeded centre vertex along a seeded unit direction, by amplitude x extent at the centre
    with the smooth falloff (1 - (d / radius)^2)^2 that is exactly 0 from the radius on -- dense and mostly zero, as real blend
    shapes are.  Returns deltas float32 (n_targets, nv, 3)."""
    v = np.asarray(v, np.float32).reshape(-1, 3).astype(np.float64)
    rng = np.random.default_rng(seed)
    extent = float((v.max(0) - v.min(0)).max()) or 1.0
    out = np.zeros((int(n_targets), len(v), 3), np.float32)
    for t in range(int(n_targets)):
        centre = v[rng.integers(0, len(v))]
        radius = rng.uniform(0.15, 0.45) * extent
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        r2 = ((v - centre) ** 2).sum(1) / (radius * radius)
        fall = np.where(r2 < 1.0, (1.0 - r2) ** 2, 0.0)
        out[t] = (float(amplitude) * extent * fall[:, None] * d).astype(np.float32)
    return out


def sheet(n, extent):
    """an open sheet of n x n quads in the plane z = 0, |x|, |y| <= extent / 2: (n + 1)^2 shared vertices, 2 n^2 triangles wound
    so that the face normals point to +z.  float32 (nv, 3), uint32 (nf, 3); sheet(1) is one leaf of the device tree"""
    n = int(n)
    t = np.linspace(-0.5 * float(extent), 0.5 * float(extent), n + 1)
    x, y = np.meshgrid(t, t)
    v = np.stack([x.ravel(), y.ravel(), np.zeros((n + 1) ** 2)], 1).astype(np.float32)
    j, i = np.mgrid[0:n, 0:n]
    a = (j * (n + 1) + i).ravel()
    f = np.concatenate([np.stack([a, a + 1, a + n + 2], 1), np.stack([a, a + n + 2, a + n + 1], 1)]).astype(np.uint32)
    return v, f


def write_obj(path, v, f):
    with open(path, "w") as o:
        for p in v:
            o.write("v %.9g %.9g %.9g\n" % tuple(p))
        for t in f:
            o.write("f %d %d %d\n" % (t[0] + 1, t[1] + 1, t[2] + 1))


def sky_image(width=256, height=128):
    """a smooth sky: zenith blue -> pale horizon -> brown ground, with a warm spot (a PNG environment stands in for
    the reference's absent HDRI; TexturedColor::SampleEnvironment maps directions onto it, scene.h:426-432)"""
    y, x = np.mgrid[0:height, 0:width].astype(np.float64)
    t = y / (height - 1)
    top, hor, gnd = np.array([0.25, 0.45, 0.9]), np.array([0.85, 0.9, 1.0]), np.array([0.35, 0.3, 0.25])
    up = np.clip(t / 0.55, 0, 1)[..., None]
    img = np.where((t < 0.55)[..., None], top * (1 - up) + hor * up, gnd)
    sun = np.exp(-(((x - 0.7 * width) / (0.05 * width)) ** 2 + ((y - 0.3 * height) / (0.08 * height)) ** 2))[..., None]
    img = np.clip(img + sun * np.array([1.0, 0.9, 0.6]), 0, 1)
    return (img * 255).astype(np.uint8)


def make_balls_scene(width, height, n_balls=64, directory=None):
    """C5 stand-in: two meshes of n_balls tessellated spheres each (the first with the ground quad), matte and
    mirror materials, ambient + point light, PNG sky as environment AND background.  Returns (scene, camera)."""
    d = directory or tempfile.mkdtemp(prefix="rt_balls_")
    va, fa = balls_scene(n_balls=n_balls, seed=1)               # n balls + the ground quad
    vb, fb = balls_scene(n_balls=n_balls, seed=2)
    vb, fb = vb[:-4], fb[:-2]                                   # the second group without a second ground
    write_obj(os.path.join(d, "balls_a.obj"), va, fa)
    write_obj(os.path.join(d, "balls_b.obj"), vb, fb)
    capi.image_write_png(os.path.join(d, "sky.png"), sky_image())
    with open(os.path.join(d, "scene.xml"), "w") as f:
        f.write(f"""<xml><scene>
  <background value="1" texture="sky.png"/><environment value="1" texture="sky.png"/>
  <object type="obj" name="balls_a.obj" material="matte"/>
  <object type="obj" name="balls_b.obj" material="mirror"/>
  <material type="blinn" name="matte"><diffuse r="0.8" g="0.5" b="0.3"/><specular value="0.4"/><glossiness value="30"/></material>
  <material type="blinn" name="mirror"><diffuse value="0.1"/><specular value="0.9"/><glossiness value="80"/><reflection value="0.8"/></material>
  <light type="ambient" name="amb"><intensity value="0.2"/></light>
  <light type="point" name="sun"><intensity value="1800"/><position x="10" y="-30" z="40"/></light>
</scene><camera><position x="0" y="-52" z="20"/><target x="0" y="-4" z="3"/><up x="0" y="0" z="1"/>
  <fov value="35"/><width value="{int(width)}"/><height value="{int(height)}"/></camera></xml>""")
    s = capi.Scene()
    s.load_xml(os.path.join(d, "scene.xml"))
    return s, s.camera()
