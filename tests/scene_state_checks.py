"""What the tests of rtk_accel_set_lights / _set_materials / _set_background share (test_gpu_scene_state.py): scenes with a part
replaced (dataclasses.replace on the oracle's flat scene), the setters fed from such a scene, the CPU oracle's frame of every
state (computed once per shape, never changed), and the synthetic scene whose leaves have chosen sizes."""
import dataclasses

import numpy as np

from views_checks import bits, same  # noqa: F401  (re-exported)

DIFFUSE, REFLECTIVE, REFRACTIVE, CONSTANT, TEXTURE = range(5)


def with_lights(flat, pos, inten):
    return dataclasses.replace(flat, light_pos=np.ascontiguousarray(pos, np.float32).reshape(-1, 3),
                               light_intensity=np.ascontiguousarray(inten, np.float32).reshape(-1))


def with_material(flat, mat, kind=None, albedo=None, ior=None, smooth=None, texture=None):
    """`flat` with row `mat` of the material table changed; a kind other than TEXTURE stores texture -1, as the library does."""
    k, a, i, s = flat.mat_kind.copy(), flat.mat_albedo.copy(), flat.mat_ior.copy(), flat.mat_smooth.copy()
    t = None if flat.mat_texture is None else flat.mat_texture.copy()
    if kind is not None:
        k[mat] = kind
        if t is not None and kind != TEXTURE:
            t[mat] = -1
    if albedo is not None:
        a[mat] = albedo
    if ior is not None:
        i[mat] = ior
    if smooth is not None:
        s[mat] = smooth
    if texture is not None:
        t[mat] = texture
    return dataclasses.replace(flat, mat_kind=k, mat_albedo=a, mat_ior=i, mat_smooth=s, mat_texture=t)


def set_lights(acc, flat):
    acc.set_lights(flat.light_pos, flat.light_intensity)


def set_materials(acc, flat):
    acc.set_materials(flat.mat_kind, flat.mat_albedo, flat.mat_ior, flat.mat_smooth, flat.mat_texture)


def light_states(flat):
    """The scene's lights; one of them moved; nine, among them intensities 0, negative and 1e-30; none; the scene's again."""
    p, i = flat.light_pos.astype(np.float32), flat.light_intensity.astype(np.float32)
    moved = p.copy()
    moved[0] = moved[0] + np.array([-6.0, 3.0, 5.0], np.float32)
    rng = np.random.default_rng(11)
    p9 = np.concatenate([p, rng.uniform([-12, 6, -12], [12, 18, 12], (5, 3)).astype(np.float32)])
    i9 = np.concatenate([i, np.array([0.0, -300.0, 1e-30, 800.0, 250.0], np.float32)])
    assert len(i) == 4 and len(i9) == 9
    return [("own", flat), ("moved", with_lights(flat, moved, i)), ("nine", with_lights(flat, p9, i9)),
            ("none", with_lights(flat, np.zeros((0, 3)), np.zeros(0))), ("own again", flat)]


def scene5_material_states(flat):
    """hw09/scene5: material 0 is the floor (reflective), 1 the dragon (diffuse).  The dragon diffuse -> reflective -> refractive
    (ior 1.5) -> constant -> diffuse with another albedo and flat shading; then the floor reflective -> diffuse."""
    assert flat.mat_kind.tolist() == [REFLECTIVE, DIFFUSE] and flat.mesh_material.tolist() == [0, 1]
    s1 = with_material(flat, 1, kind=REFLECTIVE)
    s2 = with_material(flat, 1, kind=REFRACTIVE, ior=1.5)
    s3 = with_material(s2, 1, kind=CONSTANT)
    s4 = with_material(s3, 1, kind=DIFFUSE, albedo=[0.2, 0.7, 0.4], smooth=0)
    s5 = with_material(s4, 0, kind=DIFFUSE, smooth=0)
    return [("own", flat), ("dragon reflective", s1), ("dragon refractive", s2), ("dragon constant", s3),
            ("dragon diffuse flat", s4), ("floor diffuse", s5)]


class States:
    """oracle frames of named scenes; every accel and every frame is made once"""

    def __init__(self, ora):
        self.ora = ora
        self._acc = {}
        self._frames = {}

    def accel(self, key, flat):
        if key not in self._acc:
            self._acc[key] = self.ora.Accel(self.ora.Scene(flat), self.ora.ACCEL_KD_SIMD)
        return self._acc[key]

    def frame(self, key, flat, w, h, spp=1, depth=5, gi=0):
        k = (key, w, h, spp, depth, gi)
        if k not in self._frames:
            rgb, cn = self.accel(key, flat).render(w, h, spp, depth, gi)
            rgb.setflags(write=False)
            self._frames[k] = (rgb, cn)
        return self._frames[k]


# ---------------------------------------------------------------- leaves of chosen sizes

LEAF_SIZES = (1, 63, 64, 65, 130, 200, 20, 40)      # triangles per octant of the scene box, octant o = (x > 0) + 2 (y > 0) + 4 (z > 0)
ONLY_A, ONLY_B = 7, 6                               # octants whose triangles all belong to mesh A (material 0) / mesh B (material 1)
TREE = dict(max_depth=3, max_leaf_size=1)           # x, y, z are split once each at the box's midpoint: the leaves are the octants


def octant_scene(ora, seed=7):
    """Two meshes, one material each, whose triangles interleave in space: small triangles in clusters, one cluster per octant of
    [-4, 4]^3, kept clear of the three midplanes, so with TREE every octant is one leaf that holds exactly its cluster.  Octant 0
    holds a single triangle (of A); ONLY_A / ONLY_B hold one mesh alone; everywhere else a triangle is A's or B's by coin toss.
    Light and camera stand outside, so that shadow rays cross several clusters."""
    rng = np.random.default_rng(seed)
    tris, owner, octant = [], [], []
    for o, n in enumerate(LEAF_SIZES):
        sign = np.array([1.0 if o & 1 else -1.0, 1.0 if o & 2 else -1.0, 1.0 if o & 4 else -1.0])
        c = rng.uniform(1.0, 3.5, (n, 1, 3)) * sign
        t = c + rng.uniform(-0.3, 0.3, (n, 3, 3))
        if o == 0:
            t[0] = np.array([[-4.0, -4.0, -4.0], [-3.4, -4.0, -3.7], [-3.7, -3.4, -4.0]])   # pins the box's low corner
        if o == 7:
            t[0] = np.array([[4.0, 4.0, 4.0], [3.4, 4.0, 3.7], [3.7, 3.4, 4.0]])            # ... and its high corner
        who = rng.integers(0, 2, n)
        if o in (0, ONLY_A):
            who[:] = 0
        if o == ONLY_B:
            who[:] = 1
        tris.append(t)
        owner.append(who)
        octant.append(np.full(n, o))
    tris, owner, octant = np.concatenate(tris), np.concatenate(owner), np.concatenate(octant)
    va, vb = tris[owner == 0].reshape(-1, 3), tris[owner == 1].reshape(-1, 3)
    na, nb = len(va) // 3, len(vb) // 3
    flat = ora.FlatScene(
        mesh_material=np.array([0, 1], np.int32), mesh_nverts=np.array([3 * na, 3 * nb], np.int32),
        mesh_ntris=np.array([na, nb], np.int32), vertices=np.concatenate([va, vb]).astype(np.float32),
        indices=np.concatenate([np.arange(3 * na, dtype=np.uint32).reshape(na, 3), np.arange(3 * nb, dtype=np.uint32).reshape(nb, 3)]),
        mat_kind=np.array([DIFFUSE, DIFFUSE], np.int32), mat_albedo=np.array([[0.9, 0.5, 0.3], [0.3, 0.6, 0.9]], np.float32),
        mat_ior=np.array([1.5, 1.3], np.float32), mat_smooth=np.zeros(2, np.int32),
        light_pos=np.array([[9.0, 11.0, 10.0], [-10.0, 3.0, -9.0]], np.float32), light_intensity=np.array([900.0, 700.0], np.float32),
        cam_pos=np.array([0.0, 0.0, 12.0], np.float32), cam_mat=np.array([1, 0, 0, 0, 1, 0, 0, 0, 1], np.float32),
        background=np.array([0.05, 0.1, 0.2], np.float32), width=64, height=64, bucket_size=64)
    # global triangle id -> octant and owner, in the accel's order (A's triangles first)
    tri_octant = np.concatenate([octant[owner == 0], octant[owner == 1]])
    tri_owner = np.concatenate([np.zeros(na, np.int64), np.ones(nb, np.int64)])
    return flat, tri_octant, tri_owner


def leaves_of(link, refs):
    """The leaves of a tree dump as lists of global triangle ids."""
    return [refs[s:s + c] for _, _, s, c in link if s >= 0]
