"""Generated scenes for the shading edge cases that no scene file reaches (tests/test_material_scenes.py,
tests/test_gpu_material_scenes.py, tools/make_ref_probe_fixtures.py).  A helper, not a test.

One geometry, 48 x 32 pixels: a floor; a back mirror that faces a mirror behind the camera, and two side mirrors that face
each other (reflection chains run to the depth limit: the back mirror shows between the two rows of quads, at the camera's
height); a flat-shaded glass box around a smooth-shaded glass octahedron (hn != fn); a constant quad; a black quad; two rows of
quads whose vertex uvs run past [0, 1] with grid lines at exactly 0 and 1, the lower row partly behind the glass; and a pyramid
without uvs.  The variants
differ in materials and lights alone, so one accel can be walked through them with set_materials / set_lights:

  name          outer ior, inner ior   lights besides the two base lights
  ior15_075     1.5, 0.75              one of intensity 0
  ior075_15     0.75, 1.5              one of negative intensity
  ior10_00      1.0, 0.0               one exactly on the floor
  ior24_10      2.4, 1.0               one inside the glass box
  ior15_m15     1.5, -1.5              none
  swapped       1.5, 0.75              none; the box is smooth-shaded and the octahedron flat
  textured      1.5, 0.75              all of the above and more, nine in all; floor, quads and pyramid carry textures

Bitmap lookups convert a float to size_t in the reference, which is undefined below -1: uvs stay within -1/64 on the low side of
u and 1 + 1/64 on the high side of v (the largest bitmap is 16 x 16), and go far past on the other sides.

Everything is deterministic.  Nothing here looks at what the code under test computes: rays are aimed by geometry, and where a
family is selected (`leaving`), it is by the oracle's closest hit and the numpy restatement of refract_at's inequality below;
the critical rays take the shading normal they are measured against from the oracle's hit."""
import numpy as np

from occlusion_model import dot3, normalized3
from radiance_views import ViewBatch, jittered_views

MISS = 0xFFFFFFFF
DIFFUSE, REFLECTIVE, REFRACTIVE, CONSTANT, TEXTURE = range(5)
ALBEDO, EDGES, CHECKER, BITMAP = range(4)
SIZE = (48, 32)
DEPTHS = (1, 5, 10, 16)
RAD_DEPTHS = (5, 16)
VARIANTS = ("ior15_075", "ior075_15", "ior10_00", "ior24_10", "ior15_m15", "swapped", "textured")
GLASS_VARIANTS = VARIANTS[:6]
IORS = {"ior15_075": (1.5, 0.75), "ior075_15": (0.75, 1.5), "ior10_00": (1.0, 0.0), "ior24_10": (2.4, 1.0),
        "ior15_m15": (1.5, -1.5), "swapped": (1.5, 0.75), "textured": (1.5, 0.75)}

# meshes, in order
FLOOR, MIRROR_BACK, MIRROR_LEFT, MIRROR_RIGHT, BOX, OCTA, CONST_QUAD, BLACK_QUAD = range(8)
QUADS = tuple(range(8, 16))              # lower row 8..11 at z = -4, upper row 12..15 at z = -5
PYRAMID = 16
MIRROR_FRONT = 17                        # behind the camera, facing the back mirror
# materials
M_FLOOR, M_MIRROR, M_OUTER, M_INNER, M_CONST, M_BLACK = range(6)
M_QUADS = tuple(range(6, 14))
M_PYRAMID = 14
N_MATERIALS = 15
# textures: albedo | edges 0, 0.05, 0.4 | checker 2^-2 | bitmaps 1 x 1, 3 x 5, 16 x 16
T_ALBEDO, T_EDGE0, T_EDGE005, T_EDGE04, T_CHECKER, T_BMP1, T_BMP3X5, T_BMP16 = range(8)
BITMAP_SIZES = {T_BMP1: (1, 1), T_BMP3X5: (3, 5), T_BMP16: (16, 16)}              # width, height
TEXTURE_OF = {M_FLOOR: T_CHECKER, M_QUADS[0]: T_EDGE005, M_QUADS[1]: T_BMP16, M_QUADS[2]: T_CHECKER, M_QUADS[3]: T_BMP3X5,
              M_QUADS[4]: T_ALBEDO, M_QUADS[5]: T_EDGE0, M_QUADS[6]: T_EDGE04, M_QUADS[7]: T_BMP1, M_PYRAMID: T_BMP16}
U_LINES = (-1.0 / 64, 0.0, 1.0, 1.5)
V_LINES = (-0.5, 0.0, 1.0, 1.0 + 1.0 / 64)

BOX_LO, BOX_HI = np.array([-2.0, -1.5, -2.0]), np.array([2.0, 2.5, 2.0])
OCTA_C, OCTA_R = np.array([0.0, 0.5, 0.0]), 1.25
FLOOR_Y = -2.0


def _grid(p0, du, dv):
    """A quad p0 + s du + t dv as 3 x 3 cells; the vertex uvs of the grid lines are U_LINES x V_LINES.  Normal: du x dv."""
    p0, du, dv = (np.asarray(a, np.float64) for a in (p0, du, dv))
    pos = (0.0, 1.0 / 3, 2.0 / 3, 1.0)
    v = [p0 + pos[i] * du + pos[j] * dv for j in range(4) for i in range(4)]
    uv = [(U_LINES[i], V_LINES[j]) for j in range(4) for i in range(4)]
    t = []
    for j in range(3):
        for i in range(3):
            a = j * 4 + i
            t += [[a, a + 1, a + 5], [a, a + 5, a + 4]]
    return v, t, uv


def _quad(p0, du, dv):
    p0, du, dv = (np.asarray(a, np.float64) for a in (p0, du, dv))
    return [p0, p0 + du, p0 + du + dv, p0 + dv], [[0, 1, 2], [0, 2, 3]], None


def _box(lo, hi):
    v = [[(lo, hi)[i][0], (lo, hi)[j][1], (lo, hi)[k][2]] for k in range(2) for j in range(2) for i in range(2)]   # index = i + 2 j + 4 k
    t = [[4, 5, 7], [4, 7, 6],          # z = hi, normal +z
         [1, 0, 2], [1, 2, 3],          # z = lo, normal -z
         [5, 1, 3], [5, 3, 7],          # x = hi, normal +x
         [0, 4, 6], [0, 6, 2],          # x = lo, normal -x
         [6, 7, 3], [6, 3, 2],          # y = hi, normal +y
         [0, 1, 5], [0, 5, 4]]          # y = lo, normal -y
    return v, t, None


def _octahedron(c, r):
    v = [c + r * np.array(a, np.float64) for a in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))]
    t = [[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]]
    return v, t, None


def _pyramid(c, r, h):
    c = np.asarray(c, np.float64)
    v = [c + np.array(a, np.float64) for a in ((-r, 0, r), (r, 0, r), (r, 0, -r), (-r, 0, -r), (0, h, 0))]
    return v, [[0, 1, 4], [1, 2, 4], [2, 3, 4], [3, 0, 4]], None


def _meshes():
    """[(vertices, triangles, uvs or None, material)] in mesh order"""
    out = [None] * 18
    out[FLOOR] = _grid([-8, FLOOR_Y, 8], [16, 0, 0], [0, 0, -14]) + (M_FLOOR,)
    out[MIRROR_BACK] = _quad([-8, FLOOR_Y, -6], [16, 0, 0], [0, 11, 0]) + (M_MIRROR,)
    out[MIRROR_LEFT] = _quad([-8, FLOOR_Y, 8], [0, 0, -14], [0, 11, 0]) + (M_MIRROR,)
    out[MIRROR_RIGHT] = _quad([8, FLOOR_Y, -6], [0, 0, 14], [0, 11, 0]) + (M_MIRROR,)
    out[BOX] = _box(BOX_LO, BOX_HI) + (M_OUTER,)
    out[OCTA] = _octahedron(OCTA_C, OCTA_R) + (M_INNER,)
    out[CONST_QUAD] = _quad([2.5, FLOOR_Y, 3.5], [3, 0, 0], [0, 2.5, 0]) + (M_CONST,)
    out[BLACK_QUAD] = _quad([-5.5, FLOOR_Y, 3.5], [3, 0, 0], [0, 2.5, 0]) + (M_BLACK,)
    for i in range(4):
        out[QUADS[i]] = _grid([-8 + 4 * i, FLOOR_Y, -4], [4, 0, 0], [0, 5, 0]) + (M_QUADS[i],)
        out[QUADS[4 + i]] = _grid([-8 + 4 * i, 4, -5], [4, 0, 0], [0, 6, 0]) + (M_QUADS[4 + i],)
    out[PYRAMID] = _pyramid([-1.5, FLOOR_Y, 4.25], 0.75, 1.5) + (M_PYRAMID,)
    out[MIRROR_FRONT] = _quad([8, FLOOR_Y, 9.5], [-16, 0, 0], [0, 11, 0]) + (M_MIRROR,)
    return out


BASE_LIGHTS = [((3.0, 8.0, 6.0), 900.0), ((-4.0, 6.0, 2.0), 600.0)]
L_ZERO = ((1.0, 7.0, 3.0), 0.0)
L_NEGATIVE = ((-2.0, 5.0, 5.0), -300.0)
L_ON_FLOOR = ((1.0, FLOOR_Y, 6.0), 400.0)
L_IN_GLASS = ((1.5, 2.0, 1.5), 200.0)
LIGHTS = {"ior15_075": BASE_LIGHTS + [L_ZERO], "ior075_15": BASE_LIGHTS + [L_NEGATIVE], "ior10_00": BASE_LIGHTS + [L_ON_FLOOR],
          "ior24_10": BASE_LIGHTS + [L_IN_GLASS], "ior15_m15": BASE_LIGHTS, "swapped": BASE_LIGHTS,
          "textured": BASE_LIGHTS + [L_ZERO, L_NEGATIVE, L_ON_FLOOR, L_IN_GLASS, ((0.0, 9.0, -3.0), 500.0), ((5.0, 1.0, 7.0), 150.0),
                                     ((-5.0, 4.0, -5.0), 250.0)]}


def _textures():
    rng = np.random.default_rng(2024)
    kind = np.array([ALBEDO, EDGES, EDGES, EDGES, CHECKER, BITMAP, BITMAP, BITMAP], np.int32)
    a = rng.uniform(0.1, 1.0, (8, 3)).astype(np.float32)
    b = rng.uniform(0.1, 1.0, (8, 3)).astype(np.float32)
    param = np.array([0, 0.0, 0.05, 0.4, 0.25, 0, 0, 0], np.float32)
    bitmap, pixels, off = np.zeros((8, 3), np.int32), [], 0
    for t, (w, h) in BITMAP_SIZES.items():
        a[t] = b[t] = 0
        bitmap[t] = (off, w, h)
        pixels.append(rng.integers(0, 256, w * h * 3, dtype=np.uint8))
        off += w * h * 3
    b[T_ALBEDO] = 0
    return kind, a, b, param, np.concatenate(pixels), bitmap


def material_rows(name):
    """-> dict(kind, albedo, ior, smooth, texture) of variant `name`: what set_materials takes"""
    rng = np.random.default_rng(7)
    kind = np.full(N_MATERIALS, DIFFUSE, np.int32)
    albedo = rng.uniform(0.2, 1.0, (N_MATERIALS, 3)).astype(np.float32)
    ior = np.ones(N_MATERIALS, np.float32)
    smooth = np.zeros(N_MATERIALS, np.int32)
    texture = np.full(N_MATERIALS, -1, np.int32)
    kind[M_MIRROR], kind[M_OUTER], kind[M_INNER], kind[M_CONST] = REFLECTIVE, REFRACTIVE, REFRACTIVE, CONSTANT
    albedo[M_OUTER] = albedo[M_INNER] = albedo[M_BLACK] = 0
    ior[M_OUTER], ior[M_INNER] = IORS[name]
    smooth[M_INNER] = 1
    smooth[M_QUADS[0]] = smooth[M_PYRAMID] = 1                 # the cosine law's normal of a texture material follows the flag too
    if name == "swapped":
        smooth[M_OUTER], smooth[M_INNER] = 1, 0
    if name == "textured":
        for m, t in TEXTURE_OF.items():
            kind[m], texture[m], albedo[m] = TEXTURE, t, 0
    return dict(kind=kind, albedo=albedo, ior=ior, smooth=smooth, texture=texture)


def light_rows(name):
    pos = np.array([p for p, _ in LIGHTS[name]], np.float32).reshape(-1, 3)
    return pos, np.array([i for _, i in LIGHTS[name]], np.float32)


def make_scene(ora, name):
    """-> ora.FlatScene of variant `name`"""
    meshes = _meshes()
    uvs, has = [], []
    for v, t, uv, m in meshes:
        has.append(0 if uv is None else 1)
        if uv is not None:
            uvs.append(np.asarray(uv, np.float32))
    rows = material_rows(name)
    tk, ta, tb, tp, px, bm = _textures()
    lp, li = light_rows(name)
    c, s = np.cos(0.25), np.sin(0.25)
    return ora.FlatScene(
        mesh_material=np.array([m for *_, m in meshes], np.int32), mesh_nverts=np.array([len(v) for v, *_ in meshes], np.int32),
        mesh_ntris=np.array([len(t) for _, t, *_ in meshes], np.int32),
        vertices=np.ascontiguousarray(np.concatenate([np.asarray(v, np.float64) for v, *_ in meshes]), np.float32),
        indices=np.ascontiguousarray(np.concatenate([np.asarray(t) for _, t, *_ in meshes]), np.uint32),
        mat_kind=rows["kind"], mat_albedo=rows["albedo"], mat_ior=rows["ior"], mat_smooth=rows["smooth"],
        light_pos=lp, light_intensity=li, cam_pos=np.array([0.0, 3.5, 9.0], np.float32),
        cam_mat=np.array([1, 0, 0, 0, c, -s, 0, s, c], np.float32), background=np.array([0.1, 0.3, 0.2], np.float32),
        width=SIZE[0], height=SIZE[1], bucket_size=16, mat_texture=rows["texture"], uvs=np.ascontiguousarray(np.concatenate(uvs)),
        mesh_has_uvs=np.array(has, np.int32), tex_kind=tk, tex_color_a=ta, tex_color_b=tb, tex_param=tp, tex_pixels=px, tex_bitmap=bm)


SCENE_ARRAYS = ("mesh_material", "mesh_nverts", "mesh_ntris", "vertices", "indices", "mat_kind", "mat_albedo", "mat_ior", "mat_smooth",
                "mat_texture", "uvs", "mesh_has_uvs", "tex_kind", "tex_color_a", "tex_color_b", "tex_param", "tex_pixels", "tex_bitmap",
                "light_pos", "light_intensity", "cam_pos", "cam_mat", "background")


def scene_arrays(flat):
    """name -> array: everything the scene is made of, as stored beside the recorded outputs"""
    return {"scene_" + k: np.ascontiguousarray(getattr(flat, k)) for k in SCENE_ARRAYS}


def rtk_scene(rtk, f):
    """rtk.Scene.from_arrays of a flat scene, texture tables, texels and uvs included"""
    return rtk.Scene.from_arrays(f.mesh_material, f.mesh_nverts, f.mesh_ntris, f.vertices, f.indices, f.mat_kind, f.mat_albedo,
                                 f.mat_ior, f.mat_smooth, f.light_pos, f.light_intensity, f.cam_pos, f.cam_mat, f.background,
                                 f.width, f.height, f.bucket_size, mat_texture=f.mat_texture, uvs=f.uvs, mesh_has_uvs=f.mesh_has_uvs,
                                 tex_kind=f.tex_kind, tex_color_a=f.tex_color_a, tex_color_b=f.tex_color_b, tex_param=f.tex_param,
                                 tex_pixels=f.tex_pixels, tex_bitmap=f.tex_bitmap)


# ---------------------------------------------------------------- what refract_at decides, in numpy float32

def shading_normal(flat, hits, rest):
    """`mat->smooth ? hn : fn` of every hit (rows of a miss: zeros)"""
    hit = hits["mesh"] != MISS
    mat = flat.mesh_material[np.where(hit, hits["mesh"], 0)]
    return np.where((flat.mat_smooth[mat] != 0)[:, None], hits["normal"], rest["face_normal"]).astype(np.float32)


def refraction_case(flat, rays, hits, rest):
    """The branch of refract_at (render.hpp:252-266) every ray's closest hit takes -> (refractive bool[n], leaving bool[n]:
    0 < dot(i, n), tir bool[n]: eta_r / eta_i < sin_i_n), the arithmetic in float32 and in the reference's order."""
    hit = hits["mesh"] != MISS
    mat = flat.mesh_material[np.where(hit, hits["mesh"], 0)]
    refractive = hit & (flat.mat_kind[mat] == REFRACTIVE)
    with np.errstate(all="ignore"):
        n = normalized3(shading_normal(flat, hits, rest))
        i = normalized3(np.ascontiguousarray(rays[:, 3:6], np.float32))
        leaving = np.float32(0) < dot3(i, n)
        eta_i = np.where(leaving, flat.mat_ior[mat], np.float32(1)).astype(np.float32)
        eta_r = np.where(leaving, np.float32(1), flat.mat_ior[mat]).astype(np.float32)
        n = np.where(leaving[:, None], -n, n)
        cos_i = -dot3(i, n)
        sin_i = np.sqrt(np.float32(1) - cos_i * cos_i, dtype=np.float32)
        tir = eta_r / eta_i < sin_i
    return refractive, refractive & leaving, refractive & tir


# ---------------------------------------------------------------- radiance rays a camera cannot produce

def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _tangent_frame(n):
    a = np.array([1.0, 0, 0]) if abs(n[0]) < 0.9 else np.array([0, 1.0, 0])
    t = _unit(np.cross(n, a))
    return t, np.cross(n, t)


DELTAS = (-1e-2, -1e-4, -1e-6, 1e-6, 1e-4, 1e-2)       # rad, about the critical angle; a float32 direction resolves about 1e-7
N_AZ = 8


def _shading_normal_at(oacc, flat, point, fn):
    """`mat->smooth ? hn : fn` of the surface point `point` of a glass face with outward face normal `fn`, from the oracle's hit of
    a ray along -fn: on a smooth mesh refract_at measures its angles against the interpolated normal, so rays are aimed with it."""
    ray = np.concatenate([point + 0.25 * fn, -fn]).astype(np.float32)[None, :]
    hits, rest = oacc.intersect(ray, False), oacc.intersect_rest(ray, False)
    assert flat.mat_kind[flat.mesh_material[hits["mesh"][0]]] == REFRACTIVE
    return _unit(shading_normal(flat, hits, rest)[0])


def _critical_rays(point, normal, ratio, side):
    """len(DELTAS) rows of N_AZ rays that reach `point`, where the outward shading normal is `normal`, at the angle asin(ratio) +
    delta from it: side "entry" from outside (0.4 away), side "exit" from inside the medium (0.3 away)."""
    out = []
    t, b = _tangent_frame(normal)
    theta_c = np.arcsin(ratio)
    for delta in DELTAS:
        for k in range(N_AZ):
            phi = 2 * np.pi * (k + 0.25) / N_AZ
            th = theta_c + delta
            d = (-1.0 if side == "entry" else 1.0) * np.cos(th) * normal + np.sin(th) * (np.cos(phi) * t + np.sin(phi) * b)
            out.append(np.concatenate([point - (0.4 if side == "entry" else 0.3) * d, d]))
    return out


# where the critical rays are aimed: (mesh, material, point, outward face normal) for rays from outside and from inside the medium
_AIM = {
    "entry": [(BOX, M_OUTER, np.array([0.75, 0.5, 2.0]), np.array([0, 0, 1.0])),                 # (off the face's diagonal y = x + 0.5)
              (BOX, M_OUTER, np.array([2.0, 0.25, -0.5]), np.array([1.0, 0, 0])),
              (OCTA, M_INNER, OCTA_C + OCTA_R * np.array([0.3, 0.3, 0.4]), _unit([1.0, 1, 1])),
              (OCTA, M_INNER, OCTA_C + OCTA_R * np.array([-0.25, 0.5, 0.25]), _unit([-1.0, 1, 1]))],
    "exit": [(BOX, M_OUTER, np.array([1.5, 1.5, 2.0]), np.array([0, 0, 1.0])),                  # (off the faces' diagonals, too)
             (BOX, M_OUTER, np.array([2.0, -0.5, 1.5]), np.array([1.0, 0, 0])),
             (OCTA, M_INNER, OCTA_C + OCTA_R * np.array([0.3, 0.3, 0.4]), _unit([1.0, 1, 1])),
             (OCTA, M_INNER, OCTA_C + OCTA_R * np.array([-0.25, 0.5, 0.25]), _unit([-1.0, 1, 1]))],
}


def critical_groups(flat, side):
    """The (mesh, ratio) of every group of len(DELTAS) * N_AZ critical rays of `side`, in the order the rays are made.  A critical
    angle exists on entry for 0 < ior < 1 (asin(ior)) and on exit for 1 < ior (asin(1 / ior)); ior 1, 0 and negative have none
    (eta_r / eta_i is 1, 0 or +inf, or negative: refract_at's inequality never changes sides short of grazing)."""
    out = []
    for mesh, mat, _, _ in _AIM[side]:
        ior = float(flat.mat_ior[mat])
        if side == "entry" and 0 < ior < 1:
            out.append((mesh, ior))
        if side == "exit" and 1 < ior:
            out.append((mesh, 1.0 / ior))
    return out


def _critical_family(oacc, flat, side):
    rays = []
    for mesh, mat, point, fn in _AIM[side]:
        ior = float(flat.mat_ior[mat])
        ratio = ior if side == "entry" and 0 < ior < 1 else 1.0 / ior if side == "exit" and 1 < ior else None
        if ratio is not None:
            rays += _critical_rays(point, _shading_normal_at(oacc, flat, point, fn), ratio, side)
    return rays


def _leaving_candidates(flat, seed, n):
    """Rays aimed from close by at points near the vertices of the two glass meshes: where the mesh is smooth-shaded, the hit
    normal there leans far from the face normal, and a ray can meet the front of a face with 0 < dot(i, hn)."""
    rng = np.random.default_rng(seed)
    starts = np.concatenate([[0], np.cumsum(flat.mesh_nverts)[:-1]])
    out = []
    for mesh in (BOX, OCTA):
        v = flat.vertices[starts[mesh]:starts[mesh] + flat.mesh_nverts[mesh]].astype(np.float64)
        first = int(np.sum(flat.mesh_ntris[:mesh]))
        tris = flat.indices[first:first + flat.mesh_ntris[mesh]].astype(np.int64)
        for _ in range(n):
            t = tris[rng.integers(len(tris))]
            bary = rng.dirichlet((6.0, 1.0, 1.0))
            p = bary @ v[np.roll(t, rng.integers(3))]
            d = _unit(rng.normal(size=3))
            out.append(np.concatenate([p - 0.4 * d, d]))
    return np.array(out, np.float32)


def _stack(fam):
    rays, masks, at = [], {}, 0
    total = sum(len(v) for v in fam.values())
    for k, v in fam.items():
        masks[k] = np.zeros(total, bool)
        masks[k][at:at + len(v)] = True
        at += len(v)
        rays += list(v)
    return np.ascontiguousarray(np.array(rays, np.float64).reshape(-1, 6), np.float32), masks


_G = [(x, y) for x in (-1.5, -0.5, 0.25, 1.0, 1.75) for y in (-0.75, 0.25, 1.0, 1.75)]


def special_radiance_rays(ora, flat, oacc=None):
    """Rays whose first hit is found with back-face culling, as the reference's probe and a camera ray find theirs ->
    (rays float32 [n, 6], {family: bool[n]}).  Families:
      normal_outside   exactly along the inward normal of a box face, from outside: normalized(i + cos_i_n * n) normalises zero
      on_face          origins exactly on the box's z = 2 face, directions into the box, out of it and within the face
      into_inner       from between box and octahedron onto the octahedron: glass entered from inside glass as a first hit
      critical         from outside onto the glass whose ior lies in (0, 1), at the critical angle of entry asin(ior) + DELTAS
                       from the shading normal (critical_groups(flat, "entry"); none for the other iors)
      leaving          close-range rays whose closest hit is refractive with 0 < dot(i, n): the only way a culled first hit
                       leaves a medium, through a smooth mesh's leaning hit normals
    A culled first hit never meets a flat glass face from inside: those cases are unculled_radiance_rays."""
    oacc = oacc or ora.Accel(ora.Scene(flat), ora.ACCEL_KD_SIMD)
    fam = {}
    g = _G
    fam["normal_outside"] = ([[x, y, 3.0, 0, 0, -1.0] for x, y in g] + [[5.0, y, x, -1.0, 0, 0] for x, y in g]
                             + [[x, 6.0, y, 0, -1.0, 0] for x, y in g] + [[x, y, 3.25, 0, 0, -3.0] for x, y in g[:8]]
                             + [[x, y, -3.0, 0, 0, 0.7] for x, y in g[:8]])
    dirs = [(0.25, 0.125, -1.0), (0, 0, -1.0), (0.5, -0.25, 1.0), (0, 0, 1.0), (1.0, 0.5, 0.0), (-0.75, 0.25, -0.25)]
    fam["on_face"] = [[x, y, 2.0, *d] for x, y in g[::2] for d in dirs]
    rng = np.random.default_rng(41)
    o = OCTA_C + 1.6 * _unit(rng.normal(size=(48, 3)))                    # inside the box (its faces are 2 from the centre)
    fam["into_inner"] = np.concatenate([o, OCTA_C + rng.uniform(-0.3, 0.3, (48, 3)) - o], axis=1).tolist()
    fam["critical"] = _critical_family(oacc, flat, "entry")
    cand = _leaving_candidates(flat, 5, 3000)
    h, rest = oacc.intersect(cand, True), oacc.intersect_rest(cand, True)
    _, leaving, _ = refraction_case(flat, cand, h, rest)
    fam["leaving"] = cand[leaving][:128].tolist()
    return _stack(fam)


def unculled_radiance_rays(ora, flat, oacc=None):
    """Rays that start inside the glass and whose first hit is found WITHOUT culling (rtk_radiance_params.cull = 0), so that it
    meets a face from inside.  The reference's probe culls first hits, so these are compared with the oracle alone ->
    (rays float32 [n, 6], {family: bool[n]}).  Families:
      normal_inside    from between box and octahedron exactly along a box face's normal, outwards: normal incidence on exit
      inside_inner     origins inside the octahedron, directions at random
      critical_exit    from inside the glass whose ior is above 1 onto its own face, at the critical angle of the exit
                       asin(1 / ior) + DELTAS from the shading normal (critical_groups(flat, "exit"))"""
    oacc = oacc or ora.Accel(ora.Scene(flat), ora.ACCEL_KD_SIMD)
    fam = {}
    fam["normal_inside"] = ([[x, 2.25, 1.5, 0, 0, 1.0] for x in (-1.5, -0.5, 0.5, 1.5)] + [[1.75, y, 0.25, 1.0, 0, 0] for y in (-1.0, 0.0, 1.0, 2.0)]
                            + [[x, 2.25, 1.5, 0, 0, -1.0] for x in (-1.5, -0.5, 0.5, 1.5)] + [[x, 2.0, 1.75, 0, -1.0, 0] for x in (-1.5, -0.5, 0.5, 1.5)]
                            + [[x, 2.25, 1.5, 0, 0, 2.5] for x in (-1.25, 0.75)])
    rng = np.random.default_rng(99)
    o = OCTA_C + rng.uniform(-0.3, 0.3, (48, 3))
    fam["inside_inner"] = np.concatenate([o, rng.normal(size=(48, 3))], axis=1).tolist()
    fam["critical_exit"] = _critical_family(oacc, flat, "exit")
    return _stack(fam)


def view_batch(ora, flat):
    """one 32 x 32 view near the scene's camera"""
    return ViewBatch(ora, jittered_views(flat, 1, seed=12), 32, 32)


def radiance_rays(ora, flat, oacc=None):
    """-> (rays: the special rays, then the view batch; masks: the families and "view")"""
    special, masks = special_radiance_rays(ora, flat, oacc)
    view = view_batch(ora, flat).rays
    n = len(special) + len(view)
    masks = {k: np.concatenate([m, np.zeros(len(view), bool)]) for k, m in masks.items()}
    masks["view"] = np.arange(n) >= len(special)
    return np.ascontiguousarray(np.concatenate([special, view]), np.float32), masks


# ---------------------------------------------------------------- occlusion queries through stacked glass

def stacked_glass_queries():
    """-> (rays [n, 6], max_t [n], surfaces int[n]: glass surfaces on the line before the opaque quad at z = -4, or the floor).
    Lines along -z at heights that meet the lower quads: from in front of the box through the octahedron (4 surfaces) or beside it
    (2), from inside the box in front of the octahedron (3) or beside it (1), from behind the box (0); for every line max_t
    ends before the first surface, between each two, between the last and the quad, and behind the quad; directions of length
    1 and 2 (max_t is in units of the direction)."""
    rays, max_t, surf = [], [], []
    lines = [((0.25, 0.75), 5.0, [2.0, None, None, -2.0]), ((-0.5, 0.75), 5.0, [2.0, None, None, -2.0]),
             ((1.75, 0.5), 5.0, [2.0, -2.0]), ((-1.5, -1.0), 5.0, [2.0, -2.0]),
             ((0.25, 0.75), 1.75, [None, None, -2.0]), ((-0.25, 0.25), 1.9, [None, None, -2.0]),
             ((1.75, 0.5), 1.5, [-2.0]), ((-1.75, 1.5), 0.0, [-2.0]),
             ((0.5, 0.5), -2.5, []), ((2.25, 0.5), 5.0, [])]
    for (x, y), z0, zs in lines:
        # the octahedron's surface on this line: |x| + |y - cy| + |z| = r
        zo = OCTA_R - abs(x - OCTA_C[0]) - abs(y - OCTA_C[1])
        cross = [z if z is not None else None for z in zs]
        k = [i for i, z in enumerate(cross) if z is None]
        if k:
            assert zo > 0
            cross[k[0]], cross[k[1]] = zo, -zo
        cross = [z for z in cross if z < z0] + [-4.0]
        stops = [z0 - 0.5 * (z0 - cross[0])] + [0.5 * (a + b) for a, b in zip(cross[:-1], cross[1:])] + [-4.5, -40.0]
        for length in (1.0, 2.0):
            for stop in stops:
                rays.append([x, y, z0, 0, 0, -length])
                max_t.append((z0 - stop) / length)
                surf.append(len(cross) - 1)
    return np.array(rays, np.float32), np.array(max_t, np.float32), np.array(surf, np.int32)


# ---------------------------------------------------------------- the census: what the cases reach

def census(ora, flat, rays=None, oacc=None):
    """From the oracle's closest hits (culled) of `rays` (default: the camera rays of the 48 x 32 frame) -> counts:
    kind_<k> per material kind, tex_<k> per texture kind, refractive, tir_entry, tir_exit, refract_entry, refract_exit, and
    smooth_differs: hits on smooth refractive triangles whose hit normal and face normal differ in some bit."""
    oacc = oacc or ora.Accel(ora.Scene(flat), ora.ACCEL_KD_SIMD)
    if rays is None:
        rays = oacc.camera_rays(*SIZE).reshape(-1, 6)
    rays = np.ascontiguousarray(rays, np.float32)
    hits, rest = oacc.intersect(rays, True), oacc.intersect_rest(rays, True)
    hit = hits["mesh"] != MISS
    mat = flat.mesh_material[np.where(hit, hits["mesh"], 0)]
    out = {"rays": len(rays), "miss": int((~hit).sum())}
    for k in range(5):
        out[f"kind_{k}"] = int((hit & (flat.mat_kind[mat] == k)).sum())
    textured = hit & (flat.mat_kind[mat] == TEXTURE)
    for k in range(4):
        out[f"tex_{k}"] = int((textured & (flat.tex_kind[np.where(textured, flat.mat_texture[mat], 0)] == k)).sum())
    refractive, leaving, tir = refraction_case(flat, rays, hits, rest)
    out["refractive"] = int(refractive.sum())
    out["tir_entry"], out["tir_exit"] = int((tir & ~leaving).sum()), int((tir & leaving).sum())
    out["refract_entry"] = int((refractive & ~tir & ~leaving).sum())
    out["refract_exit"] = int((refractive & ~tir & leaving).sum())
    differs = (np.ascontiguousarray(hits["normal"]).view(np.uint32) != np.ascontiguousarray(rest["face_normal"]).view(np.uint32)).any(axis=1)
    out["smooth_differs"] = int((refractive & (flat.mat_smooth[mat] != 0) & differs).sum())
    return out
