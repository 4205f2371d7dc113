"""What the tests of the textures and uvs of a live accel share (test_textures_abi.py, test_gpu_textures.py): the oracle's flat scene
with its texture table or its uvs replaced (dataclasses.replace, beside scene_state_checks.py), and the setters fed from such a
scene.  A texture here is a Tex: kind, the two colours, the parameter, and uint8 [h, w, 3] texels for a bitmap."""
import dataclasses

import numpy as np

ALBEDO, EDGES, CHECKER, BITMAP = range(4)


@dataclasses.dataclass
class Tex:
    kind: int
    a: tuple = (0.0, 0.0, 0.0)
    b: tuple = (0.0, 0.0, 0.0)
    param: float = 0.0
    pixels: np.ndarray = None


def textures_of(flat):
    """the texture table of a flat scene as a list of Tex"""
    out = []
    for i, kind in enumerate(flat.tex_kind if flat.tex_kind is not None else []):
        if kind == BITMAP:
            off, w, h = (int(x) for x in flat.tex_bitmap[i])
            out.append(Tex(BITMAP, pixels=flat.tex_pixels[off:off + w * h * 3].reshape(h, w, 3).copy()))
        else:
            out.append(Tex(int(kind), tuple(flat.tex_color_a[i]), tuple(flat.tex_color_b[i]), float(flat.tex_param[i])))
    return out


def with_textures(flat, texs):
    """`flat` with the texture table `texs`: what rtk_scene_create takes, bitmaps packed one behind the other"""
    n = len(texs)
    bitmap, pixels, off = np.zeros((n, 3), np.int32), [], 0
    for i, t in enumerate(texs):
        if t.kind == BITMAP:
            h, w, _ = t.pixels.shape
            bitmap[i] = (off, w, h)
            pixels.append(np.ascontiguousarray(t.pixels, np.uint8).reshape(-1))
            off += w * h * 3
    bmp = [t.kind == BITMAP for t in texs]
    return dataclasses.replace(
        flat, tex_kind=np.array([t.kind for t in texs], np.int32),
        tex_color_a=np.array([(0, 0, 0) if z else t.a for t, z in zip(texs, bmp)], np.float32).reshape(n, 3),
        tex_color_b=np.array([(0, 0, 0) if z else t.b for t, z in zip(texs, bmp)], np.float32).reshape(n, 3),
        tex_param=np.array([0 if z else t.param for t, z in zip(texs, bmp)], np.float32),
        tex_pixels=np.concatenate(pixels) if pixels else np.zeros(0, np.uint8), tex_bitmap=bitmap)


def dense_uvs(flat):
    """[n_vertices, 2]: the uvs of every vertex, zeros for the meshes without uvs (loader.hpp:199-207)"""
    out = np.zeros((int(flat.mesh_nverts.sum()), 2), np.float32)
    has = flat.mesh_has_uvs if flat.mesh_has_uvs is not None else np.zeros(len(flat.mesh_nverts), np.int32)
    v = u = 0
    for nv, h in zip(flat.mesh_nverts, has):
        if h:
            out[v:v + nv] = flat.uvs[u:u + nv]
            u += nv
        v += nv
    return out


def with_uvs(flat, uv):
    """`flat` in which every mesh carries the rows of the dense [n_vertices, 2] array `uv`"""
    uv = np.ascontiguousarray(uv, np.float32)
    assert uv.shape == (int(flat.mesh_nverts.sum()), 2)
    return dataclasses.replace(flat, uvs=uv, mesh_has_uvs=np.ones(len(flat.mesh_nverts), np.int32))


def set_textures(acc, flat):
    t = textures_of(flat)
    acc.set_textures([x.kind for x in t], [x.a for x in t] or None, [x.b for x in t] or None, [x.param for x in t] or None,
                     [x.pixels for x in t])


def check_table(acc, flat):
    """textures() and texture_pixels() of `acc` are flat's table: colours and parameters by their bits, texels byte for byte"""
    want, got = textures_of(flat), acc.textures()
    assert got["kind"].tolist() == [t.kind for t in want]
    for i, t in enumerate(want):
        px = acc.texture_pixels(i)
        if t.kind == BITMAP:
            assert (got["width"][i], got["height"][i]) == (t.pixels.shape[1], t.pixels.shape[0]), i
            assert px.shape == t.pixels.shape and px.tobytes() == t.pixels.tobytes(), i
            assert not got["color_a"][i].any() and not got["color_b"][i].any() and got["param"][i] == 0, i
        else:
            assert px.size == 0 and (got["width"][i], got["height"][i]) == (0, 0), i
            assert got["color_a"][i].tobytes() == np.array(t.a, np.float32).tobytes(), i
            assert got["color_b"][i].tobytes() == np.array(t.b, np.float32).tobytes(), i
            assert got["param"][i].tobytes() == np.float32(t.param).tobytes(), i
