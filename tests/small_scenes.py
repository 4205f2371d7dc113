"""Small scenes that more than one test file builds."""
import numpy as np


def two_quad_scene(ora):
    """A floor, a mirror standing on it and one light, 16x16: the scene of regions_check.cpp (and views_check.cpp)."""
    return ora.FlatScene(
        mesh_material=np.array([0, 1], np.int32), mesh_nverts=np.array([4, 4], np.int32), mesh_ntris=np.array([2, 2], np.int32),
        vertices=np.array([[-3, -1, 0], [3, -1, 0], [3, -1, -6], [-3, -1, -6],
                           [-1.5, -1, -4], [1.5, -1, -4], [1.5, 1, -4], [-1.5, 1, -4]], np.float32),
        indices=np.array([[0, 1, 2], [0, 2, 3], [0, 1, 2], [0, 2, 3]], np.uint32),
        mat_kind=np.array([ora.MAT_DIFFUSE, ora.MAT_REFLECTIVE], np.int32),
        mat_albedo=np.array([[0.9, 0.6, 0.3], [1, 1, 1]], np.float32), mat_ior=np.array([1.0, 1.0], np.float32),
        mat_smooth=np.zeros(2, np.int32), light_pos=np.array([[0, 3, -2]], np.float32),
        light_intensity=np.array([150], np.float32), cam_pos=np.zeros(3, np.float32),
        cam_mat=np.eye(3, dtype=np.float32).reshape(-1), background=np.array([0.25, 0.5, 0.75], np.float32),
        width=16, height=16, bucket_size=64)
