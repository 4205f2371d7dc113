"""Child process of tests/test_gpu_denoise.py: RTK_DENOISE_LDS_MAX_STEP is read once per process, so every setting of it gets a
fresh one.  usage: python denoise_child.py OUT.npy -- filters the two synthetic 130x70 images of denoise_model.knob_case() with
whatever the environment says and saves the result."""
import importlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import denoise_model as dm  # noqa: E402


def main(out_path):
    rtk = importlib.import_module("simd-raytracer_amd")
    planes, params = dm.knob_case()
    out = rtk.denoise(planes["rgb"], planes["normal"], planes["position"], planes["depth"], planes["noise"], planes["albedo"],
                      rtk.DenoiseConfig(**params))
    np.save(out_path, out)


if __name__ == "__main__":
    main(sys.argv[1])
