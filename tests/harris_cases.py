"""The images and parameters of the orb_score 0 GPU parity tests (tests/test_gpu_orb_harris.py), shared with the CPU test that checks
on the oracle's output that every case exercises the mode (tests/test_harris_host.py)."""
import numpy as np

from stvo_amd import synth

# name: (cols, rows, nfeatures, nlevels, scale_factor, fast_th, seeds (one image each: the batch), make_image keywords)
CASES = {
    "kitti_1level_batch": (1241, 376, 1000, 1, 1.2, 20, (100, 101, 102), {}),                 # neither side a multiple of the 64 x 64 tile
    "kitti_2000_single": (1241, 376, 2000, 1, 1.2, 20, (100,), {}),                           # config_kitti.yaml's budget, B = 1
    "euroc_4levels_batch": (752, 480, 600, 4, 1.2, 20, (900, 901), dict(n_rects=400, n_discs=100)),
    "small_single": (640, 200, 300, 1, 1.2, 12, (307,), dict(n_rects=120, n_discs=30, noise=4.0)),
    "odd_size_3levels": (401, 299, 500, 3, 1.5, 9, (5,), dict(n_rects=300, n_discs=60)),
}


def images(name):
    cols, rows, _, _, _, _, seeds, kw = CASES[name]
    return np.stack([synth.make_image(s, cols=cols, rows=rows, **kw) for s in seeds])
