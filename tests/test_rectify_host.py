"""Stereo rectification on the host (stvo_rectify_compute, no device): R1, R2, P1, P2 and the pipeline camera against the numpy
second statement (tests/np_rectify.py), the CV_16SC2 maps bit for bit against numpy maps built from the library's own R / P, the
geometry of the result (independent of any OpenCV version), the reference's quirks, the dataset-file readers (Python and the C++
mirror PinholeStereoCamera(params_file))."""
import copy
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import np_rectify as nr
from stvo_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = os.path.join(ROOT, "tests", "golden", "dataset_params")
FILES = ["euroc_params.yaml", "perceptin_params.yaml", "kitti00-02.yaml"]


def calib_of(name):
    return capi.read_dataset_params(os.path.join(PARAMS, name))


def kitti_distorted():
    c = calib_of("kitti00-02.yaml")
    c.d[:] = [-0.17, 0.021, 0.0004, -0.0003]
    c.fy = 722.5  # != fx: form A puts fx on both diagonal entries of P
    return c


def fisheye_variant():
    c = calib_of("euroc_params.yaml")
    c.form = capi.RECT_FORM_FISHEYE
    c.Dl[:4] = [-0.0153, 0.0052, -0.0021, 0.0003]
    c.Dr[:4] = [-0.0149, 0.0047, -0.0018, 0.0002]
    return c


def random_calib(rng, small=False):
    c = capi.RectCalib()
    c.form = capi.RECT_FORM_RADTAN
    if small:
        c.width, c.height = int(rng.integers(96, 260)), int(rng.integers(64, 200))
    else:
        c.width, c.height = int(rng.integers(320, 1400)), int(rng.integers(240, 1000))
    for K in (c.Kl, c.Kr):
        f = rng.uniform(0.6, 1.3) * c.width
        K[:] = [f * rng.uniform(0.99, 1.01), f * rng.uniform(0.99, 1.01), c.width / 2 + rng.uniform(-25, 25), c.height / 2 + rng.uniform(-25, 25)]
    nd = int(rng.choice([4, 5, 8]))
    c.n_dist = nd
    for D in (c.Dl, c.Dr):
        vals = [rng.uniform(-0.4, 0.05), rng.uniform(-0.05, 0.15), rng.uniform(-1e-3, 1e-3), rng.uniform(-1e-3, 1e-3)]
        if nd >= 5:
            vals.append(rng.uniform(-0.02, 0.02))
        if nd == 8:
            vals += [rng.uniform(-0.01, 0.01) for _ in range(3)]
        D[:nd] = vals
    r = rng.normal(size=3) * math.radians(rng.uniform(0.05, 2.0)) / math.sqrt(3)
    c.R[:] = np.array(nr.rodrigues_v2m(list(r))).reshape(-1)
    b = rng.uniform(0.04, 0.6)
    c.t[:] = [-b * rng.choice([1, 1, 1, -1]), rng.uniform(-0.02, 0.02) * b, rng.uniform(-0.02, 0.02) * b]
    c.b = b
    return c


def rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300)


def check_camera(c, cam):
    ref = nr.rectify_calib(c)
    for k in ("R1", "R2", "P1", "P2"):
        assert rel(cam[k], ref[k]) <= 1e-10, k
    for k in ("fx", "fy", "cx", "cy", "b"):
        assert abs(cam["cam"][k] - ref["cam"][k]) <= 1e-10 * abs(ref["cam"][k]), k
    assert cam["dist"] == ref["dist"]


# ---- against the second statement ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", FILES)
def test_shipped_files_match_numpy(name):
    c = calib_of(name)
    cam, m1, m2 = capi.rectify_compute(c)
    check_camera(c, cam)
    e1, e2 = nr.maps_from_camera(c, cam)
    assert np.array_equal(m1, e1) and np.array_equal(m2, e2)


def test_kitti_style_with_distortion_matches_numpy():
    c = kitti_distorted()
    cam, m1, m2 = capi.rectify_compute(c)
    check_camera(c, cam)
    assert cam["dist"] == 1
    e1, e2 = nr.maps_from_camera(c, cam)
    assert np.array_equal(m1, e1) and np.array_equal(m2, e2)
    assert np.array_equal(m1[0], m1[1]) and np.array_equal(m2[0], m2[1])  # both images use the left map


def test_fisheye_variant_matches_numpy():
    c = fisheye_variant()
    cam, m1, m2 = capi.rectify_compute(c)
    check_camera(c, cam)
    # the rectification is the rad-tan one, fed the fisheye coefficients: the same R / P as a rad-tan calibration with them
    c_rt = copy.copy(c)
    c_rt.form = capi.RECT_FORM_RADTAN
    cam_rt = capi.rectify_compute(c_rt, maps=False)
    for k in ("R1", "R2", "P1", "P2"):
        assert np.array_equal(cam[k], cam_rt[k])
    e1, e2 = nr.maps_from_camera(c, cam)
    diff = (m1 != e1).any(axis=-1) | (m2 != e2)
    if diff.any():  # only where u * 32 or v * 32 is within 1e-6 of a half-integer (library atan may differ by an ulp)
        K = [[nr.f32(v) for v in c.Kl[:4]], [nr.f32(v) for v in c.Kr[:4]]]
        for s, i, j in zip(*np.nonzero(diff)):
            u, v = _fisheye_uv(K[s], list((c.Dr if s else c.Dl)[:4]), cam["R2" if s else "R1"], cam["P2" if s else "P1"], c.width, i, j)
            near = [abs(abs(q * 32 - math.floor(q * 32)) - 0.5) < 1e-6 for q in (u, v)]
            assert any(near), (s, i, j, u, v)
    assert diff.mean() < 1e-4


def _fisheye_uv(K, D, R, P, w, i, j):
    iR = nr._ir(P, R)
    _x, _y, _w = i * iR[0][1] + iR[0][2], i * iR[1][1] + iR[1][2], i * iR[2][1] + iR[2][2]
    for _ in range(j):
        _x += iR[0][0]; _y += iR[1][0]; _w += iR[2][0]
    x, y = _x / _w, _y / _w
    r = math.sqrt(x * x + y * y)
    th = math.atan(r)
    t2 = th * th
    td = th * (1 + D[0] * t2 + D[1] * t2 * t2 + D[2] * t2 * t2 * t2 + D[3] * t2 * t2 * t2 * t2)
    sc = 1.0 if r == 0 else td / r
    return K[0] * x * sc + K[2], K[1] * y * sc + K[3]


def test_random_calibrations_match_numpy():
    rng = np.random.default_rng(20261016)
    for trial in range(200):
        with_maps = trial % 10 == 0
        c = random_calib(rng, small=with_maps)
        if with_maps:
            cam, m1, m2 = capi.rectify_compute(c)
            e1, e2 = nr.maps_from_camera(c, cam)
            assert np.array_equal(m1, e1) and np.array_equal(m2, e2), trial
        else:
            cam = capi.rectify_compute(c, maps=False)
        check_camera(c, cam)


# ---- geometry ------------------------------------------------------------------------------------------------------------------

def _distort(K, D, x, y):
    k = nr.dist12(D)
    r2 = x * x + y * y
    kr = (1 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2) / (1 + ((k[7] * r2 + k[6]) * r2 + k[5]) * r2)
    xd = x * kr + 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x)
    yd = y * kr + k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y
    return K[0] * xd + K[2], K[1] * yd + K[3]


def _undistort(K, D, u, v, iters=200):
    k = nr.dist12(D)
    x0, y0 = (u - K[2]) / K[0], (v - K[3]) / K[1]
    x, y = x0.copy(), y0.copy()
    for _ in range(iters):
        r2 = x * x + y * y
        icd = (1 + ((k[7] * r2 + k[6]) * r2 + k[5]) * r2) / (1 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2)
        x = (x0 - 2 * k[2] * x * y - k[3] * (r2 + 2 * x * x)) * icd
        y = (y0 - k[2] * (r2 + 2 * y * y) - 2 * k[3] * x * y) * icd
    return x, y


@pytest.mark.parametrize("case", ["euroc", "perceptin", "random"])
def test_rectified_rows_agree_and_disparity_is_fb_over_z(case):
    rng = np.random.default_rng(7)
    cals = {"euroc": [calib_of("euroc_params.yaml")], "perceptin": [calib_of("perceptin_params.yaml")],
            "random": [random_calib(rng) for _ in range(10)]}[case]
    for c in cals:
        cam = capi.rectify_compute(c, maps=False)
        R1, R2, P1, P2 = cam["R1"], cam["R2"], cam["P1"], cam["P2"]
        for M in (R1, R2):
            assert np.abs(M @ M.T - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(M) - 1) < 1e-12
        K1 = [nr.f32(v) for v in c.Kl[:4]]
        K2 = [nr.f32(v) for v in c.Kr[:4]]
        R, t = np.array(c.R[:]).reshape(3, 3), np.array(c.t[:])
        n = 400
        X = np.stack([rng.uniform(-1.5, 1.5, n), rng.uniform(-1.0, 1.0, n), rng.uniform(3.0, 25.0, n)], axis=1) * np.array([1, 1, 1])
        X[:, :2] *= X[:, 2:3] * 0.35  # inside a ~70 degree frustum
        Xr = X @ R.T + t
        ul, vl = _distort(K1, c.Dl[:c.n_dist], X[:, 0] / X[:, 2], X[:, 1] / X[:, 2])
        ur, vr = _distort(K2, c.Dr[:c.n_dist], Xr[:, 0] / Xr[:, 2], Xr[:, 1] / Xr[:, 2])
        keep = (ul > 0) & (ul < c.width) & (vl > 0) & (vl < c.height) & (ur > 0) & (ur < c.width) & (vr > 0) & (vr < c.height)
        assert keep.sum() > 50
        rect = []
        for (u, v, K, D, Rk, P) in ((ul, vl, K1, c.Dl[:c.n_dist], R1, P1), (ur, vr, K2, c.Dr[:c.n_dist], R2, P2)):
            x, y = _undistort(K, D, u[keep], v[keep])
            q = np.stack([x, y, np.ones_like(x)], axis=1) @ (P[:, :3] @ Rk).T
            rect.append((q[:, 0] / q[:, 2], q[:, 1] / q[:, 2]))
        (xl, yl), (xr, yr) = rect
        assert np.abs(yl - yr).max() < 1e-6
        Z = (X[keep] @ R1.T)[:, 2]
        disp = P1[0, 0] * np.linalg.norm(t) / Z  # |disparity| = fc |t| / Z; its sign is the side the right camera sits on
        assert np.abs(np.abs(xl - xr) - disp).max() < 1e-6
        assert np.all(np.sign(xl - xr) == -np.sign(P2[0, 3]))
        assert abs(abs(P2[0, 3]) - P1[0, 0] * np.linalg.norm(t)) < 1e-9 * P1[0, 0]


@pytest.mark.parametrize("name", ["euroc_params.yaml", "perceptin_params.yaml"])
def test_alpha_zero_maps_stay_on_the_source(name):
    """alpha = 0 keeps only valid pixels: every map entry lies on the source image ([0, cols] x [0, rows]: the scale uses the
    `width` terms) and the tightest border is within a pixel."""
    c = calib_of(name)
    _, m1, m2 = capi.rectify_compute(c)
    X, Y = nr.map_coords(m1, m2)
    margin = min(X.min(), Y.min(), c.width - X.max(), c.height - Y.max())
    assert margin >= 0.0
    assert margin < 1.0


# ---- quirks of the reference's constructor -----------------------------------------------------------------------------------

def test_intrinsics_are_rounded_to_float_first():
    c = calib_of("euroc_params.yaml")
    c2 = copy.copy(c)
    c2.Kl[:] = [nr.f32(v) for v in c.Kl[:4]]
    c2.Kr[:] = [nr.f32(v) for v in c.Kr[:4]]
    a, b = capi.rectify_compute(c), capi.rectify_compute(c2)
    for k in ("R1", "R2", "P1", "P2"):
        assert np.array_equal(a[0][k], b[0][k])
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    # a difference below float resolution does not move anything; one above it does
    c3 = copy.copy(c)
    c3.Kl[0] = c.Kl[0] + 1e-6
    assert np.array_equal(capi.rectify_compute(c3, maps=False)["P1"], a[0]["P1"])
    c3.Kl[1] = c.Kl[1] + 1e-3
    assert not np.array_equal(capi.rectify_compute(c3, maps=False)["P1"], a[0]["P1"])


def test_pipeline_camera_is_p1_and_baseline_is_cam_bl():
    c = calib_of("euroc_params.yaml")
    cam = capi.rectify_compute(c, maps=False)
    P1 = cam["P1"]
    assert (cam["cam"]["fx"], cam["cam"]["fy"], cam["cam"]["cx"], cam["cam"]["cy"]) == (P1[0, 0], P1[1, 1], P1[0, 2], P1[1, 2])
    assert cam["cam"]["b"] == 0.110077842
    assert cam["cam"]["b"] != np.linalg.norm(np.array(c.t[:]))
    c2 = copy.copy(c)
    c2.t[:] = [v * 2 for v in c.t[:]]
    cam2 = capi.rectify_compute(c2, maps=False)
    assert cam2["cam"]["b"] == c.b and cam2["P1"][0, 0] == P1[0, 0]


def test_form_a_repeats_fx_and_keeps_intrinsics():
    c = kitti_distorted()
    cam = capi.rectify_compute(c, maps=False)
    assert cam["P1"][1, 1] == nr.f32(c.fx) and cam["P1"][1, 1] != nr.f32(c.fy)
    assert cam["cam"]["fy"] == c.fy and cam["cam"]["fx"] == c.fx and cam["cam"]["cx"] == c.cx  # as read, not float-rounded
    assert np.array_equal(cam["R1"], np.eye(3)) and np.array_equal(cam["P1"], cam["P2"])


def test_dist_is_false_when_d0_is_zero():
    c = kitti_distorted()
    c.d[0] = 0.0  # d1..d3 non-zero: still no rectification (dist = d0 != 0)
    assert capi.rectify_compute(c, maps=False)["dist"] == 0
    assert capi.rectify_compute(calib_of("kitti00-02.yaml"), maps=False)["dist"] == 0


def test_rl_rr_are_ignored(tmp_path):
    src = open(os.path.join(PARAMS, "euroc_params.yaml")).read()
    p = tmp_path / "e.yaml"
    p.write_text(src.replace("Rl: [0.9999663475300330", "Rl: [0.5").replace("Rr: [0.9999633526194376", "Rr: [0.25"))
    a = capi.rectify_compute(capi.read_dataset_params(str(p)), maps=False)
    b = capi.rectify_compute(calib_of("euroc_params.yaml"), maps=False)
    for k in ("R1", "R2", "P1", "P2"):
        assert np.array_equal(a[k], b[k])


def test_reader_forms_and_multiline_lists():
    e = calib_of("euroc_params.yaml")
    assert e.form == capi.RECT_FORM_RADTAN and e.n_dist == 4 and e.width == 752 and e.height == 480
    assert e.R[3] == -2.31713572e-03 and e.R[8] == 9.99900663e-01 and e.t[2] == -0.0008537  # R spans three lines
    assert calib_of("kitti00-02.yaml").form == capi.RECT_FORM_KITTI
    p = capi.parse_dataset_yaml("cam0:\n  Kl: [1, 2,\n   3, 4]  # c\n  dtype: equidistant\n  cam_bl: 0.5\nx: 3\n")
    assert p == {"cam0": {"Kl": [1.0, 2.0, 3.0, 4.0], "dtype": "equidistant", "cam_bl": 0.5}, "x": 3.0}


def test_bad_calibrations_are_refused():
    c = calib_of("euroc_params.yaml")
    c.n_dist = 6
    with pytest.raises(capi.StvoError):
        capi.rectify_compute(c, maps=False)
    c = fisheye_variant()
    c.n_dist = 5
    with pytest.raises(capi.StvoError):
        capi.rectify_compute(c, maps=False)


# ---- the C++ mirror ------------------------------------------------------------------------------------------------------------

DRIVER = r"""
#include <cstdio>
#include "pinholeStereoCamera.h"
int main(int argc, char** argv) {
    for (int i = 1; i < argc; ++i) {
        StVO::PinholeStereoCamera cam{std::string(argv[i])};
        const stvo_rect_camera& r = cam.getRectification();
        std::printf("%d %d %d %.17g %.17g %.17g %.17g %.17g", cam.getWidth(), cam.getHeight(), (int)cam.getDist(), cam.getFx(),
                    cam.getFy(), cam.getCx(), cam.getCy(), cam.getB());
        for (int k = 0; k < 12; ++k) std::printf(" %.17g", r.P1[k]);
        for (int k = 0; k < 12; ++k) std::printf(" %.17g", r.P2[k]);
        for (int k = 0; k < 9; ++k) std::printf(" %.17g", r.R1[k]);
        std::printf("\n");
    }
    return 0;
}
"""


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_cpp_camera_from_file_matches_capi(tmp_path):
    lib = os.path.join(ROOT, "stvo-pl_amd")
    assert os.path.exists(os.path.join(lib, "libstvo_host.so")), "build first (python __graft_entry__.py)"
    src = tmp_path / "drv.cpp"
    src.write_text(DRIVER)
    exe = str(tmp_path / "drv")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(lib, "host"), str(src), "-o", exe, "-L", lib, "-lstvo_host",
                           "-lstvo_hip", "-Wl,-rpath," + lib])
    p = str(tmp_path / "fish.yaml")
    with open(p, "w") as f:  # the fisheye form: a dtype key
        f.write(open(os.path.join(PARAMS, "euroc_params.yaml")).read().replace("cam_bl:", "dtype: equidistant\n  cam_bl:"))
    paths = [os.path.join(PARAMS, n) for n in FILES] + [p]
    out = subprocess.run([exe] + paths, capture_output=True, text=True, timeout=120, check=True).stdout.strip().splitlines()
    assert len(out) == len(paths)
    for path, line in zip(paths, out):
        v = line.split()
        c = capi.read_dataset_params(path)
        cam = capi.rectify_compute(c, maps=False)
        assert (int(v[0]), int(v[1]), int(v[2])) == (c.width, c.height, cam["dist"])
        got = [float(x) for x in v[3:]]
        exp = ([cam["cam"][k] for k in ("fx", "fy", "cx", "cy", "b")] + list(cam["P1"].reshape(-1)) + list(cam["P2"].reshape(-1)) +
               list(cam["R1"].reshape(-1)))
        assert got == exp, path
