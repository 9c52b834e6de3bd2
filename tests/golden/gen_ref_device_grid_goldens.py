"""Generates tests/golden/ref_device_grid_goldens.npz from the REFERENCE's own grid + Bresenham code, for the GPU test
that checks the DEVICE-side grid builder / rasteriser / window gather (csrc/stereo_assoc_kernels.hip point_cells_kernel,
line_cells_kernel; csrc/grid_kernels.hip grid_cover) directly against reference outputs — not through the oracle.

Runs only in the development container: needs oracle/_ref/libstvo_ref.so, which oracle/Makefile builds from
/root/reference/src/{gridStructure,lineIterator}.cpp (compiled unmodified, by path).  The fixture holds data only:
seeded pixel-space inputs for the three KITTI calibrations of BASELINE configs[4] (1241x376, 1242x375, 1226x370) and the
reference's outputs:
  * per grid cell, the ids GridStructure holds after `grid.at(x, y).push_back(id)` for every right key-point
    (src/stereoFrame.cpp:135-139) resp. every LineIterator cell of every right key-line (:325-338) — obtained as
    GridStructure::get with a zero window on each of the 64 x 48 cells;
  * per right key-line, the getLineCoords cell list (src/gridStructure.cpp:33-41, src/lineIterator.cpp:34-77);
  * per left feature, GridStructure::get with the stereo window (matching_s_ws = 10, :141-143 / :340-342); for lines
    the union of the two end-point windows (src/matching.cpp:213-215 inserts both into one unordered_set).
The only arithmetic restated here (numpy) is the cell of a pixel: (int)(float * double) with inv = 64 / cols, 48 / rows
(src/stereoFrame.cpp:47-48,132,138,321-322,335).
    python tests/golden/gen_ref_device_grid_goldens.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "stvo-pl_amd", "python"))
import oracle_lib  # noqa: E402

SIZES = [(1241, 376), (1242, 375), (1226, 370)]  # kitti00-02.yaml, kitti03.yaml, kitti04-10.yaml
WS = 10


def cells_of(xy_f32, cols, rows):
    inv = np.array([64.0 / cols, 48.0 / rows])
    return (xy_f32.astype(np.float64) * inv).astype(np.int32)  # C truncation toward zero


def grid_get(ref, ent, owner, q, w, n_owner):
    nq = len(q)
    off = np.empty(nq + 1, np.int32)
    res = np.empty(max(nq * min(n_owner, 512), 16), np.int32)
    tot = ref.ref_grid_get(np.ascontiguousarray(ent, np.int32).reshape(-1), owner.ctypes.data, len(ent), 48, 64,
                           np.ascontiguousarray(q, np.int32).reshape(-1), nq, w[0], w[1], w[2], w[3], off, res, len(res))
    assert tot <= len(res), (tot, len(res))
    return off.copy(), res[:tot].copy()


def main():
    ref = oracle_lib.load_ref()
    assert ref is not None, "build oracle/_ref first (make -C oracle)"
    rng = np.random.default_rng(20260927)
    all_cells = np.stack(np.meshgrid(np.arange(64), np.arange(48)), -1).reshape(-1, 2).astype(np.int32)  # c = y * 64 + x
    out = {"sizes": np.array(SIZES, np.int32), "ws": np.int32(WS)}
    buf = np.empty((1024, 2), np.int32)
    for c, (cols, rows) in enumerate(SIZES):
        n, m = 700 + 100 * c, 90 + 10 * c
        # ---- key-points: mostly inside the image, a few on / beyond its borders (sink cells), a few on exact cell borders
        kp = [np.stack([rng.uniform(0, cols, n), rng.uniform(0, rows, n)], 1) for _ in range(2)]
        for k in kp:
            k[:6] = [[-3.0, 10.0], [cols + 2.5, 20.0], [50.0, -1.5], [60.0, rows + 4.0], [cols - 1e-3, rows - 1e-3], [0.0, 0.0]]
            j = rng.integers(0, 64, 12)
            k[6:18, 0] = j * cols / 64.0  # float32 rounding decides the side of the border
        kp_l, kp_r = (k.astype(np.float32) for k in kp)
        ids = np.arange(n, dtype=np.int32)
        ent_r = cells_of(kp_r, cols, rows)
        out[f"kp_l_{c}"], out[f"kp_r_{c}"] = kp_l, kp_r
        out[f"pcell_off_{c}"], out[f"pcell_out_{c}"] = grid_get(ref, ent_r, ids, all_cells, (0, 0, 0, 0), n)
        q = cells_of(kp_l, cols, rows)
        out[f"pcells_l_{c}"] = q
        out[f"pcand_off_{c}"], out[f"pcand_out_{c}"] = grid_get(ref, ent_r, ids, q, (WS, 0, 0, 0), n)
        # ---- key-lines
        def lines():
            s = np.stack([rng.uniform(5, cols - 5, m), rng.uniform(5, rows - 5, m)], 1)
            L = rng.uniform(3, 350, m); a = rng.uniform(0, 2 * np.pi, m)
            e = s + np.stack([L * np.cos(a), L * np.sin(a)], 1)
            e[:, 0] = np.clip(e[:, 0], -8, cols + 8); e[:, 1] = np.clip(e[:, 1], -8, rows + 8)  # some end points leave the image
            kl = np.concatenate([s, e], 1)
            kl[0] = [100.0, 50.0, 100.0, 300.0]; kl[1] = [40.0, 200.0, 900.0, 200.0]; kl[2] = [300.5, 100.25, 301.0, 100.5]
            return kl.astype(np.float32)
        kl_l, kl_r = lines(), lines()
        inv_w, inv_h = 64.0 / cols, 48.0 / rows
        ent, owner = [], []
        for j in range(m):
            x1, y1, x2, y2 = (float(kl_r[j, 0]) * inv_w, float(kl_r[j, 1]) * inv_h, float(kl_r[j, 2]) * inv_w, float(kl_r[j, 3]) * inv_h)
            k = ref.ref_line_coords(x1, y1, x2, y2, buf.reshape(-1), 1024)
            ent.append(buf[:k].copy()); owner.append(np.full(k, j, np.int32))
        out[f"lline_off_{c}"] = np.cumsum([0] + [len(e) for e in ent]).astype(np.int32)  # LineIterator cells of every right line
        ent = np.concatenate(ent); owner = np.concatenate(owner)
        out[f"lline_cells_{c}"] = ent
        out[f"kl_l_{c}"], out[f"kl_r_{c}"] = kl_l, kl_r
        out[f"lcell_off_{c}"], out[f"lcell_out_{c}"] = grid_get(ref, ent, owner, all_cells, (0, 0, 0, 0), m)
        ql = np.concatenate([cells_of(kl_l[:, 0:2], cols, rows), cells_of(kl_l[:, 2:4], cols, rows)], 1)
        out[f"lcells_l_{c}"] = ql
        o1, r1 = grid_get(ref, ent, owner, ql[:, 0:2], (WS, 0, 0, 0), m)
        o2, r2 = grid_get(ref, ent, owner, ql[:, 2:4], (WS, 0, 0, 0), m)
        off, res = [0], []
        for i in range(m):
            u = np.union1d(r1[o1[i]:o1[i + 1]], r2[o2[i]:o2[i + 1]]).astype(np.int32)
            res.append(u); off.append(off[-1] + len(u))
        out[f"lcand_off_{c}"], out[f"lcand_out_{c}"] = np.array(off, np.int32), np.concatenate(res)
    np.savez_compressed(os.path.join(HERE, "ref_device_grid_goldens.npz"), **out)
    print("wrote ref_device_grid_goldens.npz:", {k: v.shape for k, v in out.items() if k.endswith("_0")})


if __name__ == "__main__":
    main()
