#!/usr/bin/env python3
"""Randomised parity of the ORB front-end's two rankings (orb_score 0 HARRIS, 1 FAST) against the oracle and the numpy Harris statement,
through the C-ABI: random image sizes, content (scenes, noise, checkerboards, saturated blocks, dot lattices with masses of equal
responses, flat), FAST thresholds, budgets, capacities, pyramid levels and batch sizes, and the switch between the rankings on one
detector.  Test infrastructure.  Run on a GPU box from the repo root:
    python tests/fuzz_orb_harris.py [--seconds 120] [--seed 1]
Prints one line per mismatch with everything needed to replay it; exit code 1 if any."""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "stvo-pl_amd", "python")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import np_harris
import oracle_lib
from stvo_amd import capi, synth

KEYS = ("kp", "response", "angle", "desc", "octave")


def make_image(rng, cols, rows):
    kind = rng.integers(0, 8)
    seed = int(rng.integers(1, 1 << 30))
    yy, xx = np.mgrid[0:rows, 0:cols]
    if kind <= 2:
        img = synth.make_image(seed, cols, rows, n_rects=int(rng.integers(5, 400)), n_discs=int(rng.integers(0, 100)), noise=float(rng.uniform(0, 6)))
    elif kind == 3:
        img = rng.integers(0, 256, (rows, cols))
    elif kind == 4:
        p = int(rng.integers(2, 40))
        img = (((xx // p) + (yy // p)) % 2) * rng.uniform(60, 255) + rng.normal(0, rng.uniform(0, 2), (rows, cols))
    elif kind == 5:
        q = int(rng.integers(4, 17))
        img = np.kron(rng.integers(0, 2, ((rows + q - 1) // q, (cols + q - 1) // q)) * 255, np.ones((q, q)))[:rows, :cols]
    elif kind == 6:
        p = int(rng.integers(6, 12))
        img = np.where((yy % p == 0) & (xx % p == 0), 200, 40)
    else:
        img = np.full((rows, cols), int(rng.integers(0, 256)))
    return np.clip(np.rint(np.asarray(img, float)), 0, 255).astype(np.uint8)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=120.0)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--cases", type=int, default=0, help="stop after this many cases (0: run for --seconds)")
    args = ap.parse_args(argv)
    orc = oracle_lib.load()
    ctx = capi.Context(device_id=0, max_rows=2048, max_batch=8)
    t_end = time.time() + args.seconds
    case, bad, ran, bites = 0, 0, 0, 0
    try:
        while time.time() < t_end and (args.cases == 0 or case < args.cases):
            case += 1
            rng = np.random.default_rng([args.seed, case])
            cols, rows = int(rng.integers(64, 900)), int(rng.integers(64, 500))
            if rng.integers(0, 6) == 0:
                cols, rows = [(1241, 376), (1226, 370), (752, 480)][int(rng.integers(0, 3))]
            B = int(rng.integers(1, 5))
            imgs = np.stack([make_image(rng, cols, rows) for _ in range(B)])
            nlev = int(rng.integers(1, 5)); th = int(rng.integers(5, 50)); nf = int(rng.choice([20, 50, 300, 1000, 2000]))
            cap = int(rng.choice([256, 1024, 4096])); sf = float(rng.choice([1.2, 1.5, 2.0]))
            order = [int(v) for v in rng.integers(0, 2, 3)]   # the score types of three successive calls on one detector
            tag = f"seed {args.seed} case {case} {cols}x{rows} B {B} nf {nf} th {th} levels {nlev} x {sf} cap {cap} scores {order}"
            try:
                orb = capi.Orb(ctx, B, cols, rows, max_keypoints=cap, nfeatures=nf, fast_threshold=th, nlevels=nlev, scale_factor=sf, score=order[0])
            except capi.StvoError:
                continue   # (an image smaller than the border: refused, fine)
            try:
                refs = {}
                for step, score in enumerate(order):
                    if step:
                        orb.set_score_type(score)
                    out = orb.detect(imgs)
                    for b in range(B):
                        if (score, b) not in refs:
                            info = []
                            refs[score, b] = np_harris.detect_levels(orc, imgs[b], nf, nlev, sf, th, cap=cap, info=info, score=score)
                            bites += any(lv["n_cand"] > lv["n"] for lv in info)
                        ref = refs[score, b]
                        ok = all(same_bits(out[b][k], ref[k]) for k in KEYS) and out[b]["n_total"] == ref["n_total"]
                        ran += 1
                        if not ok:
                            bad += 1
                            print(f"MISMATCH {tag} step {step} score {score} image {b}: got {len(out[b]['kp'])} / n_total {out[b]['n_total']}, "
                                  f"expected {len(ref['kp'])} / {ref['n_total']}", flush=True)
            finally:
                orb.close()
    finally:
        ctx.close()
    print(f"fuzz_orb_harris: {case} cases, {ran} detections compared, {bites} with a Harris cut that bites, {bad} mismatches", flush=True)
    return 1 if bad or ran == 0 else 0


if __name__ == "__main__":
    sys.exit(main())
