#!/usr/bin/env python3
"""Randomised parity of the ORB front-end under every descriptor setting (orb_wta_k 2 / 3 / 4, orb_patch_size 2 .. 63) and both rankings
against the numpy statement (tests/np_orb_wta.py), through the C-ABI: random image sizes, content, FAST thresholds, budgets, capacities,
pyramid levels, batch sizes, edge thresholds, pools, and a second setting on the same detector.  Test infrastructure.  Run on a GPU box
from the repo root:
    python tests/fuzz_orb_wta.py [--seconds 120] [--seed 1]
Prints one line per mismatch with everything needed to replay it; exit code 1 if any.  Nothing is skipped: the edge threshold is drawn
first and the patch sizes from those it admits."""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "stvo-pl_amd", "python")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import np_orb_wta as nw
from fuzz_orb_harris import make_image, same_bits
from stvo_amd import capi

KEYS = ("kp", "response", "angle", "desc", "octave")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=120.0)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--cases", type=int, default=0, help="stop after this many cases (0: run for --seconds)")
    ap.add_argument("--max-size", type=int, default=400, help="largest image side drawn")
    args = ap.parse_args(argv)
    ctx = capi.Context(device_id=0, max_rows=2048, max_batch=8)
    t_end = time.time() + args.seconds
    case, bad, ran, seen = 0, 0, 0, set()
    try:
        while time.time() < t_end and (args.cases == 0 or case < args.cases):
            case += 1
            rng = np.random.default_rng([args.seed, case])
            edge = int(rng.choice([19, 19, 20, 23, 29, 31, 44, 50]))
            lo = 2 * edge + 1
            cols, rows = int(rng.integers(max(64, lo), max(args.max_size, lo + 40))), int(rng.integers(max(64, lo), max(args.max_size * 2 // 3, lo + 40)))
            B = int(rng.integers(1, 4))
            imgs = np.stack([make_image(rng, cols, rows) for _ in range(B)])
            nlev = int(rng.integers(1, 4)); th = int(rng.integers(5, 50)); nf = int(rng.choice([20, 50, 300, 1000]))
            cap = int(rng.choice([64, 256, 1024])); sf = float(rng.choice([1.2, 1.5, 2.0]))
            admitted = [P for P in range(2, 64) if P == 31 or nw.reach(P) <= edge]
            settings = [(int(rng.integers(2, 5)), int(rng.choice(admitted)), int(rng.integers(0, 2))) for _ in range(2)]
            pool = rng.integers(-13, 14, (512, 2)).astype(np.int8) if rng.integers(0, 2) else None
            tag = f"seed {args.seed} case {case} {cols}x{rows} B {B} nf {nf} th {th} levels {nlev} x {sf} cap {cap} edge {edge} pool {pool is not None} settings {settings}"
            orb = capi.Orb(ctx, B, cols, rows, max_keypoints=cap, nfeatures=nf, fast_threshold=th, edge_threshold=edge, nlevels=nlev, scale_factor=sf)
            try:
                if pool is not None:
                    orb.set_pattern(pool)
                base = orb.pattern().reshape(512, 2) if pool is None else pool
                for step, (k, P, score) in enumerate(settings):
                    orb.set_descriptor(k, P)
                    orb.set_score_type(score)
                    seen.add((k, P > 31, score))
                    out = orb.detect(imgs)
                    for b in range(B):
                        ref = nw.detect_levels(imgs[b], nf, nlev, sf, th, edge, base, cap, k, P, score)
                        ok = all(same_bits(out[b][key], ref[key]) for key in KEYS) and out[b]["n_total"] == ref["n_total"]
                        ran += 1
                        if not ok:
                            bad += 1
                            print(f"MISMATCH {tag} step {step} image {b}: got {len(out[b]['kp'])} / n_total {out[b]['n_total']}, "
                                  f"expected {len(ref['kp'])} / {ref['n_total']}", flush=True)
                    if step == 0:
                        orb.set_descriptor(2, 31)   # the pool is read back under the default setting
                        base = orb.pattern().reshape(512, 2)
            finally:
                orb.close()
    finally:
        ctx.close()
    print(f"fuzz_orb_wta: {case} cases, {ran} detections compared, {len(seen)} of 12 (wta_k, instance, ranking) classes, {bad} mismatches", flush=True)
    if args.cases and case < args.cases:
        print(f"fuzz_orb_wta: only {case} of {args.cases} cases ran in {args.seconds} s", flush=True)
        return 1
    return 1 if bad or ran == 0 else 0


if __name__ == "__main__":
    sys.exit(main())
