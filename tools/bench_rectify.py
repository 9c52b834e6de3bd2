"""Rectification throughput (stvo_rectify_images_dev) and its cost inside the images -> poses step.

  python tools/bench_rectify.py [--out profiles/rectify_bench.json]     (GPU)
  python tools/bench_rectify.py --isa                                   (no GPU: instruction mix of the one-channel remap kernel)

Remap: EuRoC calibration (tests/golden/dataset_params/euroc_params.yaml), 752 x 480, n = 1, 64 and 3072 pairs per launch (2 n
images), device buffers, hipEvent-free timing = host clock around `iters` launches ended by a device synchronise, after a warm-up.
Bytes per output pixel: the 1-B store, the source bytes (>= 1 B: each source byte is read once when the taps of neighbouring output
pixels hit the same cache lines) and the maps (6 B per pixel per side, read once per launch: 6 / n B per output pixel).
Step: ImagePipeline (key-points only, nlevels 4, EuRoC matching parameters) on B streams, enqueue + synchronise per step, with and
without the rectifier, alternating the two pipelines step by step."""
import argparse
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "stvo-pl_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
HBM_BYTES_PER_S = 8.0e12  # MI355X peak HBM3E bandwidth (8 TB/s); the ceiling of the roofline columns


def isa_mix():
    src = os.path.join(ROOT, "stvo-pl_amd", "csrc", "color_kernels.hip")  # rectify_color_kernel<1, false>: the grey remap
    inc = os.path.join(ROOT, "stvo-pl_amd", "csrc")
    asm = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", "-I", inc, src,
                          "-o", "-"], capture_output=True, text=True, check=True).stdout
    body = asm.split("rectify_color_kernelILi1ELb0EE", 1)[1].split(":", 1)[1]
    body = body.split("s_endpgm", 1)[0]
    counts = {}
    for line in body.splitlines():
        m = re.match(r"\s+([a-z_0-9]+)\b", line)
        if not m or line.strip().startswith(";") or m.group(1).startswith("."):
            continue
        op = m.group(1)
        cls = ("global_load" if op.startswith("global_load") else "global_store" if op.startswith("global_store") else
               "buffer" if op.startswith("buffer_") else "valu" if op.startswith("v_") else "salu/branch" if op.startswith("s_") else "other")
        counts[cls] = counts.get(cls, 0) + 1
        counts["op:" + op] = counts.get("op:" + op, 0) + 1
    return counts


def bench_remap(ctx, iters):
    import torch
    from stvo_amd import capi
    c = capi.read_dataset_params(os.path.join(ROOT, "tests", "golden", "dataset_params", "euroc_params.yaml"))
    px = c.width * c.height
    out = []
    for n in (1, 64, 3072):
        rect = capi.Rectifier(ctx, n, calib=c)
        src = torch.randint(0, 256, (2 * n, c.height, c.width), dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        torch.cuda.synchronize()
        s, d = src.data_ptr(), dst.data_ptr()
        it = max(3, iters // max(1, n // 16))
        for _ in range(3):
            rect.rectify_dev(n, s, s + n * px, d, d + n * px)
        ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(it):
            rect.rectify_dev(n, s, s + n * px, d, d + n * px)
        ctx.synchronize()
        dt = (time.perf_counter() - t0) / it
        imgs = 2 * n
        bytes_min = imgs * px * 2 + 2 * px * 6  # store + one read of every source byte + both maps
        out.append(dict(pairs=n, images_per_launch=imgs, ms_per_launch=dt * 1e3, images_per_s=imgs / dt,
                        bytes_per_output_px=bytes_min / (imgs * px), achieved_GBps_at_min_bytes=bytes_min / dt / 1e9,
                        share_of_hbm_peak=bytes_min / dt / HBM_BYTES_PER_S))
        del src, dst
        rect.close()
        torch.cuda.empty_cache()
    return out


def bench_step(B, steps):
    import numpy as np
    import torch
    from stvo_amd import capi, images, synth
    from stvo_amd.ctypes_types import match_params, opt_params
    c = capi.read_dataset_params(os.path.join(ROOT, "tests", "golden", "dataset_params", "euroc_params.yaml"))
    cam = capi.rectify_compute(c, maps=False)
    rc = dict(cam["cam"], width=c.width, height=c.height)
    pairs = synth.make_stereo_image_sequence(11, 2, rc)
    mp, op = match_params("euroc"), opt_params("euroc", has_lines=0)
    ctx = capi.Context(device_id=0, max_rows=2048, max_batch=B)
    rect = capi.Rectifier(ctx, B, calib=c)
    pipes = {"plain": images.ImagePipeline(ctx, B, rc, mp, op, max_kp=2048, nlevels=4),
             "rectify": images.ImagePipeline(ctx, B, rc, mp, op, max_kp=2048, nlevels=4, rectify=rect)}
    for p in pipes.values():
        p.set_images(np.stack([pairs[0][0]] * B), np.stack([pairs[0][1]] * B))
    torch.cuda.synchronize()
    times = {k: [] for k in pipes}
    for k in range(steps + 3):
        for name, p in pipes.items():
            t0 = time.perf_counter()
            p.enqueue()
            ctx.synchronize()
            if k >= 3:
                times[name].append(time.perf_counter() - t0)
    med = {k: float(np.median(v)) * 1e3 for k, v in times.items()}
    for p in pipes.values():
        p.close()
    rect.close()
    ctx.close()
    return dict(B=B, steps=steps, median_ms=med, added_fraction=med["rectify"] / med["plain"] - 1.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--isa", action="store_true")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.isa:
        mix = isa_mix()
        print(json.dumps(mix, indent=1, sort_keys=True))
        return
    from stvo_amd import capi
    ctx = capi.Context(device_id=0, max_rows=256, max_batch=1)
    res = dict(remap=bench_remap(ctx, a.iters))
    ctx.close()
    res["step"] = [bench_step(B, a.steps) for B in (1, 16)]
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
