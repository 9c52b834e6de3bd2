#!/usr/bin/env python3
"""The rectifier bank (stvo_rectify_bank_*) on one MI355X: one launch for mixed calibrations next to the three uniform rectifiers on
the same images, and ImagePipeline with the bank next to the same pipeline fed pre-rectified grey slots.  Writes --out
(profiles/rectify_bank_bench.json) and prints it.  python tools/bench_rectify_bank.py [--pairs 256] [--streams 128] [--iters 20] [--rounds 5]

  copy      the HBM copy rate of this run: a device-to-device copy of 1 GiB, (bytes read + bytes written) / time
  rectify   --pairs pairs round robin over KITTI 00-02 (1241 x 376, a copy), KITTI 03 (1242 x 375, a copy) and EuRoC (752 x 480, rad-tan)
            in slots of 1242 x 480: grey remap, B, G, R remap and the fused B, G, R -> grey form, the bank's one launch against the three
            uniform calls (each on its own compact buffer of the same images), alternating, --iters launches per window between device
            events, the window ending in a synchronise; the outputs are compared crop by crop first.  Bytes moved = what the algorithm
            must move (every source image read once, every destination written once, every map set read once), as a share of the copy rate
  pipeline  ImagePipeline(cam=[...], rectify=bank) at --streams streams on raw grey and on raw B, G, R slots against
            ImagePipeline(cam=[...]) on the grey slots the bank wrote: ms per enqueued step, alternating"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=256)
ap.add_argument("--streams", type=int, default=128)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rectify_bank_bench.json"))
a = ap.parse_args()
sys.path.insert(0, os.path.join(ROOT, "stvo-pl_amd", "python"))
import torch  # noqa: E402
from stvo_amd import capi, images, synth  # noqa: E402
from stvo_amd.ctypes_types import match_params, opt_params  # noqa: E402

SLOT_C, SLOT_R = 1242, 480
PARAMS = os.path.join(ROOT, "tests", "golden", "dataset_params")


def calibs():
    k03 = capi.RectCalib()   # config/dataset_params/kitti03.yaml: the KITTI form, no distortion
    c = synth.KITTI03_CAM
    k03.form, k03.width, k03.height, k03.b = capi.RECT_FORM_KITTI, c["width"], c["height"], c["b"]
    k03.fx, k03.fy, k03.cx, k03.cy = c["fx"], c["fy"], c["cx"], c["cy"]
    return [("kitti00-02", capi.read_dataset_params(os.path.join(PARAMS, "kitti00-02.yaml"))), ("kitti03", k03),
            ("euroc", capi.read_dataset_params(os.path.join(PARAMS, "euroc_params.yaml")))]


def window(fn, iters):
    """ms per call: device events around `iters` calls, the window ending in a synchronise"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def alternate(fns, iters, rounds, warm=3):
    """{name: [ms per call of every round]}, the candidates taking turns"""
    for fn in fns.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    runs = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            runs[k].append(window(fn, iters))
    return runs


def summary(runs):
    return {k: dict(ms_runs=[round(v, 4) for v in r], ms_median=round(statistics.median(r), 4)) for k, r in runs.items()}


out = dict(tool="tools/bench_rectify_bank.py", device=torch.cuda.get_device_name(0), slot=[SLOT_C, SLOT_R], iters=a.iters, rounds=a.rounds)
ctx = capi.Context(0, 2048, max(4, a.streams))
ctx.set_stream(torch.cuda.current_stream().cuda_stream)

# ---- the copy rate of this run ------------------------------------------------------------------------------------------------------
n_copy = 1 << 30
src = torch.empty(n_copy, dtype=torch.uint8, device="cuda").random_(0, 256)
dst = torch.empty_like(src)
copy_runs = alternate(dict(copy=lambda: dst.copy_(src)), 10, a.rounds)["copy"]
copy_rate = 2 * n_copy / (statistics.median(copy_runs) * 1e-3)
out["hbm_copy"] = dict(bytes_each_way=n_copy, ms_runs=[round(v, 4) for v in copy_runs], bytes_per_s_read_plus_write=copy_rate)
del src, dst

# ---- one launch against three ------------------------------------------------------------------------------------------------------
P = a.pairs
named = calibs()
rects = [capi.Rectifier(ctx, P, calib=c) for _, c in named]
sizes = [(r.cols, r.rows) for r in rects]
bank = capi.RectifierBank(ctx, P, SLOT_C, SLOT_R, rects)
assign = [b % 3 for b in range(P)]
bank.assign(assign)
members = [[b for b in range(P) if assign[b] == k] for k in range(3)]
out["calibrations"] = [dict(name=n, size=list(sizes[k]), dist=rects[k].dist, pairs=len(members[k])) for k, (n, _) in enumerate(named)]
legs = {}
for leg, ch, fused in (("grey", 1, False), ("bgr", 3, False), ("bgr_to_grey", 3, True)):
    dch = 1 if fused else ch
    tail, dtail = ((ch,) if ch > 1 else ()), ((dch,) if dch > 1 else ())
    slots = torch.empty((2, P, SLOT_R, SLOT_C) + tail, dtype=torch.uint8, device="cuda").random_(0, 256)
    bdst = torch.zeros((2, P, SLOT_R, SLOT_C) + dtail, dtype=torch.uint8, device="cuda")
    comp, cdst = [], []   # the uniform rectifiers' compact buffers of the same images
    for k, (cols, rows) in enumerate(sizes):
        idx = torch.as_tensor(members[k], device="cuda")
        comp.append(slots[:, idx, :rows, :cols].contiguous())
        cdst.append(torch.zeros((2, len(members[k]), rows, cols) + dtail, dtype=torch.uint8, device="cuda"))
    torch.cuda.synchronize()

    def one(slots=slots, bdst=bdst, ch=ch, fused=fused):
        if fused:
            bank.rectify_color_to_gray_dev(P, ch, slots[0].data_ptr(), slots[1].data_ptr(), bdst[0].data_ptr(), bdst[1].data_ptr())
        else:
            bank.rectify_dev(P, ch, slots[0].data_ptr(), slots[1].data_ptr(), bdst[0].data_ptr(), bdst[1].data_ptr())

    def three(comp=comp, cdst=cdst, ch=ch, fused=fused):
        for k, r in enumerate(rects):
            s, d, n = comp[k], cdst[k], len(members[k])
            if fused:
                r.rectify_color_to_gray_dev(n, ch, s[0].data_ptr(), s[1].data_ptr(), d[0].data_ptr(), d[1].data_ptr())
            elif ch == 1:
                r.rectify_dev(n, s[0].data_ptr(), s[1].data_ptr(), d[0].data_ptr(), d[1].data_ptr())
            else:
                r.rectify_color_dev(n, ch, s[0].data_ptr(), s[1].data_ptr(), d[0].data_ptr(), d[1].data_ptr())
    one(); three()
    torch.cuda.synchronize()
    same = all(bool(torch.equal(bdst[:, torch.as_tensor(members[k], device="cuda"), :rows, :cols], cdst[k])) for k, (cols, rows) in enumerate(sizes))
    runs = alternate(dict(bank_one_launch=one, three_uniform_rectifiers=three), a.iters, a.rounds)
    moved = sum(2 * len(members[k]) * c * r * (ch + dch) + (2 * c * r * 12 if rects[k].dist else 0) for k, (c, r) in enumerate(sizes))
    leg_out = summary(runs)
    for v in leg_out.values():
        v["bytes_per_s"] = moved / (v["ms_median"] * 1e-3)
        v["share_of_copy_rate"] = round(v["bytes_per_s"] / copy_rate, 4)
    leg_out.update(pairs=P, channels=ch, bytes_moved=moved, crops_equal=same)
    legs[leg] = leg_out
    del slots, bdst, comp, cdst
out["rectify"] = legs
bank.close()

# ---- images -> poses ----------------------------------------------------------------------------------------------------------------
B = a.streams
mp, op = match_params("kitti"), opt_params("kitti", has_lines=0)
bank = capi.RectifierBank(ctx, B, SLOT_C, SLOT_R, rects)
assign = [b % 3 for b in range(B)]
cams = [rects[k].camera for k in assign]
raw = {1: torch.zeros((2, 2 * B, SLOT_R, SLOT_C), dtype=torch.uint8, device="cuda"),
       3: torch.zeros((2, 2 * B, SLOT_R, SLOT_C, 3), dtype=torch.uint8, device="cuda")}   # [frame][left B, right B] slots
for k, cam in enumerate(rects[j].camera for j in range(3)):
    seqs = [synth.make_stereo_image_sequence(50 + 4 * k + j, 2, cam) for j in range(2)]
    for b in (b for b in range(B) if assign[b] == k):
        for f in range(2):
            for side in range(2):
                im = torch.from_numpy(seqs[(b // 3) % 2][f][side]).cuda()
                raw[1][f, side * B + b, :cam["height"], :cam["width"]] = im
                raw[3][f, side * B + b, :cam["height"], :cam["width"]] = torch.stack([im, 255 - im, im // 2 + 60], -1)
pipes = dict(bank_grey=images.ImagePipeline(ctx, B, cams, mp, op, max_kp=2048, rectify=bank, calibs=assign),
             bank_bgr=images.ImagePipeline(ctx, B, cams, mp, op, max_kp=2048, rectify=bank, calibs=assign, channels=3),
             prerectified_grey=images.ImagePipeline(ctx, B, cams, mp, op, max_kp=2048))
# the pre-rectified slots: what the bank writes for the raw grey frames
pre = torch.zeros_like(raw[1])
torch.cuda.synchronize()
for f in range(2):
    bank.rectify_dev(B, 1, raw[1][f, :B].data_ptr(), raw[1][f, B:].data_ptr(), pre[f, :B].data_ptr(), pre[f, B:].data_ptr())
torch.cuda.synchronize()
state = {k: 0 for k in pipes}


def stepper(name, buf):
    def step():
        pipes[name].enqueue(img_ptr=buf[state[name] & 1].data_ptr())
        state[name] += 1
    return step


runs = alternate(dict(bank_grey=stepper("bank_grey", raw[1]), bank_bgr=stepper("bank_bgr", raw[3]),
                      prerectified_grey=stepper("prerectified_grey", pre)), a.iters, a.rounds, warm=4)
pl = summary(runs)
for name, p in pipes.items():
    res, counts = p.seq.read()
    pl[name].update(mean_stereo_points=float(counts[:, 0].mean()), poses_ok=int((res["status"] == 0).sum()))
pl.update(streams=B, metric="ms per enqueued step (bank + detection + ingest + pipeline step)",
          same_counts_grey=bool(np.array_equal(pipes["bank_grey"].seq.read()[1], pipes["prerectified_grey"].seq.read()[1])))
out["pipeline"] = pl
for p in pipes.values():
    p.close()
bank.close()
for r in rects:
    r.close()
ctx.close()
text = json.dumps(out, indent=1)
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write(text + "\n")
print(json.dumps(out))
