"""Developer check: the matrix-core matcher (K1m) against the VALU matcher (K1 + K1v) on the bench workload.
    STVO_KNN_MFMA=0 python tools/compare_knn_modes.py dump /tmp/a.npz ; STVO_KNN_MFMA=2 python tools/compare_knn_modes.py dump /tmp/b.npz
    python tools/compare_knn_modes.py cmp /tmp/a.npz /tmp/b.npz
Two builds against each other (STVO_LIB names the library), every form of launch_match on both paths, clustered descriptors:
    STVO_LIB=old/libstvo_hip.so python tools/compare_knn_modes.py dump_forms /tmp/old.npz ; python tools/compare_knn_modes.py dump_forms /tmp/new.npz
    python tools/compare_knn_modes.py cmp_forms /tmp/old.npz /tmp/new.npz        (exit status 1 unless every array is byte-identical)"""
import sys, os
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "stvo-pl_amd", "python"))
import numpy as np

CLUSTERED = dict(cluster_frac=0.6, cluster_size=8, spread_p=0.06)  # bench.py: CORRELATED_MODELS["clustered"]


def dump_forms(path):
    """One seeded run of every form on either path.  ONE_WAY and LAZY: the configs[1] batch (2000 rows in 2048, CMP_B frame pairs)
    through stvo_track_batched_dev with mutual = 0 / 1.  BOTH_DIRS: a single stream of the headline shape through the pipeline (the
    planner's route up to four streams); eight such streams for the pipeline's LAZY + SMALL routes.  m12 and the pose results."""
    import torch
    from stvo_amd import capi, synth
    from stvo_amd.ctypes_types import match_params, opt_params
    from stvo_amd.devbatch import TrackBatch
    B = int(os.environ.get("CMP_B", "64")); n = 2000
    out = {}
    frames = [synth.make_f2f_points(synth.frame_seed(40, k), n=n, desc_model="clustered", cluster_kw=CLUSTERED) for k in range(B)]
    seqs = [synth.make_stereo_sequence(synth.frame_seed(77, s), n_frames=5, n_pts=1650, n_lines=85, cam=synth.KITTI_CAM, cluster_kw=CLUSTERED)
            for s in range(8)]
    lib = capi.load()
    for path_name, mfma in (("mfma", None), ("valu", "0")):
        os.environ.pop("STVO_KNN_MFMA", None)
        if mfma is not None:
            os.environ["STVO_KNN_MFMA"] = mfma
        lib.stvo_debug_reparse_env()
        batch = TrackBatch(frames, max_pts=2048, max_lines=0, device="cuda:0")
        ctx = capi.Context(device_id=0, max_rows=2048, max_batch=B)
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        for form, mutual in (("one_way", 0), ("lazy", 1)):
            ctx.track_batched(batch, synth.KITTI_CAM, opt_params("kitti", has_lines=0), 0.75, 0.75, mutual)
            ctx.synchronize(); torch.cuda.synchronize()
            res = batch.results()
            pre = "%s.%s." % (path_name, form)
            out[pre + "m12"] = batch.m12_pts().copy()
            for k in ("T", "status", "iters", "n_inliers_pt"):
                out[pre + k] = np.array(res[k]).copy()
        ctx.close()
        for form, S in (("both_dirs", 1), ("pipeline8", 8)):
            ctx = capi.Context(device_id=0, max_rows=2048, max_batch=S)
            dev = capi.Sequences(ctx, S, 2048, 128, synth.KITTI_CAM, match_params("kitti"), opt_params("kitti"))
            dev.enable_fetch(True)
            for f in range(5):
                res, counts = dev.push([seqs[s][f] for s in range(S)])
                if f == 0:
                    continue
                m = dev.fetch_matches()
                pre = "%s.%s.step%d." % (path_name, form, f)
                out[pre + "m12p"], out[pre + "m12l"] = m[2], m[3]
                out[pre + "T"], out[pre + "status"], out[pre + "counts"] = res["T"].copy(), res["status"].copy(), counts.copy()
            dev.close(); ctx.close()
    os.environ.pop("STVO_KNN_MFMA", None)
    lib.stvo_debug_reparse_env()
    np.savez(path, **out)
    print("dumped", len(out), "arrays;", "matches per frame, lazy:", (out["mfma.lazy.m12"] >= 0).sum(1)[:4], "valu:", (out["valu.lazy.m12"] >= 0).sum(1)[:4],
          "single stream, last step:", int((out["mfma.both_dirs.step4.m12p"] >= 0).sum()))


def cmp_forms(pa, pb):
    a, b = np.load(pa), np.load(pb)
    bad = sorted(set(a.files) ^ set(b.files))
    for k in sorted(set(a.files) & set(b.files)):
        if a[k].dtype != b[k].dtype or a[k].shape != b[k].shape or a[k].tobytes() != b[k].tobytes():
            bad.append(k)
    print("%d arrays, %d bytes: %s" % (len(a.files), sum(a[k].nbytes for k in a.files), "byte-identical" if not bad else "DIFFERENT: " + ", ".join(bad)))
    return 1 if bad else 0


if sys.argv[1] == "dump_forms":
    dump_forms(sys.argv[2])
elif sys.argv[1] == "cmp_forms":
    sys.exit(cmp_forms(sys.argv[2], sys.argv[3]))
elif sys.argv[1] == "dump":
    import torch
    from stvo_amd import capi, synth
    from stvo_amd.ctypes_types import opt_params
    from stvo_amd.devbatch import TrackBatch
    B = int(os.environ.get("CMP_B", "64")); n = 2000
    frames = [synth.make_f2f_points(synth.frame_seed(0, k), n=n) for k in range(B)]
    batch = TrackBatch(frames, max_pts=2048, max_lines=0, device="cuda:0")
    ctx = capi.Context(device_id=0, max_rows=2048, max_batch=B)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ctx.track_batched(batch, synth.KITTI_CAM, opt_params("kitti", has_lines=0), 0.75, 0.75, 1)
    ctx.synchronize(); torch.cuda.synchronize()
    res = batch.results()
    np.savez(sys.argv[2], m12=batch.m12_pts(), T=res["T"], status=res["status"], iters=res["iters"], n_inl=res["n_inliers_pt"])
else:
    a, b = np.load(sys.argv[2]), np.load(sys.argv[3])
    same = (a["m12"] == b["m12"])
    print("m12 identical:", bool(same.all()), "differing entries:", int((~same).sum()), "of", same.size)
    if not same.all():
        bad = np.argwhere(~same)[:10]
        for f, i in bad:
            print("  frame", f, "row", i, a["m12"][f, i], b["m12"][f, i])
    print("matches per frame (a, b):", (a["m12"] >= 0).sum(1)[:8], (b["m12"] >= 0).sum(1)[:8])
    print("iters a:", a["iters"][:8], "b:", b["iters"][:8], " max |dT|:", float(np.abs(a["T"] - b["T"]).max()))
