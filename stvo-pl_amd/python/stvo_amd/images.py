"""Images in, poses out, nothing through the host: the ORB point front-end (stvo_orb_detect_dev) feeding the device-resident
per-frame pipeline (stvo_seq_upload_dev + stvo_seq_step_dev) for B stereo streams.  Plumbing for tests and bench only: torch
owns the device buffers, every computation is behind the C-ABI.

Replaces, per frame and stream: StereoFrame::detectStereoPoints + matchStereoPoints (/root/reference/src/stereoFrame.cpp:88-173),
StereoFrameHandler::f2fTracking + optimizePose (src/stereoFrameHandler.cpp:106-392); with lsd = stvo_lsd_params also
detectStereoLineSegments + matchStereoLines (:191-243, :309-398): LSD detector, top-N cut, LBD descriptors (stvo_lsd_* / stvo_lbd_*);
with fld = stvo_fld_params the FLD detector of use_fld_lines instead (:244-303, stvo_fld_*);
with rectify = capi.Rectifier also the rectification of the raw pairs that Dataset::nextFrame does first (src/dataset.cpp:147-157);
with channels = 3 / 4 the frames are interleaved colour (B, G, R[, A]) as Dataset::nextFrame reads them, and the grey images every
consumer of the reference makes for itself are made on the device (stvo_color_to_gray_dev / stvo_rectify_color_to_gray_dev)."""
import ctypes as C

import numpy as np
import torch

from . import capi
from .capi import FrameFeatures


class ImagePipeline:
    def __init__(self, ctx, B, cam, mp, op, max_kp=2048, nfeatures=2000, fast_threshold=20, edge_threshold=19, device="cuda:0", nlevels=1,
                 scale_factor=1.2, lsd=None, max_kl=128, rectify=None, fld=None, orb_score=1, adaptive_fast=None,
                 trajectory=None, trajectory_log=1, tracks=0, keyframe_sets=False, channels=1, gray_weights="q14", orb_wta_k=2,
                 orb_patch_size=31, calibs=None, lines_per_stream=False, lsd_min_length_ratio=None, fld_min_length_ratio=None,
                 lsd_many_waves=False):
        """cam: one camera dict (width / height = image size) for all B streams, or a list of B dicts, one camera AND image size per stream
        (KITTI 00-02 / 03 / 04-10 side by side): the resident image buffer is then cut in slots of the largest width x the largest height,
        stream b's images occupy the top-left of their slots (set_images takes a list of B arrays of each stream's own size), the
        detector reads every image at its own size (Orb.set_image_sizes) and the pipeline is created with the B cameras; a stream that
        RESTARTs may take another camera (enqueue / push_images: cams).  Key-points only unless asked otherwise: with a list, lsd and
        fld raise ValueError, and so do a rectify that is not a capi.RectifierBank and channels other than 1 without one.
        lines_per_stream = True (with a list and lsd; ValueError without either) is the opt-in for key-lines on such streams: the LSD
        detector and LBD are built at the slot size and read every image at its own size beside ORB (Lsd.set_image_sizes,
        Lbd.set_image_sizes), with and without a rectifier bank, at every built lsd_scale (the pipeline sets LSD_SIZES_ANY_RADIUS on its
        own copy of lsd: lsd_scale 0.5 and the other blur radii run the fused blur + resize per image too); lsd_min_length_ratio = r gives stream b the minimum line length
        r * min(width_b, height_b) of its own camera (the reference's Config::minLineLength() x min(width, height)), None keeps
        lsd.min_length for all; a stream that RESTARTs hands its new size and minimum length to both with its camera.
        lsd_many_waves = True (with a list, lsd and lines_per_stream; ValueError anywhere else) sets LSD_TABLE_BY_BATCH on that detector
        (Lsd.set_table_route): up to 64 streams — 128 images per launch — then run the many-wave search under their size table, as the
        same streams under one camera do; more streams stay on one wave per image.  The same bytes either way; False (the default)
        keeps one wave per image at every B.
        lines_per_stream = True with a list and fld (not both detectors) is the same opt-in for the FLD detector of use_fld_lines: it
        and LBD are built at the slot size and read every stream's images at that stream's own size (Fld.set_image_sizes);
        fld_min_length_ratio = r gives stream b the length threshold int(r * min(width_b, height_b)) of its own camera (the reference's
        llength_th truncated by createFastLineDetector(int)), None keeps fld.length_threshold for all; the detector is created at the
        smallest threshold among fld.length_threshold and the initial streams', which sizes its stores: a camera that a RESTART brings
        later and whose image those stores cannot hold under its own threshold raises ValueError before anything is staged.  With a
        rectifier bank and channels 3 / 4 FLD and its LBD read the swapped-weight plane gray_b in the slot layout.
        With a list, rectify = capi.RectifierBank and calibs = [B ints]: the frames are RAW, stream b under calibration calibs[b] of the
        bank, whose size cam[b] must have; the slot is the bank's; enqueue first runs the bank's one launch over all streams (with
        channels 3 / 4 the fused colour -> grey form: set_images then takes lists of colour arrays into self.color) and the detector
        reads the rectified slots; a stream that RESTARTs may take another calibration with its camera (enqueue / push_images: calibs).
        nlevels / scale_factor: Config::orbNLevels /
        orbScaleFactor (the key-point octaves travel with the key-points: sigma2 = 1 / scale^(2 level)).  orb_score: Config::orbScore
        (1 FAST_SCORE, 0 HARRIS_SCORE ranking of the key-points).  orb_wta_k / orb_patch_size: Config::orbWtaK / orbPatchSize
        (capi.Orb: 2 .. 4 and 2 .. 63; the descriptor stays 32 bytes under the matchers' plain Hamming distance).  lsd: capi.lsd_params(...)
        for the key-line front-end (op.has_lines = 1, at most max_kl key-lines per image), None: key-points only (op.has_lines = 0).
        fld: capi.fld_params(...) instead of lsd, the FLD detector of use_fld_lines (src/stereoFrame.cpp:244-303); not both.
        rectify: a capi.Rectifier of the same context for at least B pairs of this size: enqueue first remaps the raw images into a
        resident rectified buffer (same stream, no host synchronisation) and the detectors read that buffer; cam is then the rectified
        camera (Rectifier.camera).  None: the images are taken as rectified.
        adaptive_fast: capi.fast_adapt_params(...) turns on the reference's adaptative_fast (StereoFrameHandler::updateFrame,
        src/stereoFrameHandler.cpp:66-86) per stream: self.fast_th (int32 [B] on the device, fast_threshold at first) is what the
        detector reads for the two images of stream b, and every enqueue ends with the rule moving it by that step's pose results —
        on the device, in stream order, the host never sees it.  None: one fixed threshold, no kernel added.
        trajectory: capi.traj_params(...) turns on the pose in the map frame and the key-frame decision per stream (the rest of
        optimizePose's "set estimated pose" block, :372-391, and needNewKF / currFrameIsKF, :1136-1218): every tracked step is followed
        by the update on the device, read_trajectory() returns the records of the last trajectory_log steps.  None: images -> poses as
        before, no launch and no allocation added.
        tracks: >= 1 turns on the feature tracks per stream (Sequences.set_tracks: which feature of the last key-frame every current
        stereo feature observes), read_tracks() returns the records of the last `tracks` steps; keyframe_sets: every stream also keeps
        the stereo set of its last key-frame (keyframe_headers / read_keyframe).  0: off, no launch and no allocation added.
        channels: 1, or 3 / 4 for interleaved colour frames uint8 [rows, cols, channels] (B, G, R[, A]; alpha ignored): self.color
        holds the 2 B colour frames, enqueue first makes the grey plane self.img from them (COLOR_BGR2GRAY in cvtColor's integer
        form gray_weights, "q14" of OpenCV 3.0 - 3.4.1 or "q15" of the later releases) — with a rectifier in the same kernel as the
        remap of the colour channels, as the reference rectifies the colour image and converts afterwards — and ORB reads it.  The
        line detector and LBD read it too, except with fld: the reference's FLD branch converts with CV_RGB2GRAY, so they read
        self.gray_b, the plane with the red and blue weights swapped, written by the same launch.  1: grey frames as before, no
        launch and no allocation added."""
        if channels not in (1, 3, 4):
            raise ValueError("ImagePipeline: channels is 1 (grey), 3 (B, G, R) or 4 (B, G, R, A)")
        if gray_weights not in capi.GRAY_WEIGHTS:
            raise ValueError("ImagePipeline: gray_weights is 'q14' or 'q15'")
        self.channels, self.gray_weights = channels, gray_weights
        self.ctx, self.B, self.K, self.M = ctx, B, max_kp, max_kl
        self.cams = None  # one camera per stream: the B dicts in force (a RESTART may bring another)
        self.bank = self.calibs = None  # a capi.RectifierBank and the calibration of every stream in force
        if not isinstance(cam, dict):
            cam = list(cam)
            if len(cam) != B:
                raise ValueError("ImagePipeline: cam is one dict or a list of B dicts")
            bank = rectify if isinstance(rectify, capi.RectifierBank) else None
            if lines_per_stream and lsd is None and fld is None:
                raise ValueError("ImagePipeline: lines_per_stream goes with lsd or fld (and cam as a list)")
            if lsd is not None and fld is not None:
                raise ValueError("ImagePipeline: one line detector, lsd or fld")
            for name, given in (("lsd", lsd is not None and not lines_per_stream), ("fld", fld is not None and not lines_per_stream),
                                ("rectify", rectify is not None and bank is None), ("channels", channels != 1 and bank is None)):
                if given:
                    raise ValueError(f"ImagePipeline: {name} is not available with one camera per stream (cam as a list): key-points only"
                                     " (rectify takes a capi.RectifierBank, which also takes channels 3 / 4; lsd and fld take lines_per_stream = True)")
            self.cams = cam
            if bank is not None:
                if bank.ctx is not ctx or bank.B < B:
                    raise ValueError("ImagePipeline: the rectifier bank must belong to the same context and hold B pairs")
                self.cols, self.rows = bank.slot_cols, bank.slot_rows  # the slot
                self.bank = bank
                self.calibs = self._check_calibs(calibs, cam)
            else:
                self.cols, self.rows = max(c["width"] for c in cam), max(c["height"] for c in cam)  # the slot
        else:
            self.cols, self.rows = cam["width"], cam["height"]
            if lines_per_stream:
                raise ValueError("ImagePipeline: lines_per_stream goes with one camera per stream (cam as a list) and lsd or fld")
            if isinstance(rectify, capi.RectifierBank):
                raise ValueError("ImagePipeline: a capi.RectifierBank goes with one camera per stream (cam as a list)")
        if self.bank is None and calibs is not None:
            raise ValueError("ImagePipeline: calibs goes with rectify = capi.RectifierBank and cam as a list")
        if lsd_many_waves and not (self.cams is not None and lsd is not None and lines_per_stream):
            raise ValueError("ImagePipeline: lsd_many_waves goes with one camera per stream (cam as a list), lsd and lines_per_stream = True")
        self.rectify = rectify
        self.lsd_min_length_ratio = lsd_min_length_ratio
        self.fld_min_length_ratio = fld_min_length_ratio
        if rectify is not None and self.bank is None and (rectify.ctx is not ctx or rectify.B < B or rectify.cols != self.cols or rectify.rows != self.rows):
            raise ValueError("ImagePipeline: the rectifier must belong to the same context, hold B pairs and match the image size")
        self.orb = capi.Orb(ctx, 2 * B, self.cols, self.rows, max_kp, nfeatures, fast_threshold, edge_threshold, nlevels, scale_factor,
                            score=orb_score, wta_k=orb_wta_k, patch_size=orb_patch_size)  # left images, then right
        if self.cams is not None:  # n = B on 2 B images: left image b and right image B + b share entry b
            try:
                self.orb.set_image_sizes([(c["width"], c["height"]) for c in self.cams])
                if self.bank is not None:
                    self.bank.assign(self.calibs + [0] * (self.bank.B - B))
            except Exception:
                self.orb.close()
                raise
        if lsd is not None and fld is not None:
            raise ValueError("ImagePipeline: one line detector, lsd or fld")
        fld_in = fld
        lp = lsd if lsd is not None else fld
        if lp is not None and (lp.nfeatures == 0 or lp.nfeatures > max_kl):
            import warnings
            warnings.warn(f"ImagePipeline: line nfeatures = {lp.nfeatures} against a capacity of {max_kl} key-lines per image: the strongest {max_kl} are kept")
        if lsd is not None and lines_per_stream:  # the opt-in has been given: a size per image at every built blur radius, on a copy
            lsd = capi.LsdParams.from_buffer_copy(lsd)
            lsd.flags |= capi.LSD_SIZES_ANY_RADIUS
        if fld is not None and lines_per_stream:  # the stores are cut for the smallest threshold the detector is given (stvo_fld_set_image_sizes)
            fld = capi.FldParams.from_buffer_copy(fld)
            fld.length_threshold = min([fld.length_threshold] + [L for L in self._fld_thresholds(self.cams, fld.length_threshold)])
        self.lsd = capi.Lsd(ctx, 2 * B, self.cols, self.rows, lsd, max_keylines=max_kl) if lsd is not None else None
        self.fld = capi.Fld(ctx, 2 * B, self.cols, self.rows, fld, max_keylines=max_kl) if fld is not None else None
        self.lines = self.lsd if self.lsd is not None else self.fld  # the key-line detector, or None
        self.lbd = capi.Lbd(ctx, 2 * B, self.cols, self.rows, max_keylines=max_kl) if self.lines is not None else None
        self.fld_length_threshold = fld_in.length_threshold if fld_in is not None else None  # the caller's, for streams without a ratio
        self.fld_store_threshold = fld.length_threshold if fld is not None else None      # the detector's: what its stores were cut for
        if self.cams is not None and self.lines is not None:  # n = B on 2 B images, as for ORB
            try:
                if lsd_many_waves:  # the size table below does not move the search off the route of the batch size
                    self.lsd.set_table_route(capi.LSD_TABLE_BY_BATCH)
                self._set_line_sizes(self.cams)
            except Exception:
                self.orb.close(); self.lines.close(); self.lbd.close()
                raise
        self.seq = capi.Sequences(ctx, B, max_kp, max_kl if self.lines is not None else 64, cam, mp, op)
        self.trajectory = trajectory
        if trajectory is not None:
            self.seq.set_trajectory(trajectory, trajectory_log)
        self.tracks, self.keyframe_sets = int(tracks), bool(keyframe_sets)
        if self.tracks or self.keyframe_sets:
            self.seq.set_tracks(log_steps=self.tracks, keyframe_sets=self.keyframe_sets)
        dev = torch.device(device)
        self.img = torch.zeros((2 * B, self.rows, self.cols), dtype=torch.uint8, device=dev)
        self.rect_img = torch.zeros((2 * B, self.rows, self.cols), dtype=torch.uint8, device=dev) if rectify is not None and channels == 1 else None
        self.color = self.gray_b = None  # colour frames in; the swapped-weight plane of the FLD branch
        if channels != 1:
            self.color = torch.zeros((2 * B, self.rows, self.cols, channels), dtype=torch.uint8, device=dev)
            if self.fld is not None:
                self.gray_b = torch.zeros((2 * B, self.rows, self.cols), dtype=torch.uint8, device=dev)
        self.kp = torch.zeros((2 * B, max_kp, 2), dtype=torch.float32, device=dev)
        self.resp = torch.zeros((2 * B, max_kp), dtype=torch.float32, device=dev)
        self.ang = torch.zeros((2 * B, max_kp), dtype=torch.float32, device=dev)
        self.desc = torch.zeros((2 * B, max_kp, 32), dtype=torch.uint8, device=dev)
        self.n = torch.zeros((2 * B,), dtype=torch.int32, device=dev)
        self.oct = torch.zeros((2 * B, max_kp), dtype=torch.int32, device=dev)
        ff = FrameFeatures()
        ff.stride_kp, ff.stride_kl = max_kp, 0
        ff.n_kp_l = C.c_void_p(self.n.data_ptr())
        ff.n_kp_r = C.c_void_p(self.n.data_ptr() + 4 * B)
        ff.kp_l = C.c_void_p(self.kp.data_ptr())
        ff.kp_r = C.c_void_p(self.kp.data_ptr() + 8 * B * max_kp)
        ff.desc_l = C.c_void_p(self.desc.data_ptr())
        ff.desc_r = C.c_void_p(self.desc.data_ptr() + 32 * B * max_kp)
        ff.oct_l = C.c_void_p(self.oct.data_ptr())
        if self.lines is not None:  # key-lines: records from the detector, descriptors from LBD, end points as the rows the ingest takes
            M = max_kl
            self.kl = torch.zeros((2 * B, M, 6), dtype=torch.float32, device=dev)   # stvo_keyline records (24 bytes)
            self.kl_xy = torch.zeros((2 * B, M, 4), dtype=torch.float32, device=dev)
            self.ldesc = torch.zeros((2 * B, M, 32), dtype=torch.uint8, device=dev)
            self.nl = torch.zeros((2 * B,), dtype=torch.int32, device=dev)
            ff.stride_kl = M
            ff.n_kl_l = C.c_void_p(self.nl.data_ptr())
            ff.n_kl_r = C.c_void_p(self.nl.data_ptr() + 4 * B)
            ff.kl_l = C.c_void_p(self.kl_xy.data_ptr())
            ff.kl_r = C.c_void_p(self.kl_xy.data_ptr() + 16 * B * M)
            ff.ldesc_l = C.c_void_p(self.ldesc.data_ptr())
            ff.ldesc_r = C.c_void_p(self.ldesc.data_ptr() + 32 * B * M)
        self.adaptive_fast = adaptive_fast
        self.fast_th = None
        if adaptive_fast is not None:
            self.fast_th = torch.full((B,), fast_threshold, dtype=torch.int32, device=dev)
            torch.cuda.current_stream(dev).synchronize()  # the fill ran on torch's stream, the library uses its own
            self.orb.set_fast_thresholds(self.fast_th)  # n_th = B on 2 B images: left image b and right image B + b share entry b
        self.fast_threshold = fast_threshold
        self.ff = ff  # (without a line detector every line pointer stays NULL: no key-lines; oct_ll NULL: one octave)
        self.slot = 0

    def _check_calibs(self, calibs, cams):
        """calibs as a list of B calibration indices of the bank, each of the size of its stream's camera"""
        if calibs is None or len(calibs) != self.B:
            raise ValueError("ImagePipeline: calibs takes one calibration index of the bank per stream (B entries)")
        calibs = [int(k) for k in calibs]
        for b, k in enumerate(calibs):
            if not 0 <= k < self.bank.K:
                raise ValueError(f"ImagePipeline: calibs[{b}] = {k} is not a calibration of the bank")
            if self.bank.sizes[k] != (cams[b]["width"], cams[b]["height"]):
                raise ValueError(f"ImagePipeline: stream {b}'s camera is {cams[b]['width']} x {cams[b]['height']}, calibration calibs[{b}] = {k} "
                                 f"of the bank {self.bank.sizes[k][0]} x {self.bank.sizes[k][1]}")
        return calibs

    def _fld_thresholds(self, cams, own):
        """the FLD length threshold of every stream's camera: int(ratio * min(width, height)) — llength_th as createFastLineDetector(int)
        truncates it (src/stereoFrameHandler.cpp:39, src/stereoFrame.cpp:257) — or the caller's where no ratio was given"""
        r = self.fld_min_length_ratio
        return [int(own) if r is None else int(r * min(c["width"], c["height"])) for c in cams]

    def _set_line_sizes(self, cams):
        """the size, and minimum line length or length threshold, of every stream's camera to the line detector and the line descriptor"""
        sizes = [(c["width"], c["height"]) for c in cams]
        if self.fld is not None:
            try:
                self.fld.set_image_sizes(sizes, self._fld_thresholds(cams, self.fld_length_threshold))
            except capi.StvoError as e:  # the store rule, or a size or threshold the detector does not take: nothing has changed
                raise ValueError(f"ImagePipeline: the FLD detector refuses a stream's camera: {e}") from e
        else:
            r = self.lsd_min_length_ratio
            self.lsd.set_image_sizes(sizes, None if r is None else [r * min(w, h) for w, h in sizes])
        self.lbd.set_image_sizes(sizes)

    def _calibs_after(self, control, calibs, new_cams):
        """The B calibrations in force once the RESTART streams of `control` have taken theirs from `calibs` (B entries, None for the
        others), checked against the cameras then in force."""
        if self.bank is None or control is None or len(calibs) != self.B:
            raise ValueError("ImagePipeline: calibs takes a rectifier bank, a control and B entries")
        ctl = np.asarray(control).reshape(-1)
        new = [k if k is not None and ctl[b] == capi.STREAM_RESTART else self.calibs[b] for b, k in enumerate(calibs)]
        return self._check_calibs(new, new_cams if new_cams is not None else self.cams)

    def _cams_after(self, control, cams):
        """The B cameras in force once the RESTART streams of `control` have taken theirs from `cams` (B entries, None for the others)."""
        if self.cams is None or control is None or len(cams) != self.B:
            raise ValueError("ImagePipeline: cams takes one camera per stream (cam as a list), a control and B entries")
        ctl = np.asarray(control).reshape(-1)
        new = [c if c is not None and ctl[b] == capi.STREAM_RESTART else self.cams[b] for b, c in enumerate(cams)]
        if any(c["width"] > self.cols or c["height"] > self.rows for c in new):
            raise ValueError("ImagePipeline: a camera's images are larger than the slot the pipeline was built with")
        if self.fld is not None:  # the store rule of stvo_fld_set_image_sizes, before anything is staged
            have = self.cols * self.rows // (self.fld_store_threshold + 1) + 1
            for b, (c, L) in enumerate(zip(new, self._fld_thresholds(new, self.fld_length_threshold))):
                need = c["width"] * c["height"] // (max(L, 0) + 1) + 1
                if L < 1 or need > have:
                    raise ValueError(f"ImagePipeline: stream {b}'s camera ({c['width']} x {c['height']}, FLD length threshold {L}) needs a store of "
                                     f"{need} segments, the detector (created at threshold {self.fld_store_threshold}) holds {have}")
        return new

    def set_images(self, left, right, cams=None):
        """left / right: uint8 [B, rows, cols] (numpy or torch), with channels 3 / 4 [B, rows, cols, channels]; copied into the
        resident image buffer.  With one camera per stream also two lists of B arrays [height_b, width_b] (with channels 3 / 4, which
        takes a rectifier bank, [height_b, width_b, channels] into self.color) of each stream's own size:
        each is placed top-left in its slot (what the slot holds beyond it is never read); cams: the B cameras whose sizes the images have,
        where they are not yet the ones in force (push_images with a RESTART)."""
        B = self.B
        cams = self.cams if cams is None else cams
        if self.cams is not None and isinstance(left, (list, tuple)):
            if len(left) != B or len(right) != B:
                raise ValueError("ImagePipeline.set_images: one image per stream and side")
            dst = self.img if self.channels == 1 else self.color
            tail = () if self.channels == 1 else (self.channels,)
            for side, imgs in ((0, left), (B, right)):
                for b, im in enumerate(imgs):
                    t = torch.as_tensor(im)
                    if tuple(t.shape) != (cams[b]["height"], cams[b]["width"]) + tail:
                        raise ValueError(f"ImagePipeline.set_images: stream {b} takes images of {cams[b]['width']} x {cams[b]['height']}")
                    dst[side + b, :t.shape[0], :t.shape[1]].copy_(t, non_blocking=True)
            return
        if self.channels != 1:
            self.color[:B].copy_(torch.as_tensor(left).reshape(B, self.rows, self.cols, self.channels), non_blocking=True)
            self.color[B:].copy_(torch.as_tensor(right).reshape(B, self.rows, self.cols, self.channels), non_blocking=True)
            return
        self.img[:B].copy_(torch.as_tensor(left).reshape(B, self.rows, self.cols), non_blocking=True)
        self.img[B:].copy_(torch.as_tensor(right).reshape(B, self.rows, self.cols), non_blocking=True)

    def enqueue(self, img_ptr=None, control=None, cams=None, calibs=None):
        """Detection + description of the 2 B resident images (or of the uint8 [2 B, rows, cols] device buffer at img_ptr: B left,
        then B right; with channels 3 / 4 the colour buffer [2 B, rows, cols, channels]), ingestion, one pipeline step — all
        asynchronous.  With a rectifier the images are raw and are rectified first.
        control: None, or B words capi.STREAM_RUN / STREAM_RESTART / STREAM_PARK for this step (Sequences.control_next_step): staged
        first, so that with adaptive_fast the restarted streams are detected at fast_threshold again (initialize sets orb_fast_th
        before it detects); the rule at the end of the step leaves the thresholds of restarted and parked streams alone.
        cams (one camera per stream only): None, or B entries — the camera dict of the sequence a RESTART stream begins, None for the
        others: the pipeline (Sequences.restart_cameras) and the detectors (Orb.set_image_sizes, and with lines_per_stream
        Lsd.set_image_sizes with the stream's minimum length, or Fld.set_image_sizes with its length threshold, and Lbd.set_image_sizes)
        take it before the detection; a camera the FLD stores cannot hold raises ValueError before anything is staged.
        calibs (rectifier bank only): None, or B entries — the calibration index a RESTART stream takes with its camera, None for the
        others; the size of every stream's calibration must be its camera's, else ValueError and nothing is staged."""
        new = self._cams_after(control, cams) if cams is not None else None
        new_k = self._calibs_after(control, calibs, new) if calibs is not None else None
        if self.bank is not None and new_k is None and new is not None:
            self._check_calibs(self.calibs, new)  # a camera of another size needs its calibration
        if control is not None:
            self.seq.control_next_step(control)
            cams_change = new is not None and new != self.cams
            calibs_change = new_k is not None and new_k != self.calibs
            if cams_change or calibs_change:
                # the detectors first: they validate every size, and what they and the bank have taken can be put back should the
                # pipeline refuse — none of them ever disagree, and a refused call leaves no control staged
                ctl = np.asarray(control).reshape(-1)
                try:
                    if cams_change:
                        self.orb.set_image_sizes([(c["width"], c["height"]) for c in new])
                        if self.lines is not None:
                            self._set_line_sizes(new)
                    if calibs_change:
                        self.bank.assign(new_k + [0] * (self.bank.B - self.B))
                    if cams_change:
                        self.seq.restart_cameras([c if ctl[b] == capi.STREAM_RESTART else None for b, c in enumerate(new)])
                except Exception:
                    self.orb.set_image_sizes([(c["width"], c["height"]) for c in self.cams])
                    if self.lines is not None:
                        self._set_line_sizes(self.cams)
                    if calibs_change:
                        self.bank.assign(self.calibs + [0] * (self.bank.B - self.B))
                    self.seq.control_next_step(np.zeros(self.B, np.int32))
                    raise
                if cams_change:
                    self.cams = new
                if calibs_change:
                    self.calibs = new_k
            if self.adaptive_fast is not None:
                self.seq.restart_fast_dev(self.fast_th, self.fast_threshold)
        ip = img_ptr if img_ptr is not None else (self.img if self.channels == 1 else self.color).data_ptr()
        ip, lp = self._grey_planes(ip)
        self.orb.detect_dev(ip, self.kp.data_ptr(), self.resp.data_ptr(), self.ang.data_ptr(), self.desc.data_ptr(),
                            self.n.data_ptr(), octave=self.oct.data_ptr())
        if self.lines is not None:
            self.lines.detect_dev(lp, self.kl.data_ptr(), None, self.nl.data_ptr())
            self.lbd.compute_dev(lp, self.kl.data_ptr(), self.nl.data_ptr(), self.ldesc.data_ptr())
            self.ctx._chk(self.ctx.lib.stvo_keylines_xy_dev(self.ctx.h, 2 * self.B, self.M, self.kl.data_ptr(), self.nl.data_ptr(), self.kl_xy.data_ptr()))
        self.seq.upload_dev(self.slot, self.ff)
        self.seq.step_dev(self.slot)
        if self.adaptive_fast is not None:
            self.seq.adapt_fast_dev(self.adaptive_fast, self.fast_th)
        self.slot ^= 1

    def _grey_planes(self, ip):
        """The frame at ip (raw or rectified, grey or colour, as the pipeline was made) -> (the grey planes ORB reads, the grey planes the
        line detector and LBD read): rectified first where there is a rectifier or a bank, the colour -> grey conversion fused into that
        pass; the two differ only with colour frames and a swapped plane (gray_b)."""
        side = self.B * self.rows * self.cols
        if self.channels != 1:
            ga = self.img.data_ptr()
            gb = self.gray_b.data_ptr() if self.gray_b is not None else None
            gb_r = gb + side if gb is not None else None
            if self.bank is not None:
                self.bank.rectify_color_to_gray_dev(self.B, self.channels, ip, ip + side * self.channels, ga, ga + side, gb, gb_r,
                                                    weights=self.gray_weights)
            elif self.rectify is not None:
                self.rectify.rectify_color_to_gray_dev(self.B, self.channels, ip, ip + side * self.channels, ga, ga + side, gb, gb_r,
                                                       weights=self.gray_weights)
            else:
                capi.color_to_gray_dev(self.ctx, 2 * self.B, self.rows, self.cols, self.channels, ip, ga, gb, weights=self.gray_weights)
            return ga, (gb if gb is not None else ga)
        if self.rectify is None:
            return ip, ip
        rp = self.rect_img.data_ptr()
        if self.bank is not None:
            self.bank.rectify_dev(self.B, 1, ip, ip + side, rp, rp + side)
        else:
            self.rectify.rectify_dev(self.B, ip, ip + side, rp, rp + side)
        return rp, rp

    def push_images(self, left, right, control=None, cams=None, calibs=None):
        """One frame of every stream: (pose results [B], counts [B, 4]) like Sequences.push.  control, cams, calibs: as for enqueue (the
        images of a stream that takes another camera have that camera's size)."""
        new = self._cams_after(control, cams) if cams is not None else None
        if calibs is not None:
            self._calibs_after(control, calibs, new)  # refused before an image is taken
        self.set_images(left, right, cams=new)
        torch.cuda.current_stream().synchronize()  # the copies above ran on torch's stream, the library uses its own
        self.enqueue(control=control, cams=cams, calibs=calibs)
        return self.seq.read()

    def read_trajectory(self, n_last=1):
        """TRAJ_RECORD_DTYPE [n, B]: Tfw / Tfw_cov (before a key-frame reset), entropy_ratio, t, r, new_kf, frame of the last
        n <= trajectory_log tracked steps, oldest first (Sequences.read_trajectory; synchronises)."""
        if self.trajectory is None:
            raise ValueError("ImagePipeline.read_trajectory: built without trajectory")
        return self.seq.read_trajectory(n_last)

    def read_tracks(self, n_last=1):
        """(points [n, B, K], lines [n, B, M] as TRACK_DTYPE, counts [n, B, 2]) of the last n <= tracks steps, oldest first
        (Sequences.read_tracks; synchronises)."""
        if not self.tracks:
            raise ValueError("ImagePipeline.read_tracks: built without tracks")
        return self.seq.read_tracks(n_last)

    def keyframe_headers(self):
        return self.seq.keyframe_headers()

    def read_keyframe(self, b):
        return self.seq.read_keyframe(b)

    def export_streams(self, streams):
        """(blobs uint8 [n, bytes], thresholds int32 [n] or None): everything the named streams carry into the next pair
        (Sequences.export_streams) and, with adaptive_fast, the FAST threshold their next detection reads — the caller's array, so it
        travels beside the blob.  Synchronises."""
        blobs = self.seq.export_streams(streams)   # (synchronises the context's stream: the rule behind the last step has run)
        th = None
        if self.fast_th is not None:
            th = self.fast_th.cpu().numpy()[np.asarray(streams, np.int64).reshape(-1)].astype(np.int32)
        return blobs, th

    def import_streams(self, streams, blobs, fast_thresholds=None):
        """The named streams continue from `blobs` (Sequences.import_streams: of this or another pipeline with the same features,
        camera and parameters); with adaptive_fast, fast_thresholds [n] become their thresholds (None: fast_threshold, as for a
        restarted stream).  The thresholds are written between two synchronisations of the context's stream and of torch's, which
        orders the write behind the rule of the last step and in front of the next detection."""
        self.seq.import_streams(streams, blobs)    # (synchronises the context's stream)
        if self.fast_th is not None:
            idx = torch.as_tensor(np.asarray(streams, np.int64).reshape(-1), device=self.fast_th.device)
            th = np.full(idx.numel(), self.fast_threshold, np.int32) if fast_thresholds is None else np.asarray(fast_thresholds, np.int32).reshape(-1)
            if th.size != idx.numel():
                raise ValueError("ImagePipeline.import_streams: one threshold per stream")
            self.fast_th[idx] = torch.as_tensor(th, device=self.fast_th.device)
            torch.cuda.current_stream(self.fast_th.device).synchronize()

    def fast_thresholds(self):
        """Host copy of the per-stream FAST thresholds the NEXT detection will read (synchronises); tests and tools."""
        if self.fast_th is None:
            raise ValueError("ImagePipeline.fast_thresholds: built without adaptive_fast")
        self.ctx.synchronize()
        return self.fast_th.cpu().numpy().copy()

    def close(self):
        self.seq.close()
        self.orb.close()
        if self.lines is not None:
            self.lines.close()
            self.lbd.close()
