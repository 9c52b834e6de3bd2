"""Feature tracks per stream — a plain numpy / Python statement of the rule the device pipeline's track kernel implements
(csrc/track_update.h), written from the reference, not from the kernel:

  * matchF2FPoints / matchF2FLines (src/stereoFrameHandler.cpp:144-152, :167-179) walk the previous frame's features i1 in ASCENDING
    order and, for i2 = matches_12[i1] >= 0, assign curr[i2].idx = prev[i1].idx — a later i1 that names the same i2 overwrites;
  * the stereo association numbers a new frame's features by position (src/stereoFrame.cpp:151,165,350,384);
  * currFrameIsKF renumbers by position (:1190-1206) for the frames that FOLLOW;
  * initialize (:35-52) treats the first frame as a key-frame (prev_f_iskf = true).

On top of idx the record carries age (matches in a row, saturating at 65535), kf (idx names a feature of the last key-frame) and inlier
(the pose kernel's flag of the previous feature, -1 when nothing matched).  TEST INFRASTRUCTURE ONLY."""
import numpy as np

RUN, RESTART, PARK = 0, 1, 2
TRACK = np.dtype([("idx", "<i4"), ("age", "<u2"), ("kf", "u1"), ("inlier", "i1")])


def fresh(n, kf):
    t = np.zeros(n, TRACK)
    t["idx"] = np.arange(n)
    t["kf"] = kf
    t["inlier"] = -1
    return t


def step(prev_state, m12, inl, n_cur, ctl=RUN, first=False, new_kf=0):
    """One stream, one feature kind.  prev_state: TRACK rows of the previous stereo set (as left by the previous call), m12 / inl: the
    f2f match and the inlier flag per previous feature (as long as prev_state; ignored for a first frame, RESTART and PARK).
    Returns (record [n_cur], state carried to the next step [n_cur])."""
    if first or ctl == RESTART:
        rec = fresh(n_cur, 1)
    elif ctl == PARK:
        rec = fresh(n_cur, 0)
    else:
        rec = fresh(n_cur, 0)
        m12 = np.asarray(m12[:len(prev_state)], np.int64)
        i1 = np.nonzero((m12 >= 0) & (m12 < n_cur))[0]     # ascending; numpy assigns the LAST value where an index repeats,
        i2 = m12[i1]                                       # which is what the reference's loop does
        rec["idx"][i2] = prev_state["idx"][i1]
        rec["age"][i2] = np.minimum(prev_state["age"][i1].astype(np.int64) + 1, 65535)
        rec["kf"][i2] = prev_state["kf"][i1]
        rec["inlier"][i2] = np.asarray(inl[:len(prev_state)])[i1]
    is_kf = first or ctl == RESTART or (ctl == RUN and new_kf == 1)
    if is_kf:                                      # currFrameIsKF / initialize: numbered by position from here on
        state = fresh(n_cur, 1)
        state["inlier"] = rec["inlier"]
    else:
        state = rec.copy()
    return rec, state


class Stream:
    """The chain of one stream, points and key-lines: feed it what the pipeline's existing interfaces report for every step."""

    def __init__(self):
        self.state = [np.zeros(0, TRACK), np.zeros(0, TRACK)]
        self.serial = 0

    def step(self, counts, m12=(None, None), inl=(None, None), n_prev=None, ctl=RUN, first=False, new_kf=0):
        """counts: (stereo points, stereo lines) of the step; m12 / inl: the stream's f2f rows (capacity long); n_prev: the previous
        counts as the f2f stage saw them (default: what the previous call was given; a stream under a control presents none)."""
        recs = []
        for k in range(2):
            prev = self.state[k]
            if n_prev is not None:
                prev = prev[:n_prev[k]]
            if first or ctl != RUN:
                prev = prev[:0]
            rec, self.state[k] = step(prev, m12[k], inl[k], int(counts[k]), ctl, first, new_kf)
            recs.append(rec)
        if first or ctl == RESTART:
            self.serial = 1
        elif ctl == RUN and new_kf == 1:
            self.serial += 1
        return recs
