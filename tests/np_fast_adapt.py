"""numpy statement of the adaptive FAST threshold rule, written from the reference's StereoFrameHandler::updateFrame
(src/stereoFrameHandler.cpp:66-86) line by line — the expectation stvo_fast_adapt_dev / stvo_seq_adapt_fast_dev are compared with.

    :68-72  int min_fast, max_fast, fast_inc, feat_th;  float err_th                  (Config::fastMinTh() ... fastErrTh())
    :75     if( curr_frame->DT == Matrix4d::Identity() || curr_frame->err_norm > err_th )
    :76         orb_fast_th = std::max( min_fast, orb_fast_th - 2*fast_inc );
    :78-79  else if( n_inliers_pt < feat_th )      the same
    :80-81  else if( n_inliers_pt < feat_th * 2 )  orb_fast_th = std::max( min_fast, orb_fast_th - fast_inc );
    :82-83  else if( n_inliers_pt > feat_th * 3 )  orb_fast_th = std::min( max_fast, orb_fast_th + fast_inc );
    :84-85  else if( n_inliers_pt > feat_th * 4 )  orb_fast_th = std::min( max_fast, orb_fast_th + 2*fast_inc );

Eigen's == on matrices is true when every coefficient compares equal (so -0.0 counts as 0); err_norm is a double and err_th a float,
so the comparison widens err_th: 0.3 compares as 0.300000011920929.  max / min clip on the side moved towards only: a threshold that
starts outside [min_fast, max_fast] on the other side is not pulled in."""
import numpy as np


def update(th, T, err, n_inliers_pt, min_th, max_th, inc_th, feat_th, err_th):
    """The threshold of the next detection of one stream, from what optimizePose left in curr_frame (T = DT, err = err_norm)."""
    th, n = int(th), int(n_inliers_pt)
    err_th = float(np.float32(err_th))
    T = np.asarray(T, np.float64).reshape(4, 4)
    if bool(np.all(T == np.eye(4))) or float(err) > err_th:
        th = max(min_th, th - 2 * inc_th)
    elif n < feat_th:
        th = max(min_th, th - 2 * inc_th)
    elif n < feat_th * 2:
        th = max(min_th, th - inc_th)
    elif n > feat_th * 3:
        th = min(max_th, th + inc_th)
    elif n > feat_th * 4:
        th = min(max_th, th + 2 * inc_th)
    return th


def update_batch(th, results, prm):
    """th [B] and results [B] (records with the fields T [16], err, n_inliers_pt) -> the new thresholds, int32 [B].
    prm: anything with the attributes min_th, max_th, inc_th, feat_th, err_th."""
    return np.array([update(th[b], results["T"][b], results["err"][b], results["n_inliers_pt"][b], prm.min_th, prm.max_th, prm.inc_th,
                            prm.feat_th, prm.err_th) for b in range(len(th))], np.int32)
