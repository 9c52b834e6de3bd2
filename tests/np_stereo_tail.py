"""The tails of the stereo association as a plain second statement — TEST INFRASTRUCTURE ONLY.

Written from the reference's text: the point tail src/stereoFrame.cpp:152-172, the line tail :351-395 with
filterLineSegmentDisparity :405-415 and lineSegmentOverlapStereo :473-508, PinholeStereoCamera::backProjection
(src/pinholeStereoCamera.cpp:221-229) and the LineFeature constructor / safeCopy scalings (src/stereoFeatures.cpp:107-135).
Input: the raw features, the raw stereo matches m12 (the grid matcher is tested elsewhere), the camera, the match parameters.

Decisions are taken in the reference's own types: np.float32 subtraction where the reference subtracts floats (:157, :159),
np.float64 scalars one operation at a time everywhere else (numpy scalar arithmetic is IEEE and never contracts), std::min /
std::max spelled out as the standard defines them — never fmin / fmax, which differ on NaN.  The kept records are computed twice:
in float64 in the reference's order, and in numpy.longdouble from the same float inputs (what the values would be without the
roundings of double).  Every left feature gets a tag naming the branch that decided its fate."""
import numpy as np

F32, F64, LD = np.float32, np.float64, np.longdouble

# ---- branch tags -------------------------------------------------------------------------------------------------------------
NONE, EPIPOLAR, DISPARITY, RATIO, HORIZONTAL, OV_DISJOINT, OV_SPANS, OV_PARTIAL, OV_SHORT, KEPT = range(10)
TAG_NAMES = ["no match", "epipolar", "disparity", "ratio", "horizontal", "overlap: disjoint", "overlap: right spans left",
             "overlap: partial", "overlap: length <= 0.01f", "kept"]
# the outcomes of lineSegmentOverlapStereo (:473-508); OV_FLAT is the left segment below line_horiz_th (overlap stays 1)
OV_FLAT = 10
OV_NAMES = {OV_FLAT: "flat left segment", OV_DISJOINT: "disjoint", OV_SPANS: "right spans left", OV_PARTIAL: "partial",
            OV_SHORT: "length <= 0.01f"}


def std_min(a, b):
    """std::min(a, b): (b < a) ? b : a"""
    return b if b < a else a


def std_max(a, b):
    """std::max(a, b): (a < b) ? b : a"""
    return b if a < b else a


def _mp(mp):
    return {k: F64(getattr(mp, k)) for k in ("max_dist_epip", "min_disp", "stereo_overlap_th", "line_horiz_th", "ls_min_disp_ratio",
                                             "orb_scale_factor", "lsd_scale")}


def back_projection(cam, u, v, disp, T=F64):
    """pinholeStereoCamera.cpp:221-229"""
    bd = T(cam["b"]) / T(disp)
    return [bd * (T(u) - T(cam["cx"])), bd * (T(v) - T(cam["cy"])), bd * T(cam["fx"])]


def level_sigma2(sigma2, scale, level, T=F64):
    """for (i < level) sigma2 *= scale;  sigma2 = 1.f / (sigma2 * sigma2)   (stereoFeatures.cpp:44-46, :112-114, :126-128)"""
    s = T(sigma2)
    for _ in range(int(level)):
        s = s * T(scale)
    return T(F32(1.0)) / (s * s)


# ---- points (:152-172) ---------------------------------------------------------------------------------------------------------
def stereo_points(kp_l, oct_l, kp_r, m12, cam, mp):
    """-> dict(tag [nl], src [k] kept left indices in order, rc [k, 4] float32 {u, v, float disparity, level}, P / P_ld [k, 3],
    sigma2 [k]).  Element-wise over the frame: every numpy array operation below is one IEEE operation per element in the type of
    its operands, exactly as the scalar form."""
    p = _mp(mp)
    kp_l = np.asarray(kp_l, F32).reshape(-1, 2); kp_r = np.asarray(kp_r, F32).reshape(-1, 2)
    m12 = np.asarray(m12, np.int64)[:len(kp_l)]
    tag = np.full(len(kp_l), NONE, np.int32)
    i1 = np.nonzero(m12 >= 0)[0]
    i2 = m12[i1]
    with np.errstate(all="ignore"):
        dy = kp_l[i1, 1] - kp_r[i2, 1]  # float - float (:157)
        dx = kp_l[i1, 0] - kp_r[i2, 0]  # float - float, then widened: double disp_ = ... (:159)
        assert dy.dtype == F32 and dx.dtype == F32
        epi = np.abs(dy).astype(F64) <= p["max_dist_epip"]
        dsp = dx.astype(F64) >= p["min_disp"]
        tag[i1] = np.where(epi, np.where(dsp, KEPT, DISPARITY), EPIPOLAR)
        src = i1[epi & dsp].astype(np.int32)
        d32 = dx[epi & dsp]
        u, v = kp_l[src, 0], kp_l[src, 1]
        lvl = np.asarray(oct_l, np.int32)[src]
        rc = np.stack([u, v, d32, lvl.astype(F32)], axis=1).astype(F32).reshape(len(src), 4)
        P = np.stack(back_projection(cam, u.astype(F64), v.astype(F64), d32.astype(F64), np.asarray), axis=1).reshape(len(src), 3)
        Pld = np.stack(back_projection(cam, u.astype(LD), v.astype(LD), d32.astype(LD), lambda x: np.asarray(x, LD)), axis=1).reshape(len(src), 3)
        s2 = np.array([level_sigma2(1.0, p["orb_scale_factor"], l) for l in lvl], F64)
    return dict(tag=tag, src=src, rc=rc, P=P, P_ld=Pld, sigma2=s2)


# ---- lines -----------------------------------------------------------------------------------------------------------------------
def row_overlap(spl_obs, epl_obs, spl_proj, epl_proj, horiz_th):
    """lineSegmentOverlapStereo (:473-508) -> (overlap, branch).  overlap = 1.f; 0.f; 0.01f are floats widened to double."""
    spl_obs, epl_obs, spl_proj, epl_proj = F64(spl_obs), F64(epl_obs), F64(spl_proj), F64(epl_proj)
    overlap = F64(F32(1.0))
    branch = OV_FLAT
    with np.errstate(all="ignore"):
        if np.abs(epl_obs - spl_obs) > F64(horiz_th):
            sln = std_min(spl_obs, epl_obs); eln = std_max(spl_obs, epl_obs)
            spn = std_min(spl_proj, epl_proj); epn = std_max(spl_proj, epl_proj)
            length = eln - spn
            if (epn < sln) or (spn > eln):
                overlap = F64(F32(0.0)); branch = OV_DISJOINT
            elif (epn > eln) and (spn < sln):
                overlap = eln - sln; branch = OV_SPANS
            else:
                overlap = std_min(eln, epn) - std_max(sln, spn); branch = OV_PARTIAL
            if length > F64(F32(0.01)):
                overlap = overlap / length
            else:
                overlap = F64(F32(0.0))
                if branch != OV_DISJOINT:  # (a right segment below the left one has length < 0 too: its overlap was 0 already)
                    branch = OV_SHORT
            if overlap > F64(F32(1.0)):
                overlap = F64(F32(1.0))
    return overlap, branch


def line_disparities(spl_x, epl_x, spr_x, epr_x, min_ratio):
    """filterLineSegmentDisparity (:405-415) -> (disp_s, disp_e, reset)"""
    with np.errstate(all="ignore"):
        ds = F64(spl_x) - F64(spr_x)
        de = F64(epl_x) - F64(epr_x)
        if std_min(ds, de) / std_max(ds, de) < F64(min_ratio):
            return F64(-1.0), F64(-1.0), True
    return ds, de, False


def reintersect(sp_l, ep_l, sp_r, ep_r, T=F64, quirk=True):
    """:366-367 — the right segment's abscissae at the left end rows.  The second line reads sp_r AFTER the first has overwritten it
    (quirk = True, the reference); quirk = False is what the text presumably meant, for the tests that show the two differ."""
    sp_l = [T(v) for v in sp_l]; ep_l = [T(v) for v in ep_l]; sp_r = [T(v) for v in sp_r]; ep_r = [T(v) for v in ep_r]
    with np.errstate(all="ignore"):
        spx = (sp_r[0] * (sp_l[1] - ep_r[1]) + ep_r[0] * (sp_r[1] - sp_l[1])) / (sp_r[1] - ep_r[1])
        q = [spx, sp_l[1]] if quirk else sp_r
        epx = (q[0] * (ep_l[1] - ep_r[1]) + ep_r[0] * (q[1] - ep_l[1])) / (q[1] - ep_r[1])
    return spx, epx


def _rel_margin(q, t):
    """how far the extended-precision quantity q is from its threshold t, relative to the larger of the two (inf where q is not finite:
    such a comparison has one answer in any arithmetic)"""
    q, t = LD(q), LD(t)
    if not np.isfinite(q):
        return np.inf
    return float(abs(q - t) / max(abs(q), abs(t), LD(1e-300)))


def stereo_lines(kl_l, oct_ll, kl_r, m12, cam, mp, quirk=True):
    """-> dict(tag, ov [nl] (branch of the overlap, -1 unmatched), margin [nl] (smallest relative distance of a decision's quantity,
    in extended precision, from its threshold), src [k], spl, epl [k, 2], sdisp, edisp [k], sP, eP, le [k, 3], s2l, s2lm [k], and the
    same values in longdouble: sdisp_ld, edisp_ld, sP_ld, eP_ld, le_ld, plus xr [k, 2] (the right abscissae that went in: the floors of
    the comparison with the device are derived from them))"""
    p = _mp(mp)
    kl_l = np.asarray(kl_l, F32).reshape(-1, 4); kl_r = np.asarray(kl_r, F32).reshape(-1, 4)
    n = len(kl_l)
    tag = np.full(n, NONE, np.int32); ov = np.full(n, -1, np.int32); margin = np.full(n, np.inf)
    out = {k: [] for k in ("src", "spl", "epl", "sdisp", "edisp", "sP", "eP", "le", "s2l", "s2lm", "sdisp_ld", "edisp_ld", "sP_ld",
                           "eP_ld", "le_ld", "xr")}
    with np.errstate(all="ignore"):
        for i1 in range(n):
            i2 = int(m12[i1])
            if i2 < 0:
                continue
            sp_l = [F64(kl_l[i1, 0]), F64(kl_l[i1, 1]), F64(1.0)]
            ep_l = [F64(kl_l[i1, 2]), F64(kl_l[i1, 3]), F64(1.0)]
            # le_l = sp_l x ep_l, divided by sqrt(le0^2 + le1^2)   (:358)
            le = [sp_l[1] * ep_l[2] - sp_l[2] * ep_l[1], sp_l[2] * ep_l[0] - sp_l[0] * ep_l[2], sp_l[0] * ep_l[1] - sp_l[1] * ep_l[0]]
            nrm = np.sqrt(le[0] * le[0] + le[1] * le[1])
            le = [le[0] / nrm, le[1] / nrm, le[2] / nrm]
            sp_r = [F64(kl_r[i2, 0]), F64(kl_r[i2, 1])]
            ep_r = [F64(kl_r[i2, 2]), F64(kl_r[i2, 3])]
            overlap, ov[i1] = row_overlap(sp_l[1], ep_l[1], sp_r[1], ep_r[1], p["line_horiz_th"])  # :363, on the ORIGINAL right rows
            spx, epx = reintersect(sp_l, ep_l, sp_r, ep_r, F64, quirk)
            ds, de, reset = line_disparities(sp_l[0], ep_l[0], spx, epx, p["ls_min_disp_ratio"])
            # the same quantities without double's roundings, for the margins and for the records
            spx_ld, epx_ld = reintersect(sp_l, ep_l, sp_r, ep_r, LD, quirk)
            ds_ld, de_ld = LD(sp_l[0]) - spx_ld, LD(ep_l[0]) - epx_ld
            m = [_rel_margin(std_min(ds_ld, de_ld) / std_max(ds_ld, de_ld), p["ls_min_disp_ratio"])]
            if not reset:
                m += [_rel_margin(ds_ld, p["min_disp"]), _rel_margin(de_ld, p["min_disp"])]
            if ov[i1] in (OV_SPANS, OV_PARTIAL):
                m.append(_rel_margin(LD(overlap), p["stereo_overlap_th"]))
            margin[i1] = min(m)
            # :371-374, clause by clause; after :366-367 the right rows ARE the left rows
            rdy = np.abs(sp_l[1] - ep_l[1])
            if not (ds >= p["min_disp"] and de >= p["min_disp"]):
                tag[i1] = RATIO if reset else DISPARITY
            elif not (np.abs(sp_l[1] - ep_l[1]) > p["line_horiz_th"] and rdy > p["line_horiz_th"]):
                tag[i1] = HORIZONTAL
            elif not (overlap > p["stereo_overlap_th"]):
                tag[i1] = ov[i1]
                assert ov[i1] != OV_FLAT or p["stereo_overlap_th"] >= 1.0
            else:
                tag[i1] = KEPT
                lvl = int(oct_ll[i1])
                s2 = level_sigma2(1.0, p["lsd_scale"], lvl)  # the constructor of :382 (stereoFeatures.cpp:107-115)
                out["src"].append(i1)
                out["spl"].append(sp_l[:2]); out["epl"].append(ep_l[:2]); out["sdisp"].append(ds); out["edisp"].append(de)
                out["sP"].append(back_projection(cam, sp_l[0], sp_l[1], ds)); out["eP"].append(back_projection(cam, ep_l[0], ep_l[1], de))
                out["le"].append(le)
                out["s2l"].append(s2)
                out["s2lm"].append(level_sigma2(s2, p["lsd_scale"], lvl))  # safeCopy scales once more (:117-135)
                out["sdisp_ld"].append(ds_ld); out["edisp_ld"].append(de_ld)
                out["sP_ld"].append(back_projection(cam, sp_l[0], sp_l[1], ds_ld, LD))
                out["eP_ld"].append(back_projection(cam, ep_l[0], ep_l[1], de_ld, LD))
                a = [LD(v) for v in sp_l]; b = [LD(v) for v in ep_l]
                c = [a[1] - b[1], b[0] - a[0], a[0] * b[1] - a[1] * b[0]]
                nl_ = np.sqrt(c[0] * c[0] + c[1] * c[1])
                out["le_ld"].append([c[0] / nl_, c[1] / nl_, c[2] / nl_])
                out["xr"].append([sp_r[0], ep_r[0]])
    k = len(out["src"])
    shp = dict(src=(k,), spl=(k, 2), epl=(k, 2), sdisp=(k,), edisp=(k,), sP=(k, 3), eP=(k, 3), le=(k, 3), s2l=(k,), s2lm=(k,),
               sdisp_ld=(k,), edisp_ld=(k,), sP_ld=(k, 3), eP_ld=(k, 3), le_ld=(k, 3), xr=(k, 2))
    res = {key: np.array(v, np.int32 if key == "src" else (LD if key.endswith("_ld") else F64)).reshape(shp[key]) for key, v in out.items()}
    res.update(tag=tag, ov=ov, margin=margin)
    return res
