"""One trajectory / key-frame update of one stream in extended precision — TEST INFRASTRUCTURE ONLY.

The judge of csrc/traj_update.h (host build and kernel alike): written from the reference's formulas — the "set estimated pose"
block of optimizePose (src/stereoFrameHandler.cpp:372-391), needNewKF / currFrameIsKF (:1136-1218) and the se(3) helpers of
src/auxiliar.cpp:113-197 — in numpy.longdouble (x87 80-bit: 64 mantissa bits, eps 1.08e-19), eleven more bits than any FP64
statement of the same products.  Every input is a double and converts exactly.  `dtype=np.float64` runs the same text in doubles
(used only where the oracle exports no piece of its own: the determinant under the entropy)."""
import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps < 1e-18, "numpy.longdouble is a double here: the extended-precision statement needs the x87 format"

FIELDS = ("Tfw", "Tfw_cov", "entropy_ratio", "t", "r", "entropy_first_prevKF", "cov_prevKF_currF")
ENTROPY_OF_SINGULAR = -999999999.99  # :1147
CV_PI = 3.1415926535897932384626433832795  # the double the reference divides by (:1159)


def initial_state():
    """As `initialize` leaves the handler (:35-51)."""
    return dict(Tfw=np.eye(4), Tfw_cov=np.eye(6), entropy_first_prevKF=0.0, T_prevKF=np.eye(4), cov_prevKF_currF=np.zeros((6, 6)),
                prev_f_iskf=1, N_prevKF_currF=0, n_frames=0, n_keyframes=0)


def _skew(v, dt):
    z = dt(0)
    return np.array([[z, -v[2], v[1]], [v[2], z, -v[0]], [-v[1], v[0], z]], dtype=dt)


def inverse_se3(T):
    R, t = T[:3, :3], T[:3, 3]
    o = np.eye(4, dtype=T.dtype)
    o[:3, :3] = R.T
    o[:3, 3] = -(R.T @ t)
    return o


def expmap_se3(x, dt=LD):
    x = np.asarray(x, dtype=dt)
    t, w = x[:3], x[3:]
    T = np.eye(4, dtype=dt)
    theta = np.sqrt(w @ w)
    if theta < dt(0.000001):
        R = np.eye(3, dtype=dt)
    else:
        s = _skew(w, dt) / theta
        I = np.eye(3, dtype=dt)
        R = I + s * np.sin(theta) + (s @ s) * (dt(1) - np.cos(theta))
        V = I + s * (dt(1) - np.cos(theta)) / theta + (s @ s) * (theta - np.sin(theta)) / theta
        t = V @ t
    T[:3, :3] = R
    T[:3, 3] = t
    return T


def _inv3(A):
    """cofactor inverse of a 3 x 3 (no LAPACK in extended precision)."""
    c = np.empty((3, 3), dtype=A.dtype)
    for i in range(3):
        for j in range(3):
            m = np.delete(np.delete(A, i, 0), j, 1)
            c[i, j] = (-1) ** (i + j) * (m[0, 0] * m[1, 1] - m[0, 1] * m[1, 0])
    det = A[0, 0] * c[0, 0] + A[0, 1] * c[0, 1] + A[0, 2] * c[0, 2]
    return c.T / det


def logmap_se3(T, dt=LD):
    T = np.asarray(T, dtype=dt)
    R, Vt = T[:3, :3], T[:3, 3]
    V = np.eye(3, dtype=dt)
    w = np.zeros(3, dtype=dt)
    cosine = (R[0, 0] + R[1, 1] + R[2, 2] - dt(1)) / dt(2)
    cosine = min(max(cosine, dt(-1)), dt(1))
    sine = min(np.sqrt(dt(1) - cosine * cosine), dt(1))
    theta = np.arccos(cosine)
    if theta > dt(0.000001):
        w_hat = theta * (R - R.T) / (dt(2) * sine)
        w = np.array([w_hat[2, 1], w_hat[0, 2], w_hat[1, 0]], dtype=dt)
        s = _skew(w, dt) / theta
        V = np.eye(3, dtype=dt) + s * (dt(1) - cosine) / theta + (s @ s) * (theta - sine) / theta
    return np.concatenate([_inv3(V) @ Vt, w])


def adjoint_se3(T):
    dt = T.dtype.type
    R = T[:3, :3]
    A = np.zeros((6, 6), dtype=T.dtype)
    A[:3, :3] = R
    A[:3, 3:] = _skew(T[:3, 3], dt) @ R
    A[3:, 3:] = R
    return A


def det(A, dt=LD):
    """Determinant by LU with partial pivoting (Matrix6d::determinant()); an exactly zero pivot column gives exactly 0."""
    A = np.array(A, dtype=dt)
    n = len(A)
    d = dt(1)
    with np.errstate(all="ignore"):
        for k in range(n):
            p = k + int(np.argmax(np.abs(A[k:, k]))) if not np.isnan(A[k:, k]).any() else k
            if p != k:
                A[[k, p]] = A[[p, k]]
                d = -d
            piv = A[k, k]
            d = d * piv
            if piv == 0:
                return dt(0)
            for i in range(k + 1, n):
                A[i, k + 1:] -= (A[i, k] / piv) * A[k, k + 1:]
    return d


def update(state, T, cov, status, prm, dt=LD):
    """state: dict as initial_state() (doubles); T [4, 4], cov [6, 6], status: the stream's pose result; prm: dict(keyframes,
    min_entropy_ratio, max_kf_t_dist, max_kf_r_dist).  Returns (new state, record, terms): both in `dt`, nothing rounded; terms = which
    operands of the decision's OR were true (empty with keyframes off)."""
    Tfw = np.asarray(state["Tfw"], dtype=dt).reshape(4, 4)
    Tcov = np.asarray(state["Tfw_cov"], dtype=dt).reshape(6, 6)
    s = dict(state)
    if status == 0:  # :372-381
        DT = np.asarray(T, dtype=dt).reshape(4, 4)
        DC = np.asarray(cov, dtype=dt).reshape(6, 6)
        A = adjoint_se3(Tfw)
        with np.errstate(invalid="ignore"):
            s["Tfw_cov"] = Tcov + A @ DC @ A.T            # unccomp_se3(prev Tfw, prev Tfw_cov, DT_cov)
        s["Tfw"] = expmap_se3(logmap_se3(Tfw @ DT, dt), dt)  # :377
    else:  # :382-391
        DT, DC = np.eye(4, dtype=dt), np.zeros((6, 6), dtype=dt)
        s["Tfw"], s["Tfw_cov"] = Tfw, Tcov
    s["n_frames"] = state["n_frames"] + 1
    rec = dict(Tfw=s["Tfw"], Tfw_cov=s["Tfw_cov"], entropy_ratio=dt(0), t=dt(0), r=dt(0), new_kf=0, frame=s["n_frames"])
    terms = set()
    if prm["keyframes"]:
        c0 = dt(3) * (dt(1) + np.log(dt(2) * np.arccos(dt(-1))))
        ent = dt(state["entropy_first_prevKF"])
        with np.errstate(all="ignore"):
            if state["prev_f_iskf"]:  # :1140-1153
                d0 = det(DC, dt)
                ent = c0 + dt(0.5) * np.log(d0) if d0 != 0 else dt(ENTROPY_OF_SINGULAR)
            Tk = np.asarray(state["T_prevKF"], dtype=dt).reshape(4, 4)
            dX = logmap_se3(inverse_se3(s["Tfw"]) @ Tk, dt)  # :1156-1159
            t = np.sqrt(dX[:3] @ dX[:3])
            r = np.sqrt(dX[3:] @ dX[3:]) * dt(180) / dt(CV_PI)
            Ai = adjoint_se3(inverse_se3(DT))
            Ak = adjoint_se3(Tk)
            acc = np.asarray(state["cov_prevKF_currF"], dtype=dt).reshape(6, 6) + Ak @ (Ai @ DC @ Ai.T) @ Ak.T  # :1162-1166
            ratio = (c0 + dt(0.5) * np.log(det(acc, dt))) / ent
        if ratio < dt(prm["min_entropy_ratio"]): terms.add("entropy")
        if np.isnan(ratio): terms.add("nan")
        if np.isinf(ratio): terms.add("inf")
        if not np.any(DC != 0) and np.array_equal(DT, np.eye(4)): terms.add("failed")
        if t > dt(prm["max_kf_t_dist"]): terms.add("t")
        if r > dt(prm["max_kf_r_dist"]): terms.add("r")
        if state["N_prevKF_currF"] > 10: terms.add("count")
        rec.update(entropy_ratio=ratio, t=t, r=r, new_kf=1 if terms else 0)
        s.update(prev_f_iskf=0, entropy_first_prevKF=ent, cov_prevKF_currF=acc)
        if terms:  # currFrameIsKF
            s.update(Tfw=np.eye(4, dtype=dt), Tfw_cov=np.eye(6, dtype=dt), T_prevKF=np.eye(4, dtype=dt),
                     cov_prevKF_currF=np.zeros((6, 6), dtype=dt), prev_f_iskf=1, N_prevKF_currF=0, n_keyframes=state["n_keyframes"] + 1)
        else:
            s["N_prevKF_currF"] = state["N_prevKF_currF"] + 1
    return s, rec, terms


def fields_of(state, rec):
    """The floating-point fields one update is judged by (FIELDS), flat."""
    out = {k: np.asarray(rec[k]).reshape(-1) for k in ("Tfw", "Tfw_cov", "entropy_ratio", "t", "r")}
    out["entropy_first_prevKF"] = np.asarray(state["entropy_first_prevKF"]).reshape(-1)
    out["cov_prevKF_currF"] = np.asarray(state["cov_prevKF_currF"]).reshape(-1)
    return out


def rounded(state):
    """The state as doubles (what a device or host statement can hold)."""
    out = {}
    for k, v in state.items():
        out[k] = int(v) if k in ("prev_f_iskf", "N_prevKF_currF", "n_frames", "n_keyframes") else np.asarray(v, dtype=np.float64)
    out["entropy_first_prevKF"] = float(out["entropy_first_prevKF"])
    return out
