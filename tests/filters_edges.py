"""Shared by tests/test_filters_edges_cpu.py and tests/test_gpu_filters_edges.py (not a test module): the filter inputs at which the device code of
hnet_filters takes paths the benign inputs of tests/test_gpu_filters.py never reach, and the numpy restatements that qualify them.

A. innovation covariances S that are singular bit for bit.  With k_net_cov = 0 a session's S is P[SEL, SEL] itself, and a session stepped without IMU
   readings passes through the propagation unchanged, so the matrices below reach hnet_ekf::invert as written.  They hold zeros and powers of two only:
   every intermediate of the elimination is exact in IEEE arithmetic and host and device meet the zero pivot by construction.
   Out of scope: a singular S at an iteration later than 0.  A posterior is never exactly rank deficient, so it cannot be constructed and is not faked.
   Dropped: a singular session with real IMU intervals before the update.  The zero offset block does not stay zero through F P F^T: the offset rows of F
   couple to p, q, v and bg (Propagator.cpp:298-301), so one interval fills it (test_filters_edges_cpu.py asserts that this is so).
B. well conditioned S whose partial pivoting swaps rows: diagonal 4^i 2^-20 (permuted per session), correlations 0.9.
C. one table of sessions at the edges of the propagation's domain (EDGE_CASES).

gauss_jordan() restates hnet_ekf::invert's pivot search and elimination; it only qualifies inputs (which column is singular, which columns swap)."""
import ctypes as C

import numpy as np

SEL = [15 + 3 * (j // 2) + j % 2 for j in range(8)]           # state rows 15 16 18 19 21 22 24 25: (x, y) of the four corners
F_PIX = 159.5
T_FRAME = 1.0 + 0.1 * 11                                       # the latest frame of test_gpu_filters._setup's 12 pushes: the reference gate is open


def gauss_jordan(S):
    """hnet_ekf::invert on a copy of S -> (inverse or None, the columns whose pivot row was swapped, the column of the zero pivot or None)"""
    a = np.array(S, float)
    n = len(a)
    inv = np.eye(n)
    swaps = []
    for col in range(n):
        piv = col
        for r in range(col + 1, n):
            if abs(a[r, col]) > abs(a[piv, col]):
                piv = r
        if a[piv, col] == 0.0:
            return None, swaps, col
        if piv != col:
            a[[col, piv]] = a[[piv, col]]
            inv[[col, piv]] = inv[[piv, col]]
            swaps.append(col)
        d = 1.0 / a[col, col]
        a[col] *= d
        inv[col] *= d
        for r in range(n):
            f = a[r, col]
            if r != col and f != 0.0:
                a[r] -= f * a[col]
                inv[r] -= f * inv[col]
    return inv, swaps, None


def s_matrix(cov, net72, k_net_cov):
    """S as hnet_ekf::update forms it from a covariance [27, 27] and a packed network record [72] (mean 8 | cov 64), in its operation order"""
    c = np.asarray(net72, np.float32)[8:].astype(np.float64).reshape(8, 8)
    return np.asarray(cov, float)[np.ix_(SEL, SEL)] + k_net_cov * c / (F_PIX * F_PIX)


def net_cov_is_pd(net72):
    c = np.asarray(net72, np.float32)[8:].astype(np.float64).reshape(8, 8)
    return bool(np.linalg.eigvalsh(0.5 * (c + c.T)).min() > 0.0)


# ---- A ----
def _diag_with_zero(at):
    s = np.eye(8) * 2.0 ** -10
    s[at, at] = 0.0
    return s


def _block_45():
    s = np.eye(8) * 2.0 ** -10
    s[4:6, 4:6] = 2.0 ** -10                                   # 2^-10 [[1, 1], [1, 1]]: column 5 is zero after the one, exact, elimination of column 4
    return s


SINGULAR_CASES = [("all_zero", np.zeros((8, 8)), 0), ("diag_zero_at_3", _diag_with_zero(3), 3), ("diag_zero_at_7", _diag_with_zero(7), 7),
                  ("block_45", _block_45(), 5)]               # (name, P[SEL, SEL], the column where invert meets the zero pivot)


def imu_block(rng):
    """the usual SPD covariance of the 15 IMU states (test_gpu_filters._state's a a^T + 1e-4 I)"""
    a = rng.standard_normal((15, 15)) * 0.01
    return a @ a.T + np.eye(15) * 1e-4


def singular_state(base, rng, s8):
    """base (a FILTER_STATE_DTYPE record array of one state) with the covariance of A: imu_block, P[SEL, SEL] = s8, zero elsewhere"""
    st = base.copy()
    cov = np.zeros((27, 27))
    cov[:15, :15] = imu_block(rng)
    cov[np.ix_(SEL, SEL)] = s8
    st["cov"] = cov
    return st


def expected_after_singular(st, t_frame):
    """what a step whose first update finds S singular leaves of a state that no IMU interval moved: t, State::reset_4pt_offset, nothing else"""
    out = st.copy()
    out["t"] = t_frame
    out["offset"] = 0.0
    cov = out["cov"][0].copy()
    cov[15:, :] = 0.0
    cov[:, 15:] = 0.0
    out["cov"] = cov
    return out


# ---- B ----
# the diagonal's exponents i of 4^i 2^-20 by position, one row per session; rows 0 - 3 run with k_net_cov = 0, rows 4 - 7 with the default.  Chosen
# (test_filters_edges_cpu.py asserts it) so that rows 0 - 3 swap in at least 5 columns each and cover 7 distinct columns alone, and that rows 4 - 7
# swap in at least 3 columns with a network covariance like the synthetic weights' (about the identity, in px^2, which under the default k_net_cov
# outweighs the five smallest diagonal entries) at 0.4 to 2.5 times its size.
PIVOT_PERMS = [(2, 7, 1, 6, 5, 3, 0, 4), (5, 4, 2, 0, 7, 6, 3, 1), (5, 3, 1, 7, 2, 6, 4, 0), (4, 7, 1, 3, 0, 2, 6, 5),
               (3, 4, 2, 1, 5, 0, 6, 7), (3, 2, 0, 4, 1, 5, 6, 7), (2, 0, 4, 1, 5, 6, 3, 7), (1, 0, 3, 2, 4, 5, 6, 7)]
PIVOT_K0 = (0, 1, 2, 3)
MIN_SWAPS, MIN_SWAP_COLUMNS = 3, 5


def pivot_s8(perm):
    d = np.array([4.0 ** i * 2.0 ** -20 for i in perm])
    s = 0.9 * np.sqrt(np.outer(d, d))
    s[np.diag_indices(8)] = d
    return s


def pivot_state(base, rng, s8):
    """base with an SPD covariance whose P[SEL, SEL] is s8 to the bit: imu_block, an offset block of s8 and 1e-6 on the four z components, and a cross
    block 0.2 La G Lo^T with |G|_2 = 1 (La, Lo the Cholesky factors), which leaves the Schur complement La (I - G G^T / 25) La^T positive definite"""
    st = base.copy()
    a = imu_block(rng)
    o = np.eye(12) * 1e-6
    idx = [s - 15 for s in SEL]
    o[np.ix_(idx, idx)] = s8
    g = rng.standard_normal((15, 12))
    g /= np.linalg.norm(g, 2)
    b = 0.2 * np.linalg.cholesky(a) @ g @ np.linalg.cholesky(o).T
    cov = np.zeros((27, 27))
    cov[:15, :15], cov[15:, 15:], cov[:15, 15:], cov[15:, :15] = a, o, b, b.T
    cov[np.ix_(SEL, SEL)] = s8
    st["cov"] = cov
    return st


# ---- the two scales a covariance difference is stated in ----
def cov_dev_max(dev, want):
    """|dev - want|max / |want|max: the scale of test_gpu_filters._close"""
    dev, want = np.asarray(dev, float), np.asarray(want, float)
    return float(np.abs(dev - want).max() / np.abs(want).max())


def cov_dev_corr(dev, want):
    """max |dev - want|_ij / sqrt(want_ii want_jj) over the entries whose two diagonals are positive: a wrong small block beside a large one shows here"""
    dev, want = np.asarray(dev, float), np.asarray(want, float)
    d = np.diag(want)
    ok = d > 0
    if not ok.any():
        return 0.0
    sc = np.sqrt(np.outer(d[ok], d[ok]))
    return float((np.abs(dev - want)[np.ix_(ok, ok)] / sc).max())


def mean_dev(dev, want):
    """the largest |dev - want| / max(1, |want|max) over t and the mean's fields (test_gpu_filters._close's measure)"""
    worst = 0.0
    for f in ("t", "p", "q", "v", "ba", "bg", "offset"):
        d, w = np.asarray(dev[f], float), np.asarray(want[f], float)
        worst = max(worst, float(np.abs(d - w).max() / max(1.0, np.abs(w).max())))
    return worst


# ---- C ----
# One session per row.  Unless a row says otherwise: test_gpu_filters._state and _params (attitude within 0.05 of identity), 16 intervals of 2 ms
# with rates of 0.3 rad/s, a window whose ends fall between readings (both are interpolated), gravity 9.81.
#   rate   ("bias", w): every reading's wm is bg + w (a 3-vector, or a length along the camera's optical axis), so the corrected rate is w exactly
#   exact  the readings sit on the state's time and on the frame's (cam_imu_dt 0): no interpolation, the corrected rate of every interval is `rate`
#   dts    the readings' spacing, interval by interval
# The 35 rad/s cases turn about the camera's optical axis: about another axis the explicit Euler step of a corner's normalised coordinate
# (x' = w (1 + x^2)) overflows within the window on host and device alike, and nothing could be compared.
EDGE_CASES = [
    dict(id="zero_rate_avg1", rate=("bias", (0.0, 0.0, 0.0)), exact=True, imu_avg=1),
    dict(id="zero_rate_avg0", rate=("bias", (0.0, 0.0, 0.0)), exact=True, imu_avg=0),
    dict(id="angle_1e-13", rate=("bias", (3e-11, -4e-11, 0.0)), exact=True),                  # |w| dt = 5e-11 x 2e-3: jr_theta's n < 1e-12 branch
    dict(id="angle_1e-11", rate=("bias", (3e-9, -4e-9, 0.0)), exact=True),                    # the other side of it
    dict(id="rate_35_dt_5ms", rate=("bias", 35.0), dts=[0.005] * 16),
    dict(id="rate_35_gap_100ms", rate=("bias", 35.0), dts=[0.005] * 3 + [0.1] + [0.005] * 3),  # one interval of 3.5 rad
    dict(id="dt_1e-9", dts=[0.005, 1e-9] * 8),
    dict(id="q_w_negative", q=(-0.8, 0.3, -0.4, 0.33)),
    dict(id="half_turn_x", q=(0.0, 1.0, 0.0, 0.0), rate=("bias", (1.5, 1.2, -1.0))),
    dict(id="half_turn_y", q=(0.0, 0.0, 1.0, 0.0), rate=("bias", (1.5, 1.2, -1.0))),
    dict(id="half_turn_z", q=(0.0, 0.0, 0.0, 1.0), rate=("bias", (1.5, 1.2, -1.0))),
    dict(id="q_random", q="random"),
    dict(id="gravity_9.7803", gravity_mag=9.7803),
    dict(id="gravity_1.62", gravity_mag=1.62),
    dict(id="cam_imu_dt_launch", cam_imu_dt=-0.0148489),                                        # uzhfpv.launch:43
    dict(id="window_400", dts=[0.002] * 400),
    dict(id="cov_12_orders", cov="span"),                                                       # 1e-12 on bg, 1 on p
]
EDGE_IDS = [c["id"] for c in EDGE_CASES]
PREFIX = 520                                                   # readings before every window: a ring of 512 has wrapped when the window is fed
RING = 512
R3_MARGIN = 1e-6                                               # quat_apply_rotvec flips the sign at r[3] < 0: device and host may round r[3] differently at zero
PREDICT_IDS = ("zero_rate_avg1", "zero_rate_avg0", "rate_35_dt_5ms", "rate_35_gap_100ms")


def _span_cov(rng):
    a = rng.standard_normal((27, 40))
    c = a @ a.T
    c /= np.sqrt(np.outer(np.diag(c), np.diag(c)))
    c = 0.5 * np.eye(27) + 0.5 * c                             # a correlation matrix, eigenvalues >= 0.5
    s = np.sqrt(np.repeat([1.0, 1e-4, 1e-2, 1e-6, 1e-12, 1e-4, 1e-4, 1e-4, 1e-4], 3))
    return c * np.outer(s, s)


def edge_sessions(t_frame=T_FRAME):
    """-> one dict per row of EDGE_CASES: id, st (the state, FILTER_STATE_DTYPE [1]), p (FilterParams), imu (IMU_DTYPE: PREFIX older readings, the
    window's, one past the frame), n_int (the intervals hnet_ekf::select_imu_readings gives the window).  Deterministic."""
    import test_gpu_filters as tg
    from cuahn_vio_amd import _capi
    from cuahn_vio_amd.homography_net import HnetFilters
    out = []
    for k, case in enumerate(EDGE_CASES):
        rng = np.random.default_rng(900 + k)
        p = tg._params(HnetFilters, rng, k)
        p.imu_avg = case.get("imu_avg", 1)
        p.cam_imu_dt = 0.0 if case.get("exact") else case.get("cam_imu_dt", p.cam_imu_dt)
        p.gravity_mag = case.get("gravity_mag", p.gravity_mag)
        dts = np.array(case.get("dts", [0.002] * 16))
        exact = bool(case.get("exact"))
        span = float(dts.sum()) + (0.0 if exact else 0.0004)
        st = tg._state(_capi, rng, t_frame - span)
        if case.get("q") == "random":
            q = np.random.default_rng(2).standard_normal(4)                # z < 0: the first flip is the input's
            st["q"] = q / np.linalg.norm(q)
        elif "q" in case:
            st["q"] = np.array(case["q"]) / np.linalg.norm(case["q"])
        if case.get("cov") == "span":
            st["cov"] = _span_cov(rng)
        t0 = float(st["t"][0]) + p.cam_imu_dt                   # the window's start on the IMU clock
        if exact:                                              # readings on the window's two ends
            ts = t0 + np.concatenate([[0.0], np.cumsum(dts)])
            ts[-1] = t_frame
            ts = np.concatenate([ts, [t_frame + dts[-1]]])
        else:                                                  # the ends fall inside the first and the last pair
            ts = t0 - 0.35 * min(dts[0], 0.002) + np.concatenate([[0.0], np.cumsum(dts), [dts.sum() + 0.002]])
        ts = np.concatenate([ts[0] - 0.002 * np.arange(PREFIX, 0, -1), ts])
        r = np.zeros(len(ts), _capi.IMU_DTYPE)
        r["t"] = ts
        r["am"] = rng.standard_normal((len(ts), 3)) * 0.5 + [0, 0, 9.81]
        r["wm"] = rng.standard_normal((len(ts), 3)) * 0.3
        if "rate" in case:
            w = case["rate"][1]
            if np.isscalar(w):                                 # along the optical axis: the camera's z in the IMU frame is row 2 of c_R_i
                axis = np.array(p.c_R_i[6:9])
                w = w * axis / np.linalg.norm(axis)
            r["wm"] = st["bg"][0] + np.asarray(w, float)
        out.append(dict(id=case["id"], st=st, p=p, imu=r, n_int=len(dts) + (0 if exact else 1), exact=exact))
    return out


def trace(ref, sess, t_frame=T_FRAME):
    """filters_ref's ref_propagate_trace on a session of edge_sessions -> (state after the propagation, q after every interval [n, 4], largest |w| dt)"""
    s = sess["st"].copy()
    r = np.ascontiguousarray(sess["imu"])
    q = np.zeros((len(r) + 1, 4))
    ang = C.c_double(0.0)
    n = ref.ref_propagate_trace(C.c_void_p(s.ctypes.data), C.byref(sess["p"]), C.c_double(t_frame), C.c_void_p(r.ctypes.data), len(r),
                                C.c_void_p(q.ctypes.data), C.byref(ang))
    assert n >= 0
    return s, q[:n], ang.value
