"""hnet_filters with innovation records and the NIS gate (include/hnet.h).  The records of a step must equal the host reference
include/hnet_ekf.h (iterated_update_gated through tests/cpp/filters_innov_ref.cpp) fed the step's own network outputs; with no gate set nothing else
may change, bit for bit; the gate must skip exactly the updates the rule names and leave the rest alone; the statistics count each accepted update
once, through a repeated attempt too; and a gated replayed flight must follow the host loop.  Main model prior-3, N = 16."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import test_gpu_filters as tg
import test_sessions_iterative_cpu as ic

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-10                                                                   # the bound of tests/test_gpu_filters.py
NONE, USED, REJECTED, SINGULAR, SKIPPED = range(5)
PREC_BF16X3, PREC_F16X2 = 2, 3
INVALID = 1


def _build(tmp, name):
    so = str(tmp / (name + ".so"))
    subprocess.run(["g++", "-std=c++17", "-O2", "-shared", "-fPIC", "-pthread", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-o", so], check=True)
    return C.CDLL(so)


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("filters_ref"), "filters_ref")


@pytest.fixture(scope="module")
def iref(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("filters_innov_ref"), "filters_innov_ref")


def _host(ref, iref, st, p, t_frame, imu, net, gate, max_nis, priors=False):
    """filters_ref's propagation, then hnet_ekf::iterated_update_gated with the network outputs net [iters][72] -> state, updates, records[, priors]"""
    from cuahn_vio_amd import _capi
    s = np.array(st, dtype=_capi.FILTER_STATE_DTYPE).reshape(1).copy()
    if imu is not None:
        r = np.ascontiguousarray(imu)
        assert ref.ref_propagate_with_imu(C.c_void_p(s.ctypes.data), C.byref(p), C.c_double(t_frame), C.c_void_p(r.ctypes.data), len(r)) >= 0
    nn = np.ascontiguousarray(net, dtype=np.float32)
    rec = np.zeros(len(nn), _capi.INNOVATION_DTYPE)
    pri = np.zeros((len(nn), 8))
    u = iref.innov_ref_iterated_gated(C.c_void_p(s.ctypes.data), C.byref(p), len(nn), C.c_void_p(nn.ctypes.data), int(gate), C.c_double(max_nis),
                                      C.c_void_p(rec.ctypes.data), None, C.c_void_p(pri.ctypes.data))
    return (s, u, rec, pri) if priors else (s, u, rec)


def _rel(dev, want):
    dev, want = np.asarray(dev, float), np.asarray(want, float)
    both_nan = np.isnan(dev) & np.isnan(want)
    d = np.where(both_nan, 0.0, np.abs(dev - want) / np.maximum(1.0, np.abs(want)))
    return float(np.max(d))


def _count(recs):
    """per session: (used, rejected, singular) over records [iters, n]"""
    return [(int((recs["flag"][:, i] == USED).sum()), int((recs["flag"][:, i] == REJECTED).sum()), int((recs["flag"][:, i] == SINGULAR).sum()))
            for i in range(recs.shape[1])]


def _check_stats(f, ids, counts, recs_list):
    """innovation_stats of every listed session equals the flags of all its records so far; reset zeroes them"""
    for k, i in enumerate(ids):
        st = f.innovation_stats(int(i))
        assert (st["used"], st["rejected"], st["singular"]) == tuple(counts[k]), (i, st, counts[k])
        nis = [float(r["nis"][it, k]) for r in recs_list for it in range(r.shape[0]) if r["flag"][it, k] == USED]
        assert st["sum_nis"] == pytest.approx(sum(nis), rel=1e-12, abs=0.0) if nis else st["sum_nis"] == 0.0
        seen = [float(r["nis"][it, k]) for r in recs_list for it in range(r.shape[0]) if r["flag"][it, k] in (USED, REJECTED)]
        assert st["max_nis"] == (max(seen) if seen else 0.0)
        f.reset_innovation_stats(int(i))
        z = f.innovation_stats(int(i))
        assert (z["used"], z["rejected"], z["singular"], z["sum_nis"], z["max_nis"]) == (0, 0, 0, 0.0, 0.0)


def _inputs(_capi, HnetFilters, seed, n, t_frame, counts):
    rng = np.random.default_rng(seed)
    ps, sts, imus = [], [], []
    for i in range(n):
        p = tg._params(HnetFilters, rng, i)
        n_int = counts[i % len(counts)]
        t0 = t_frame - 0.002 * max(n_int, 1) - 0.0004
        ps.append(p)
        sts.append(tg._state(_capi, rng, t0))
        imus.append(tg._imu(rng, t0 + p.cam_imu_dt, n_int))
    return ps, sts, imus


def _load(f, s, ps, sts, seq=None):
    for i in range(len(ps)):
        f.set_params(i, ps[i])
        f.set_state(i, sts[i])
        if seq is not None:
            s.set_seq(i, seq)


@pytest.mark.parametrize("iters", [1, 3])
def test_records_match_host_reference(blob, ref, iref, iters):
    """a. 8 sessions with 12 images and windows of 0 - 40 intervals, a ninth with 3 images (reference gate closed), one step"""
    _capi, _, _, HnetFilters = tg._mods()
    n = 9
    e, s, f = tg._setup(blob, n, iters, max_batch=16)
    t_frame = 1.0 + 0.1 * 11
    rng = np.random.default_rng(3)
    s.reset(8)
    for k in (9, 10, 11):
        s.push([8], tg._frames(rng, 1), t=[1.0 + 0.1 * k])
    assert s.image_count(8) == 3 and s.latest_time(8) == t_frame
    f.enable_innovations()
    ps, sts, imus = _inputs(_capi, HnetFilters, 50 + iters, n, t_frame, [0, 1, 2, 16, 40, 16, 3, 7, 5])
    _load(f, s, ps, sts)
    ids = np.arange(n, dtype=np.int32)
    out, net, upd = f.step(ids, [t_frame] * n, imus)
    recs = f.last_innovations(n)
    worst = {"r": 0.0, "s_diag": 0.0, "nis": 0.0}
    for i in range(n):
        gate = int(i < 8)
        want, u, rec = _host(ref, iref, sts[i], ps[i], t_frame, imus[i], net[:, i, :], gate, 0.0)
        assert upd[i] == u == (iters if gate else 0)
        assert list(recs["flag"][:, i]) == list(rec["flag"]) == [USED if gate else NONE] * iters
        assert list(recs["iteration"][:, i]) == list(rec["iteration"]) == list(range(iters))
        for fld in worst:
            worst[fld] = max(worst[fld], _rel(recs[fld][:, i], rec[fld]))
        tg._close(out[i], want[0])
    assert np.all(recs["nis"][:, :8] > 0) and np.all(np.isfinite(recs["nis"])) and not recs["nis"][:, 8].any() and not recs["r"][:, 8].any()
    print(f"records vs host, iters {iters}: largest difference r {worst['r']:.3e}, s_diag {worst['s_diag']:.3e}, nis {worst['nis']:.3e}; "
          f"NIS range {recs['nis'][:, :8].min():.3g} .. {recs['nis'][:, :8].max():.3g}")
    assert max(worst.values()) <= TOL, worst
    _check_stats(f, ids, _count(recs), [recs])
    with pytest.raises(_capi.HnetError) as ei:                                # another n than the last step's
        f.last_innovations(n - 1)
    assert ei.value.status == INVALID
    f.close(); s.close(); e.close()


def test_off_is_off_step(blob):
    """b. innovations enabled and no gate set: the step's states, priors, network outputs, updates and sequence numbers are those of an object
    without them, bit for bit; and the calls' refusals"""
    _capi, _, _, HnetFilters = tg._mods()
    n, iters = 8, 3
    ea, sa, fa = tg._setup(blob, n, iters)
    eb, sb, fb = tg._setup(blob, n, iters)
    L = _capi.lib()
    assert L.hnet_filters_set_nis_gate(fa._f, 0, C.c_double(20.09)) == INVALID   # before enabling
    rec0 = np.zeros((iters, n), _capi.INNOVATION_DTYPE)
    assert L.hnet_filters_last_innovations(fa._f, n, rec0.ctypes.data) == INVALID and not rec0["flag"].any()
    fa.enable_innovations()
    assert L.hnet_filters_enable_innovations(fa._f) == INVALID                 # once per object
    for bad in (-1.0, float("nan")):
        assert L.hnet_filters_set_nis_gate(fa._f, 0, C.c_double(bad)) == INVALID
    assert L.hnet_filters_set_nis_gate(fa._f, n, C.c_double(20.09)) == INVALID and L.hnet_filters_set_nis_gate(fa._f, -1, C.c_double(20.09)) == INVALID
    fa.set_nis_gate(2, 20.09)
    fa.set_nis_gate(2, 0.0)                                                   # and off again
    t_frame = 1.0 + 0.1 * 11
    ps, sts, imus = _inputs(_capi, HnetFilters, 61, n, t_frame, [0, 1, 2, 16, 40, 16, 3, 7])
    for f, s in ((fa, sa), (fb, sb)):
        _load(f, s, ps, sts, seq=7)
    ids = np.arange(n, dtype=np.int32)
    a, b = fa.step(ids, [t_frame] * n, imus), fb.step(ids, [t_frame] * n, imus)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    assert fa.last_priors(n).tobytes() == fb.last_priors(n).tobytes()
    assert fa.get_state(ids).tobytes() == fb.get_state(ids).tobytes()
    assert [sa.seq(i) for i in ids] == [sb.seq(i) for i in ids] == [7 + iters] * n
    recs = fa.last_innovations(n)
    assert np.all(recs["flag"] == USED) and list(a[2]) == [iters] * n
    assert L.hnet_filters_last_innovations(fb._f, n, rec0.ctypes.data) == INVALID  # the last call ran with innovations off
    _check_stats(fa, ids, _count(recs), [recs])
    for o in (fa, fb, sa, sb, ea, eb):
        o.close()


def test_off_is_off_advance(blob):
    """b. the same for hnet_filters_advance on rings of 64 readings that wrap (the set-up of test_feed_equals_step, 3 ticks)"""
    _capi, _, _, HnetFilters = tg._mods()
    iters = 3
    ea, sa, fa = tg._setup(blob, 8, iters)
    eb, sb, fb = tg._setup(blob, 8, iters)
    fa.enable_innovations()
    fa.enable_feed(64)
    fb.enable_feed(64)
    rng = np.random.default_rng(23)
    counts = [0, 1, 2, 16, 40, 16, 3, 7]
    ids = np.arange(8, dtype=np.int32)
    t_frame = np.full(8, 1.0 + 0.1 * 11)
    ps, hist, fed = [], [], [0] * 8
    for i in range(8):
        p = tg._params(HnetFilters, rng, i)
        st = tg._state(_capi, rng, t_frame[i])
        for f in (fa, fb):
            f.set_params(i, p)
            f.set_state(i, st)
        ps.append(p)
        ts = t_frame[i] + p.cam_imu_dt - 0.0007 + 0.002 * np.arange(3 * 42 + 4)
        r = np.zeros(len(ts), _capi.IMU_DTYPE)
        r["t"], r["wm"], r["am"] = ts, rng.standard_normal((len(ts), 3)) * 0.3, rng.standard_normal((len(ts), 3)) * 0.5 + [0, 0, 9.81]
        hist.append(r)
    fr = tg._frames(rng, 3)
    all_recs = []
    for tick in range(3):
        t_frame = t_frame + 0.002 * np.maximum(counts, 0.1) + 0.0004
        for s in (sa, sb):
            s.push(ids, np.repeat(fr[tick][None], 8, 0), t=list(t_frame))
        chunks = []
        for i in range(8):
            upto = int(np.searchsorted(hist[i]["t"], t_frame[i] + ps[i].cam_imu_dt, side="right")) + 1
            chunks.append(hist[i][fed[i]:upto])
            fed[i] = upto
        for f in (fa, fb):
            f.feed_imu(ids, chunks)
        a, b = fa.advance(ids), fb.advance(ids)
        assert list(a[3]) == [_capi.ADV_STEPPED] * 8 and list(a[2]) == [iters] * 8
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)), tick
        assert fa.last_priors(8).tobytes() == fb.last_priors(8).tobytes()
        assert fa.get_state(ids).tobytes() == fb.get_state(ids).tobytes()
        assert [sa.seq(i) for i in ids] == [sb.seq(i) for i in ids]
        recs = fa.last_innovations(8)
        assert np.all(recs["flag"] == USED) and np.all(recs["nis"] > 0)
        all_recs.append(recs)
    assert max(fed) > 64                                                      # the rings wrapped
    total = [tuple(sum(c[i][k] for c in map(_count, all_recs)) for k in range(3)) for i in range(8)]
    _check_stats(fa, ids, total, all_recs)
    for o in (fa, fb, sa, sb, ea, eb):
        o.close()


LO_GROUP, K_LO = (1, 3, 4, 6), 1000.0                                         # test c's second group of cameras and its multiple of k_net_cov


def test_gate_rejects_half(blob):
    """c. the gate at the midpoint between the 4th and 5th largest iteration-0 NIS of 8 sessions: the 4 above are REJECTED then SKIPPED and end where a
    step with the reference gate closed ends (propagation + reset), the 4 below are untouched by the gate; every forward still runs.

    "Untouched" needs the 4 below to stay under the gate in iterations 1 and 2 as well, and with one k_net_cov for all 8 they do not: an applied update
    shrinks P and with it S, the synthetic network's output hardly follows the moved prior, and the NIS of every session grows from 0.7 - 2.3 at
    iteration 0 to 3.4 - 4.6 later, above any midpoint of the iteration-0 values (then the rule correctly gives USED, REJECTED, SKIPPED).  So the
    sessions are two groups of cameras: 0, 2, 5, 7 weigh the network covariance with the default k_net_cov, 1, 3, 4, 6 with K_LO times it.  All 8 see the
    same images and near priors, so their iteration-0 residuals are alike; S of the second group is larger in the positive-definite order, so its
    iteration-0 NIS is smaller, towards 1 / K_LO of the first group's as k_net_cov C / 159.5^2 takes S over; its gain falls the same way, P and the prior
    hardly move, and its later NIS stays near its first.  That this holds is asserted, not assumed."""
    _capi, _, _, HnetFilters = tg._mods()
    n, iters = 8, 3
    e, s, f = tg._setup(blob, n, iters)
    ec, sc, fc = tg._setup(blob, n, iters, frames=6)                         # 6 images: the reference gate stays closed
    f.enable_innovations()
    t_frame = 1.0 + 0.1 * 11
    ps, sts, imus = _inputs(_capi, HnetFilters, 71, n, t_frame, [0, 1, 2, 16, 40, 16, 3, 7])
    for i in LO_GROUP:
        ps[i].k_net_cov *= K_LO
    ids = np.arange(n, dtype=np.int32)
    _load(f, s, ps, sts, seq=4)
    _load(fc, sc, ps, sts, seq=4)
    ung = f.step(ids, [t_frame] * n, imus)
    rec_u = f.last_innovations(n)
    assert np.all(rec_u["flag"] == USED)
    nis0 = rec_u["nis"][0]
    order = np.sort(nis0)[::-1]
    assert order[3] != order[4], order
    gate = 0.5 * (order[3] + order[4])
    above = nis0 > gate
    assert above.sum() == 4
    print(f"gate: iteration-0 NIS {np.array2string(nis0, precision=4)}, gate {gate:.6g}; later iterations {np.array2string(rec_u['nis'][1:], precision=4)}")
    assert sorted(np.flatnonzero(~above)) == list(LO_GROUP)
    assert rec_u["nis"][:, ~above].max() < gate, "the 4 below must stay below in every iteration, or the rule rejects them later"
    for i in ids:
        f.set_nis_gate(int(i), gate)
    _load(f, s, ps, sts, seq=4)
    got = f.step(ids, [t_frame] * n, imus)
    rec_g = f.last_innovations(n)
    closed = fc.step(ids, [t_frame] * n, imus)
    assert list(closed[2]) == [0] * n
    for i in range(n):
        if above[i]:
            assert list(rec_g["flag"][:, i]) == [REJECTED, SKIPPED, SKIPPED] and got[2][i] == 0
            assert got[0][i].tobytes() == closed[0][i].tobytes()
            assert rec_g["nis"][0, i] == nis0[i] and not rec_g["nis"][1:, i].any()
        else:
            assert list(rec_g["flag"][:, i]) == [USED] * iters and got[2][i] == iters
            assert got[0][i].tobytes() == ung[0][i].tobytes() and rec_g[:, i].tobytes() == rec_u[:, i].tobytes()
    assert got[1][0].tobytes() == ung[1][0].tobytes() and np.all(np.isfinite(got[1]))
    assert [s.seq(int(i)) for i in ids] == [4 + iters] * n                     # the forwards ran for all 8
    assert f.get_state(ids).tobytes() == got[0].tobytes()
    cu, cg = _count(rec_u), _count(rec_g)
    _check_stats(f, ids, [tuple(a + b for a, b in zip(cu[i], cg[i])) for i in range(n)], [rec_u, rec_g])
    for o in (f, fc, s, sc, e, ec):
        o.close()


def test_repair_counts_once(blob):
    """d. an iterative model whose activations overflow the fp16 planes: the step demotes it once and reruns; the statistics count every update once and
    the records are those of fresh objects whose iterative engine runs HNET_PREC_BF16X3 from the start, bit for bit"""
    from cuahn_vio_amd.homography_net import HnetEngine
    _capi, _, _, HnetFilters = tg._mods()
    iters, n = 3, 4
    ov = ic.overflow_iterative_blob()
    t_frame = 1.0 + 0.1 * 11
    ps, sts, imus = _inputs(_capi, HnetFilters, 47, n, t_frame, [16])
    ids = np.arange(n, dtype=np.int32)
    res = []
    for prec in (PREC_F16X2, PREC_BF16X3):
        e, s, f = tg._setup(blob, n, iters, precision=PREC_F16X2)
        ie = HnetEngine(ov, variant="prior1", mc_samples=8, dropout_p=0.1, mc_seed=9, max_batch=8, precision=prec)
        s.set_iterative_model(ie)
        f.enable_innovations()
        for i in ids:
            f.set_nis_gate(int(i), 20.090)
        _load(f, s, ps, sts)
        out, net, upd = f.step(ids, [t_frame] * n, imus)
        recs = f.last_innovations(n)
        assert ie.precision() == PREC_BF16X3 and e.precision() == PREC_F16X2   # (demoted once, the iterative context only)
        assert [s.seq(int(i)) for i in ids] == [iters] * n and np.all(np.isfinite(net))
        cnt = _count(recs)
        assert [c[0] for c in cnt] == [int(u) if u >= 0 else -1 - int(u) for u in upd]
        _check_stats(f, ids, cnt, [recs])
        res.append((out, net, upd, recs))
        for o in (f, s, ie, e):
            o.close()
    same = all(x.tobytes() == y.tobytes() for x, y in zip(res[0], res[1]))
    print(f"repair: flags {res[0][3]['flag'].T.tolist()}, bitwise equal to the fresh BF16X3 step: {same}")
    assert res[0][3].tobytes() == res[1][3].tobytes()
    assert same


def test_chained_replay_with_gate_matches_host_loop(blob, ref, iref):
    """e. 3 sessions x 30 frames of replay_indoor_forward_7, I = 2, a gate at the 99 % quantile: device steps against the host loop, which runs
    hnet_ekf::iterated_update_gated around hnet_sessions_infer on a second sessions object (the prior of forward `it` is the one the header hands its
    network after the first `it` outputs)"""
    from cuahn_vio_amd import replay
    _capi, HnetEngine, HnetSessions, HnetFilters = tg._mods()
    fx = replay.load_fixture("indoor_forward_7")
    imu, R, v = tg._synthetic_imu(fx)
    iters, K, N, GATE = 2, 3, 30, 20.090
    mk = dict(variant="prior3", mc_samples=16, dropout_p=0.05, mc_seed=3, max_batch=4)
    e1, e2 = HnetEngine(blob, **mk), HnetEngine(blob, **mk)
    s1, s2 = HnetSessions(e1, K), HnetSessions(e2, K)
    f = HnetFilters(s1, iters)
    f.enable_innovations()
    p = HnetFilters.default_params()
    for j in range(9):
        p.c_R_i[j] = fx["c_R_i"].reshape(-1)[j]
    for j in range(3):
        p.i_t_i2c[j] = fx["i_t_i2c"][j]
    rng = np.random.default_rng(4)
    host = np.zeros(K, _capi.FILTER_STATE_DTYPE)
    for k in range(K):
        st = np.zeros(1, _capi.FILTER_STATE_DTYPE)
        st["t"] = fx["t"][0]
        qx = fx["q_xyzw"][0]
        st["q"] = [qx[3], qx[0], qx[1], qx[2]]
        st["p"] = R[0].T @ (fx["p"][0] - [0, 0, float(fx["floor_z"])])
        st["v"] = R[0].T @ v[0]
        st["ba"] = rng.standard_normal(3) * 0.02
        st["bg"] = rng.standard_normal(3) * 0.002
        st["cov"] = np.diag(np.r_[np.full(15, 1e-5), np.full(12, 1e-6)])
        f.set_params(k, p)
        f.set_state(k, st[0])
        f.set_nis_gate(k, GATE)
        host[k] = st[0]
    ids = np.arange(K, dtype=np.int32)
    frame0 = replay.render_frame(fx, 0)
    for s in (s1, s2):
        s.push(ids, np.repeat(frame0[None], K, 0), t=[fx["t"][0]] * K)
    forwards = same_prior = 0
    flags = np.zeros(5, int)
    nis_used = []
    for k in range(1, N + 1):
        tk = float(fx["t"][k])
        fr = replay.render_frame(fx, k)
        for s in (s1, s2):
            s.push(ids, np.repeat(fr[None], K, 0), t=[tk] * K)
        win = imu[(imu["t"] > fx["t"][k - 1] - 0.01) & (imu["t"] < tk + 0.01)]
        dev, net, upd = f.step(ids, [tk] * K, [win] * K)
        pri = f.last_priors(K)
        recs = f.last_innovations(K)
        # host loop
        r = np.ascontiguousarray(win)
        for j in range(K):
            assert ref.ref_propagate_with_imu(C.c_void_p(host[j:j + 1].ctypes.data), C.byref(p), C.c_double(tk), C.c_void_p(r.ctypes.data), len(r)) >= 0
        gate = [int(s2.latest_time(j) == tk and s2.image_count(j) > 10) for j in range(K)]
        hnet = np.zeros((iters, K, 72), np.float32)
        for it in range(iters):
            prior_px = np.stack([_host(ref, iref, host[j], p, tk, None, hnet[:, j, :], gate[j], GATE, priors=True)[3][it] for j in range(K)])
            mean, cov = s2.infer(ids, prior_px)
            hnet[it, :, :8], hnet[it, :, 8:] = mean, cov.reshape(K, 64)
            forwards += 1
            same_prior += int(np.array_equal(prior_px.astype(np.float32), pri[it]))
        for j in range(K):
            st, u, rec = _host(ref, iref, host[j], p, tk, None, hnet[:, j, :], gate[j], GATE)
            host[j] = st[0]
            assert list(recs["flag"][:, j]) == list(rec["flag"]), (k, j, recs["flag"][:, j], rec["flag"])
            assert upd[j] == u
            for fl in rec["flag"]:
                flags[fl] += 1
            nis_used += [float(x) for x, fl in zip(rec["nis"], rec["flag"]) if fl == USED]
    print(f"chained with gate: {forwards} forwards, {same_prior} with bitwise-equal priors; flags none {flags[NONE]} used {flags[USED]} "
          f"rejected {flags[REJECTED]} skipped {flags[SKIPPED]} singular {flags[SINGULAR]}; mean NIS of the used {np.mean(nis_used) if nis_used else 0:.4g}")
    got = f.get_state(ids)
    worst = 0.0
    for j in range(K):
        for fld in ("p", "q", "v", "ba", "bg"):
            worst = max(worst, np.abs(got[j][fld] - host[j][fld]).max() / max(1.0, np.abs(host[j][fld]).max()))
        worst = max(worst, np.abs(got[j]["cov"] - host[j]["cov"]).max() / np.abs(host[j]["cov"]).max())
    print(f"chained with gate: largest final state difference {worst:.3e}")
    assert same_prior == forwards, (same_prior, forwards)
    assert worst <= 1e-8, worst
    assert [s1.seq(j) for j in ids] == [s2.seq(j) for j in ids] == [N * iters] * K
    st_sum = [f.innovation_stats(j) for j in range(K)]
    assert sum(x["used"] for x in st_sum) == flags[USED] and sum(x["rejected"] for x in st_sum) == flags[REJECTED]
    f.close(); s1.close(); s2.close(); e1.close(); e2.close()
