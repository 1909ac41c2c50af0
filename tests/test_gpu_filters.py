"""hnet_filters (include/hnet.h): the per-frame filter work of VioManager.cpp:188-275 for many sessions on the device.  A step must equal the host
reference include/hnet_ekf.h (propagate_with_imu + iterated_update, tests/cpp/filters_ref.cpp) fed with the step's own network outputs, chain
over a replayed flight like the host loop of INTEGRATION.md §6 around a second sessions object, honour the reference's gate and reset, leave
unlisted sessions and failed calls without a trace, and run at full capacity."""
import ctypes as C
import os
import subprocess
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL_MEAN, TOL_COV = 1e-10, 1e-10


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("filters_ref") / "filters_ref.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-shared", "-fPIC", "-pthread", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "filters_ref.cpp"), "-o", so], check=True)
    return C.CDLL(so)


def _mods():
    from cuahn_vio_amd import _capi
    from cuahn_vio_amd.homography_net import HnetEngine, HnetFilters, HnetSessions
    return _capi, HnetEngine, HnetSessions, HnetFilters


def _rot(axis_angle):
    a = np.asarray(axis_angle, float)
    th = np.linalg.norm(a)
    if th == 0:
        return np.eye(3)
    k = a / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def _params(HnetFilters, rng, i):
    p = HnetFilters.default_params()
    R = _rot(rng.standard_normal(3) * 0.05) @ np.array(p.c_R_i).reshape(3, 3)
    for k in range(9):
        p.c_R_i[k] = R.reshape(-1)[k]
    for k in range(3):
        p.i_t_i2c[k] += rng.standard_normal() * 0.01
    p.imu_avg = 0 if i % 5 == 4 else 1
    p.cam_imu_dt = 0.001 * (i % 3)
    return p


def _state(_capi, rng, t):
    st = np.zeros(1, _capi.FILTER_STATE_DTYPE)
    st["t"] = t
    q = np.array([1.0, 0, 0, 0]) + rng.standard_normal(4) * 0.05
    st["q"] = q / np.linalg.norm(q)
    st["p"] = [0.1, -0.05, -1.2] + rng.standard_normal(3) * 0.05
    st["v"] = rng.standard_normal(3) * 0.4
    st["ba"] = rng.standard_normal(3) * 0.05
    st["bg"] = rng.standard_normal(3) * 0.005
    st["offset"] = rng.standard_normal((4, 3)) * 0.005
    a = rng.standard_normal((27, 27)) * 0.01
    st["cov"] = a @ a.T + np.eye(27) * 1e-4
    return st


def _imu(rng, t0, n_int, dt=0.002):
    """n_int intervals of dt inside [t0, t0 + n_int dt] plus one reading either side; n_int = 0: no readings"""
    if n_int == 0:
        return np.zeros(0, np.dtype([("t", "<f8"), ("wm", "<f8", 3), ("am", "<f8", 3)]))
    ts = t0 - 0.0007 + dt * np.arange(n_int + 2)
    r = np.zeros(len(ts), np.dtype([("t", "<f8"), ("wm", "<f8", 3), ("am", "<f8", 3)]))
    r["t"] = ts
    r["wm"] = rng.standard_normal((len(ts), 3)) * 0.3
    r["am"] = rng.standard_normal((len(ts), 3)) * 0.5 + [0, 0, 9.81]
    return r


def _frames(rng, n):
    base = rng.integers(0, 256, (224, 320), dtype=np.uint8)
    return np.stack([np.roll(base, (i % 7) - 3, axis=1) for i in range(n)])


def _ref_step(ref, st, p, t_frame, imu, iters, net, gate):
    """filters_ref from the same starting state with the step's network outputs net [iters][72]"""
    s = st.copy()
    r = np.ascontiguousarray(imu)
    k = ref.ref_propagate_with_imu(C.c_void_p(s.ctypes.data), C.byref(p), C.c_double(t_frame), C.c_void_p(r.ctypes.data), len(r))
    assert k >= 0
    nn = np.ascontiguousarray(net, dtype=np.float32)
    u = ref.ref_iterated_update(C.c_void_p(s.ctypes.data), C.byref(p), iters, C.c_void_p(nn.ctypes.data), int(gate))
    return s, u


def _close(dev, want):
    for f in ("t", "p", "q", "v", "ba", "bg", "offset"):
        d, w = np.asarray(dev[f], float), np.asarray(want[f], float)
        assert np.abs(d - w).max() <= TOL_MEAN * max(1.0, np.abs(w).max()), (f, d, w)
    dc, wc = np.asarray(dev["cov"]), np.asarray(want["cov"])
    assert np.abs(dc - wc).max() <= TOL_COV * np.abs(wc).max(), np.abs(dc - wc).max() / np.abs(wc).max()


def _setup(blob, n_sess, iters, max_batch=8, frames=12, precision=None, seed=1):
    _capi, HnetEngine, HnetSessions, HnetFilters = _mods()
    kw = {} if precision is None else {"precision": precision}
    e = HnetEngine(blob, variant="prior3", mc_samples=16, dropout_p=0.05, mc_seed=9, max_batch=max_batch, **kw)
    s = HnetSessions(e, n_sess)
    f = HnetFilters(s, iters)
    rng = np.random.default_rng(seed)
    fr = _frames(rng, frames)
    ids = np.arange(n_sess, dtype=np.int32)
    for k in range(frames):
        for b in range(0, n_sess, max_batch):
            sub = ids[b:b + max_batch]
            s.push(sub, np.repeat(fr[k][None], len(sub), 0), t=[1.0 + 0.1 * k] * len(sub))
    return e, s, f


@pytest.mark.parametrize("iters", [1, 3])
def test_step_matches_host_reference(blob, ref, iters):
    _capi, _, _, HnetFilters = _mods()
    e, s, f = _setup(blob, 8, iters)
    rng = np.random.default_rng(10 + iters)
    t_frame = 1.0 + 0.1 * 11                                                   # every session's latest time, 12 images: gated on
    counts = [0, 1, 2, 16, 40, 16, 3, 7]
    ps, sts, imus = [], [], []
    for i in range(8):
        p = _params(HnetFilters, rng, i)
        f.set_params(i, p)
        n_int = counts[i]
        t0 = t_frame - 0.002 * max(n_int, 1) - 0.0004
        st = _state(_capi, rng, t0)
        f.set_state(i, st)
        ps.append(p)
        sts.append(st)
        imus.append(_imu(rng, t0 + p.cam_imu_dt, n_int))
    ids = np.arange(8, dtype=np.int32)
    seq0 = [s.seq(i) for i in ids]
    out, net, upd = f.step(ids, [t_frame] * 8, imus)
    got = f.get_state(ids)
    assert got.tobytes() == out.tobytes()
    assert [s.seq(i) for i in ids] == [q + iters for q in seq0]
    for i in range(8):
        want, u = _ref_step(ref, sts[i], ps[i], t_frame, imus[i], iters, net[:, i, :], gate=1)
        assert upd[i] == u == iters
        _close(got[i], want[0])
        assert np.all(got[i]["offset"] == 0) and np.all(got[i]["cov"][15:, :] == 0) and np.all(got[i]["cov"][:, 15:] == 0)
    # the priors the forwards read: (float)(offset x 159.5) of the state before each update
    pri = f.last_priors(8)
    for i in range(8):
        s0 = sts[i].copy()
        r = np.ascontiguousarray(imus[i])
        ref.ref_propagate_with_imu(C.c_void_p(s0.ctypes.data), C.byref(ps[i]), C.c_double(t_frame), C.c_void_p(r.ctypes.data), len(r))
        p0 = np.zeros(8, np.float32)
        ref.ref_prior(C.c_void_p(s0.ctypes.data), C.c_void_p(p0.ctypes.data))
        assert np.abs(pri[0, i] - p0).max() <= 1e-6 * max(1.0, np.abs(p0).max())
    f.close(); s.close(); e.close()


def _synthetic_imu(fx, rate=500.0):
    """IMU readings at `rate` Hz along the replayed trajectory: body rates from consecutive attitudes, specific force from the position's
    second difference (with gravity), linearly interpolated from the 30 Hz poses"""
    from cuahn_vio_amd import replay
    t, p = fx["t"], fx["p"]
    R = np.stack([replay.quat_to_rot(q) for q in fx["q_xyzw"]])
    w = np.zeros((len(t), 3))
    for k in range(len(t) - 1):
        Rr = R[k].T @ R[k + 1]
        ang = np.arccos(np.clip((np.trace(Rr) - 1) / 2, -1, 1))
        axis = np.array([Rr[2, 1] - Rr[1, 2], Rr[0, 2] - Rr[2, 0], Rr[1, 0] - Rr[0, 1]])
        w[k] = axis / (2 * np.sin(ang)) * ang / (t[k + 1] - t[k]) if ang > 1e-12 else 0
    w[-1] = w[-2]
    v = np.gradient(p, t, axis=0)
    a = np.gradient(v, t, axis=0)
    am = np.einsum("kji,kj->ki", R, a + [0, 0, 9.81])
    ts = np.arange(t[0], t[-1], 1.0 / rate)
    out = np.zeros(len(ts), np.dtype([("t", "<f8"), ("wm", "<f8", 3), ("am", "<f8", 3)]))
    out["t"] = ts
    for j in range(3):
        out["wm"][:, j] = np.interp(ts, t, w[:, j])
        out["am"][:, j] = np.interp(ts, t, am[:, j])
    return out, R, v


def test_chained_replay_matches_host_loop(blob, ref):
    """60 frames of replay_indoor_forward_7 (3 sessions with different biases): device steps vs the INTEGRATION §6 host loop
    (filters_ref propagation + hnet_sessions_infer + hnet_ekf::update) on a second sessions object of the same blob"""
    from cuahn_vio_amd import replay
    _capi, HnetEngine, HnetSessions, HnetFilters = _mods()
    fx = replay.load_fixture("indoor_forward_7")
    imu, R, v = _synthetic_imu(fx)
    iters, K, N = 2, 3, 60
    mk = dict(variant="prior3", mc_samples=16, dropout_p=0.05, mc_seed=3, max_batch=4)
    e1, e2 = HnetEngine(blob, **mk), HnetEngine(blob, **mk)
    s1, s2 = HnetSessions(e1, K), HnetSessions(e2, K)
    f = HnetFilters(s1, iters)
    p = HnetFilters.default_params()
    for j in range(9):
        p.c_R_i[j] = fx["c_R_i"].reshape(-1)[j]
    for j in range(3):
        p.i_t_i2c[j] = fx["i_t_i2c"][j]
    # default measurement scale (k_net_cov 10).  The synthetic weights measure nothing; a small initial IMU covariance keeps their updates from
    # driving the state to non-finite values within 60 frames, while they still move it far from the propagation alone (checked below)
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
        host[k] = st[0]
    params = (_capi.FilterParams * K)(*([p] * K))
    ids = np.arange(K, dtype=np.int32)
    prop_only = host.copy()                                                  # the same flight without any update
    compared = same_prior = 0
    frame0 = replay.render_frame(fx, 0)
    for s in (s1, s2):
        s.push(ids, np.repeat(frame0[None], K, 0), t=[fx["t"][0]] * K)
    for k in range(1, N + 1):
        tk = float(fx["t"][k])
        fr = replay.render_frame(fx, k)
        for s in (s1, s2):
            s.push(ids, np.repeat(fr[None], K, 0), t=[tk] * K)
        win = imu[(imu["t"] > fx["t"][k - 1] - 0.01) & (imu["t"] < tk + 0.01)]
        dev, net, upd = f.step(ids, [tk] * K, [win] * K)
        pri = f.last_priors(K)
        if k == 1:
            with pytest.raises(_capi.HnetError):                             # another n than the last step's is refused
                f.last_priors(K - 1)
        # host loop
        r = np.ascontiguousarray(win)
        for j in range(K):
            assert ref.ref_propagate_with_imu(C.c_void_p(host[j:j + 1].ctypes.data), C.byref(p), C.c_double(tk), C.c_void_p(r.ctypes.data), len(r)) >= 0
            ref.ref_propagate_with_imu(C.c_void_p(prop_only[j:j + 1].ctypes.data), C.byref(p), C.c_double(tk), C.c_void_p(r.ctypes.data), len(r))
        ref.ref_reset_batch(C.c_void_p(prop_only.ctypes.data), K)
        gate = np.array([int(s2.latest_time(j) == tk and s2.image_count(j) > 10) for j in range(K)], np.int32)
        for it in range(iters):
            prior_px = host["offset"][:, :, :2].reshape(K, 8) * 159.5
            prior_cam = np.ascontiguousarray(host["offset"][:, :, :2].reshape(K, 8))
            mean, cov = s2.infer(ids, prior_px)
            if np.array_equal(prior_px.astype(np.float32), pri[it]):
                same_prior += 1
                assert np.array_equal(mean, net[it, :, :8]) and np.array_equal(cov.reshape(K, 64), net[it, :, 8:])
            compared += 1
            ref.ref_update_batch(C.c_void_p(host.ctypes.data), params, K, C.c_void_p(mean.ctypes.data), C.c_void_p(cov.ctypes.data),
                                 C.c_void_p(prior_cam.ctypes.data), C.c_void_p(gate.ctypes.data), int(it != iters - 1), 1)
        ref.ref_reset_batch(C.c_void_p(host.ctypes.data), K)
        assert list(upd) == [iters * int(g) for g in gate]
    assert same_prior >= compared // 2, (same_prior, compared)
    got = f.get_state(ids)
    for j in range(K):
        for fld in ("p", "q", "v", "ba", "bg"):
            assert np.abs(got[j][fld] - host[j][fld]).max() <= 1e-8 * max(1.0, np.abs(host[j][fld]).max()), (j, fld)
        assert np.abs(got[j]["cov"] - host[j]["cov"]).max() <= 1e-8 * np.abs(host[j]["cov"]).max()
    assert [s1.seq(j) for j in ids] == [s2.seq(j) for j in ids] == [N * iters] * K
    moved = max(np.abs(got[j][fld] - prop_only[j][fld]).max() for j in range(K) for fld in ("p", "v", "bg"))
    assert moved > 1e-3, moved                                              # the 1e-8 agreement covers what the updates did
    print(f"chained: {compared} forwards compared, {same_prior} with bitwise-equal priors; updates moved the state by up to {moved:.3g}")
    f.close(); s1.close(); s2.close(); e1.close(); e2.close()


def test_gate_and_reset(blob, ref):
    _capi, _, _, HnetFilters = _mods()
    e, s, f = _setup(blob, 3, 2, frames=6)                                   # 6 images: gated off
    rng = np.random.default_rng(2)
    ids = np.arange(3, dtype=np.int32)
    t_frame = 1.0 + 0.1 * 5
    sts = []
    for i in ids:
        st = _state(_capi, rng, t_frame - 0.02)
        f.set_state(int(i), st)
        sts.append(st)
    imus = [_imu(rng, t_frame - 0.02, 10) for _ in ids]
    out, net, upd = f.step(ids, [t_frame] * 3, imus)
    assert list(upd) == [0, 0, 0] and [s.seq(int(i)) for i in ids] == [2, 2, 2] and np.all(np.isfinite(net))
    p = HnetFilters.default_params()
    for i in ids:
        want, u = _ref_step(ref, sts[i], p, t_frame, imus[i], 2, net[:, i, :], gate=0)
        assert u == 0
        _close(out[i], want[0])
        assert np.all(out[i]["offset"] == 0)
    # enough images, but a t_frame other than the session's latest time: no update either
    fr = _frames(rng, 6)
    for k in range(6):
        s.push(ids, np.repeat(fr[k][None], 3, 0), t=[2.0 + 0.1 * k] * 3)
    assert s.image_count(0) == 12
    _, _, upd = f.step(ids, [2.45] * 3, [_imu(rng, 2.40, 20)] * 3)
    assert list(upd) == [0, 0, 0]
    _, _, upd = f.step(ids, [2.5] * 3, [_imu(rng, 2.45, 20)] * 3)
    assert list(upd) == [2, 2, 2]
    f.close(); s.close(); e.close()


def test_subsets_bookkeeping_and_errors(blob):
    _capi, _, _, HnetFilters = _mods()
    e, s, f = _setup(blob, 6, 1, frames=12)
    rng = np.random.default_rng(6)
    t_frame = 1.0 + 0.1 * 11
    for i in range(6):
        f.set_state(i, _state(_capi, rng, t_frame - 0.03))
    all_ids = np.arange(6, dtype=np.int32)
    before = f.get_state(all_ids)
    sub = np.array([4, 1], np.int32)
    f.step(sub, [t_frame] * 2, [_imu(rng, t_frame - 0.03, 15)] * 2)
    after = f.get_state(all_ids)
    for i in (0, 2, 3, 5):
        assert after[i].tobytes() == before[i].tobytes()
    for i in (1, 4):
        assert after[i].tobytes() != before[i].tobytes()
    assert [s.seq(i) for i in range(6)] == [0, 1, 0, 0, 1, 0]
    # hnet_sessions_infer on the same object continues the same sequence numbers
    s.infer([1], prior=np.zeros((1, 8)))
    assert s.seq(1) == 2

    def snap():
        return f.get_state(all_ids).tobytes(), [s.seq(i) for i in range(6)], [s.image_count(i) for i in range(6)]

    ref_snap = snap()
    bad = [
        (np.array([0, 0], np.int32), [t_frame + 1] * 2, _capi.HnetError),      # repeated id
        (np.array([7], np.int32), [t_frame + 1], _capi.HnetError),             # id out of range
        (np.arange(6, dtype=np.int32).repeat(2)[:9] % 6, [t_frame + 1] * 9, _capi.HnetError),   # n > max_batch
        (np.array([0], np.int32), [t_frame - 1.0], _capi.HnetError),           # t_frame before the state
        (np.array([2], np.int32), [t_frame - 0.03], _capi.HnetError),          # t_frame == state t
    ]
    for ids, tf, exc in bad:
        with pytest.raises(exc):
            f.step(ids, tf, [_imu(rng, tf[0] - 0.01, 3)] * len(ids))
        assert snap() == ref_snap
    s.reset(3)                                                               # one image short
    s.push([3], _frames(rng, 1), t=[5.0])
    ref_snap = snap()
    with pytest.raises(_capi.HnetError) as ei:
        f.step([3], [t_frame + 1], [_imu(rng, t_frame, 3)])
    assert ei.value.status == _capi.ERR_NOT_READY and snap() == ref_snap
    f.close(); s.close(); e.close()


def test_full_capacity(blob, ref):
    _capi, _, _, HnetFilters = _mods()
    B = 256
    e, s, f = _setup(blob, B, 1, max_batch=B, frames=12)
    rng = np.random.default_rng(8)
    t_frame = 1.0 + 0.1 * 11
    ids = np.arange(B, dtype=np.int32)
    sts = [_state(_capi, rng, t_frame - 0.0325) for _ in range(B)]
    for i in range(B):
        f.set_state(i, sts[i])
    imus = [_imu(rng, t_frame - 0.0325, 16) for _ in range(B)]
    out, net, upd = f.step(ids, [t_frame] * B, imus)                          # gated on: t_frame is every session's latest time, 12 images
    assert np.all(upd == 1)
    p = HnetFilters.default_params()
    for i in range(0, B, 17):
        want, u = _ref_step(ref, sts[i], p, t_frame, imus[i], 1, net[:, i, :], gate=1)
        assert u == 1
        _close(out[i], want[0])
    for i in range(B):
        sts[i]["t"] = t_frame
        f.set_state(i, sts[i])
    imus = [_imu(rng, t_frame, 16) for _ in range(B)]
    t2 = t_frame + 0.0325
    t0 = time.perf_counter()
    out, net, upd = f.step(ids, [t2] * B, imus)
    wall = (time.perf_counter() - t0) * 1e3
    tm = f.last_timing()
    assert np.all(np.isfinite(out["cov"])) and np.all(np.isfinite(out["p"])) and np.all(upd == 0)
    for i in range(0, B, 17):
        want, _ = _ref_step(ref, sts[i], p, t2, imus[i], 1, net[:, i, :], gate=0)
        _close(out[i], want[0])
    print(f"full capacity: {B} sessions x 16 intervals: device {tm['device_ms']:.3f} ms, step host {tm['host_ms']:.3f} ms, wall {wall:.3f} ms")
    f.close(); s.close(); e.close()
