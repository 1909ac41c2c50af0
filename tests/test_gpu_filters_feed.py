"""The fed filters (include/hnet.h: hnet_filters_enable_feed / feed_imu / advance): device IMU rings, selection and the static initialiser on the
device, one call that advances every camera that is ready.  A fed tick must equal hnet_filters_step with host-selected windows; the selection must be
hnet_ekf::select_imu_readings on the same history; the initialiser must agree with the host header; a cold start must reach flight like a host loop
built from the header functions and hnet_sessions_infer; calls that do nothing and failed calls leave no trace."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import test_filters_cpu as tc
import test_filters_feed_cpu as fc
import test_gpu_filters as tg

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# The initialiser on the device against the host header on the same readings: the window sums are a 256-lane tree instead of a serial loop.
# Measured over the accepted sessions of test_initialiser_matches_host_header: largest relative difference (in the _close sense) MEASURED_INIT_DIFF;
# the bound is ten times that, and may never exceed 1e-9 (a larger difference means a wrong or badly ordered reduction).
MEASURED_INIT_DIFF = 1.066e-14
INIT_TOL = 10 * MEASURED_INIT_DIFF
assert INIT_TOL <= 1e-9


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("filters_ref") / "filters_ref.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-shared", "-fPIC", "-pthread", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "filters_ref.cpp"), "-o", so], check=True)
    return C.CDLL(so)


@pytest.fixture(scope="module")
def fref(tmp_path_factory):
    return fc.build_ref(str(tmp_path_factory.mktemp("filters_feed_ref") / "filters_feed_ref.so"))


def _engine(blob, max_batch, seed=9):
    _capi, HnetEngine, HnetSessions, HnetFilters = tg._mods()
    return HnetEngine(blob, variant="prior3", mc_samples=16, dropout_p=0.05, mc_seed=seed, max_batch=max_batch)


def _rel_state(dev, want):
    """the largest difference in the sense of test_gpu_filters._close: per field |d - w| / max(1, |w|max), covariance |d - w| / |w|max"""
    worst = 0.0
    for f in ("t", "p", "q", "v", "ba", "bg", "offset"):
        d, w = np.asarray(dev[f], float), np.asarray(want[f], float)
        worst = max(worst, float(np.abs(d - w).max() / max(1.0, np.abs(w).max())))
    dc, wc = np.asarray(dev["cov"]), np.asarray(want["cov"])
    return max(worst, float(np.abs(dc - wc).max() / np.abs(wc).max()))


def _host_select(fref, hist, t0, t1):
    _capi = tg._mods()[0]
    rec = np.ascontiguousarray(hist)
    k = fref.feed_ref_trim_prop(C.c_void_p(rec.ctypes.data), len(rec), C.c_double(rec["t"][-1])) if len(rec) else 0
    rec = np.ascontiguousarray(rec[k:])
    out = np.zeros(len(rec) + 2, _capi.IMU_DTYPE)
    m = fref.feed_ref_select(C.c_void_p(rec.ctypes.data), len(rec), C.c_double(t0), C.c_double(t1), C.c_void_p(out.ctypes.data))
    return out[:m]


def _same_readings(got, want):
    assert len(got) == len(want), (got["t"], want["t"])
    for f in ("t", "wm", "am"):
        if len(want):
            assert np.abs(got[f] - want[f]).max() <= 1e-12 * max(1.0, np.abs(want[f]).max()), f


def _host_propagate(ref, st, p, t_frame, hist, reset=True):
    s = st.copy()
    r = np.ascontiguousarray(hist)
    assert ref.ref_propagate_with_imu(C.c_void_p(s.ctypes.data), C.byref(p), C.c_double(t_frame), C.c_void_p(r.ctypes.data), len(r)) >= 0
    if reset:
        ref.ref_reset_batch(C.c_void_p(s.ctypes.data), 1)
    return s


@pytest.mark.parametrize("iters", [1, 3])
def test_feed_equals_step(blob, ref, fref, iters):
    """8 sessions, 0 - 40 intervals per tick, cam_imu_dt / imu_avg varied, 5 ticks on rings of 64 readings (they wrap): feed_imu + advance on one
    filters object, hnet_filters_step with the window taken from the full history on another"""
    _capi, HnetEngine, HnetSessions, HnetFilters = tg._mods()
    ea, sa, fa = tg._setup(blob, 8, iters)
    eb, sb, fb = tg._setup(blob, 8, iters)
    fa.enable_feed(64)
    rng = np.random.default_rng(20 + iters)
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
        ts = t_frame[i] + p.cam_imu_dt - 0.0007 + 0.002 * np.arange(5 * 42 + 4)        # one stream per session for the whole test
        r = np.zeros(len(ts), _capi.IMU_DTYPE)
        r["t"], r["wm"], r["am"] = ts, rng.standard_normal((len(ts), 3)) * 0.3, rng.standard_normal((len(ts), 3)) * 0.5 + [0, 0, 9.81]
        hist.append(r)
    fr = tg._frames(rng, 6)
    worst, bitwise = 0.0, True
    for tick in range(5):
        t_prev, t_frame = t_frame, t_frame + 0.002 * np.maximum(counts, 0.1) + 0.0004
        for s in (sa, sb):
            s.push(ids, np.repeat(fr[tick][None], 8, 0), t=list(t_frame))
        chunks = []
        for i in range(8):                                                              # hand over what arrived: up to the first reading past the frame
            upto = int(np.searchsorted(hist[i]["t"], t_frame[i] + ps[i].cam_imu_dt, side="right")) + 1
            chunks.append(hist[i][fed[i]:upto])
            fed[i] = upto
        fa.feed_imu(ids, chunks)
        sta, neta, upda, status = fa.advance(ids)
        assert list(status) == [_capi.ADV_STEPPED] * 8
        stb, netb, updb = fb.step(ids, list(t_frame), [hist[i][:fed[i]] for i in range(8)])
        assert list(upda) == list(updb) == [iters] * 8
        for i in range(8):
            tg._close(sta[i], stb[i])
            worst = max(worst, _rel_state(sta[i], stb[i]))
            _same_readings(fa.last_selection(i), _host_select(fref, hist[i][:fed[i]], t_prev[i] + ps[i].cam_imu_dt, t_frame[i] + ps[i].cam_imu_dt))
        pa, pb = fa.last_priors(8), fb.last_priors(8)
        assert np.abs(pa - pb).max() <= 1e-6 * max(1.0, np.abs(pb).max())
        bitwise = bitwise and sta.tobytes() == stb.tobytes() and pa.tobytes() == pb.tobytes() and neta.tobytes() == netb.tobytes()
        # measured on the MI355X: the two paths agree to the bit (the same kernels on the same selected readings; the device's interpolation of the
        # window ends rounds like the host's), so the 1e-10 above is kept only as the message for a first divergence and equality is what is asserted
        assert bitwise, (tick, worst)
        assert fa.get_state(ids).tobytes() == sta.tobytes()
        assert [sa.seq(i) for i in ids] == [sb.seq(i) for i in ids]
    print(f"feed vs step, iters {iters}: largest state difference {worst:.3e}, bitwise equal: {bitwise}")
    for o in (fa, fb, sa, sb, ea, eb):
        o.close()


def test_feed_equals_step_with_every_layer_and_a_propagate_only_session(blob, ref):
    """Everything a step's attempt can contain at once, on both paths: max_batch 4, 4 sessions, 8 samples, 3 IEKF iterations, an iterative model attached,
    innovation and photometric records on.  Sessions 0 - 2 step for three ticks, through hnet_filters_step on one filters object and through feed_imu +
    advance on another; the advance also lists session 3, whose camera restarts before every frame, so it has one image and only propagates: the call's
    tables then are wider (4) than its forwards (3).  Bytes are compared for the stepping sessions, session 3 against the host header's propagation."""
    _capi, HnetEngine, HnetSessions, HnetFilters = tg._mods()
    iters, n = 3, 3
    objs = []
    for _ in range(2):
        e = HnetEngine(blob, variant="prior3", mc_samples=8, dropout_p=0.05, mc_seed=9, max_batch=4)
        ie = HnetEngine(blob, variant="prior1", mc_samples=8, dropout_p=0.1, mc_seed=9, max_batch=4)
        s = HnetSessions(e, 4)
        s.set_iterative_model(ie)
        f = HnetFilters(s, iters)
        f.enable_innovations()
        f.enable_photometric()
        objs.append((e, ie, s, f))
    (ea, ia, sa, fa), (eb, ib, sb, fb) = objs
    fa.enable_feed(64)
    rng = np.random.default_rng(77)
    fr = tg._frames(rng, 15)
    every = np.arange(4, dtype=np.int32)
    ids = every[:n]
    for k in range(12):                                                                 # 12 images each: the reference's gate is open (count > 10)
        for s in (sa, sb):
            s.push(every, np.stack([np.roll(fr[k], 5 * i, axis=0) for i in range(4)]), t=[1.0 + 0.1 * k] * 4)
    counts = [16, 3, 40, 7]
    t_frame = np.full(4, 1.0 + 0.1 * 11)
    ps, hist, fed = [], [], [0] * 4
    for i in range(4):
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
    for tick in range(3):
        t_frame = t_frame + 0.002 * np.array(counts) + 0.0004
        frames = np.stack([np.roll(fr[12 + tick], 5 * i, axis=0) for i in range(4)])
        sa.reset(3)                                                                     # (the filter keeps its state: PROPAGATED, as in test_cold_start_to_flight)
        sa.push(every, frames, t=list(t_frame))
        sb.push(ids, frames[:n], t=list(t_frame[:n]))
        chunks = []
        for i in range(4):
            upto = int(np.searchsorted(hist[i]["t"], t_frame[i] + ps[i].cam_imu_dt, side="right")) + 1
            chunks.append(hist[i][fed[i]:upto])
            fed[i] = upto
        fa.feed_imu(every, chunks)
        before3, seq3 = fa.get_state([3]), sa.seq(3)
        sta, neta, upda, status = fa.advance(every)
        assert list(status) == [_capi.ADV_STEPPED] * n + [_capi.ADV_PROPAGATED]
        stb, netb, updb = fb.step(ids, list(t_frame[:n]), [hist[i][:fed[i]] for i in range(n)])
        assert list(upda[:n]) == list(updb) == [iters] * n and upda[3] == 0
        assert sta[:n].tobytes() == stb.tobytes(), tick
        assert np.ascontiguousarray(neta[:, :n]).tobytes() == netb.tobytes() and np.isfinite(netb).all() and not neta[:, 3].any(), tick
        assert fa.last_priors(n).tobytes() == fb.last_priors(n).tobytes(), tick
        assert fa.last_innovations(n).tobytes() == fb.last_innovations(n).tobytes(), tick
        assert fa.last_photometric(n).tobytes() == fb.last_photometric(n).tobytes(), tick
        assert fa.get_state(every).tobytes() == sta.tobytes()
        assert [sa.seq(i) for i in ids] == [sb.seq(i) for i in ids] and sa.seq(3) == seq3
        assert sta[3]["t"] == t_frame[3]
        tg._close(sta[3], _host_propagate(ref, before3, ps[3], t_frame[3], hist[3][:fed[3]])[0])
    for group in objs:
        for o in reversed(group):
            o.close()


SELECT_CASES = ["inside", "split_both_ends", "reading_on_t1", "reading_on_t0", "imu_slower_than_camera", "all_after_t1", "duplicated_stamps",
                "near_duplicate_at_t0"]


@pytest.mark.parametrize("prefill", [0, 20])
def test_selection_matches_host(blob, fref, prefill):
    """the edge cases of tests/test_filters_cpu.py CASES whose newest reading lies past the frame, one session each in one advance; prefill = 20 puts
    20 older readings into the rings of 32 first, so that every case's window straddles the ring's wrap point"""
    _capi, HnetEngine, HnetSessions, HnetFilters = tg._mods()
    K = len(SELECT_CASES)
    e = _engine(blob, K)
    s = HnetSessions(e, K)
    f = HnetFilters(s, 1)
    f.enable_feed(32)
    rng = np.random.default_rng(5)
    ids = np.arange(K, dtype=np.int32)
    hist, win = [], []
    for i, name in enumerate(SELECT_CASES):
        ts, t0, t1 = tc.CASES[name]
        r = fc.imu_records(tc._readings(ts, np.random.default_rng(len(name))))
        if prefill:
            old = fc.imu_records(tc._readings(-1.0 + 0.01 * np.arange(prefill), rng))
            f.feed_imu([i], [old])
            r = np.concatenate([old, r])
        hist.append(r[-32:])
        win.append((t0, t1))
        st = tg._state(_capi, rng, t0)
        f.set_state(i, st)
    f.feed_imu(ids, [h[-len(tc.CASES[n][0]):] if prefill else h for h, n in zip(hist, SELECT_CASES)])
    s.push(ids, tg._frames(rng, K), t=[w[1] for w in win])
    _, _, _, status = f.advance(ids)
    assert list(status) == [_capi.ADV_PROPAGATED] * K
    for i, name in enumerate(SELECT_CASES):
        want = _host_select(fref, hist[i], *win[i])
        _same_readings(f.last_selection(i), want)
        if not prefill and name == "imu_slower_than_camera":
            assert len(want) == 2
        if not prefill and name == "duplicated_stamps":
            assert len(want) > 2 and np.all(np.diff(want["t"]) >= 1e-12)
    for o in (f, s, e):
        o.close()


def test_initialiser_matches_host_header(blob, ref, fref):
    """16 sessions with the streams of tests/test_filters_feed_cpu.py mixed in one advance: the decisions, and the accepted states against
    hnet_ekf::initialize_with_imu + initialize_cov + propagate_with_imu + reset_4pt_offset on the same readings.  Session 15's frame is older than
    its time0: it keeps the initial state itself."""
    _capi, HnetEngine, HnetSessions, HnetFilters = tg._mods()
    K = 16
    e = _engine(blob, K)
    s = HnetSessions(e, K)
    f = HnetFilters(s, 1)
    f.enable_feed(1024)
    ids = np.arange(K, dtype=np.int32)
    rng = np.random.default_rng(8)
    streams, t_frame, ps = [], [], []
    for i in range(K):
        kind = "still_then_jerk" if i >= 12 else fc.KINDS[i % len(fc.KINDS)]
        r, wait, expect = fc.stream(kind, 100 + i)
        streams.append((fc.imu_records(r), wait, expect))
        f.set_init_params(i, fc.init_params(wait, height=0.1 + 0.05 * i))
        p = tg._params(HnetFilters, rng, i)
        f.set_params(i, p)
        ps.append(p)
        t_frame.append(1.5 if i == 15 else 2.9 - 0.01 * i)
    f.feed_imu(ids, [r for r, _, _ in streams])
    s.push(ids, tg._frames(rng, K), t=t_frame)
    before = f.get_state(ids)
    out, _, _, status = f.advance(ids)
    got = f.get_state(ids)
    worst = 0.0
    for i in range(K):
        rec, wait, expect = streams[i]
        assert status[i] == (_capi.ADV_INITIALIZED if expect else _capi.ADV_WAIT_INIT), (i, status[i])
        assert f.initialized(i) == expect
        if not expect:
            assert got[i].tobytes() == before[i].tobytes() and s.image_count(i) == 0
            continue
        want = fc.c_initialize(fref, rec.view(np.float64).reshape(-1, 7), wait, height=0.1 + 0.05 * i)
        assert want["t"][0] == 2.0 and s.image_count(i) == 1 and s.seq(i) == 0
        if i != 15:
            want = _host_propagate(ref, want, ps[i], t_frame[i], rec)
        assert got[i].tobytes() == out[i].tobytes()
        assert got[i]["t"] == want["t"][0]
        worst = max(worst, _rel_state(got[i], want[0]))
    print(f"initialiser, device vs host header: largest relative difference {worst:.3e} (bound {INIT_TOL:.1e})")
    assert worst <= INIT_TOL, worst
    for o in (f, s, e):
        o.close()


def test_cold_start_to_flight(blob, ref, fref):
    """replay_indoor_forward_7 behind a still IMU prefix with a jerk: three sessions (jerks at different times) go WAIT_INIT ... INITIALIZED, STEPPED
    with the gate opening after image 10, and after 60 frames agree with a host loop built from the header functions and hnet_sessions_infer on a
    second sessions object.  The frame that initialises is image 1 of its session, so the next one is image 2 and steps (the forward runs from the
    second image on, HomographyNet.cpp:155-158); PROPAGATED needs a filter with a state and a session with one image, which here is session 2's
    camera restarting at frame 20 (hnet_sessions_reset on both sessions objects, the filter kept)."""
    from cuahn_vio_amd import replay
    _capi, HnetEngine, HnetSessions, HnetFilters = tg._mods()
    fx = replay.load_fixture("indoor_forward_7")
    flight, R, v = tg._synthetic_imu(fx)
    iters, K, N = 2, 3, 60
    mk = dict(variant="prior3", mc_samples=16, dropout_p=0.05, mc_seed=3, max_batch=4)
    e1, e2 = HnetEngine(blob, **mk), HnetEngine(blob, **mk)
    s1, s2 = HnetSessions(e1, K), HnetSessions(e2, K)
    f = HnetFilters(s1, iters)
    f.enable_feed(4096)
    p = HnetFilters.default_params()
    for j in range(9):
        p.c_R_i[j] = fx["c_R_i"].reshape(-1)[j]
    for j in range(3):
        p.i_t_i2c[j] = fx["i_t_i2c"][j]
    params = (_capi.FilterParams * K)(*([p] * K))
    # the flight starts in the air: init_height is the height above the floor there (the launch file's 0.1 m would put the ground plane inside the flight)
    height = float(fx["p"][0][2] - fx["floor_z"])
    ip = fc.init_params(1, height=height)
    rng = np.random.default_rng(12)
    t0 = float(fx["t"][0])
    imus = []
    for j in range(K):                       # 3 s of a still IMU (the first flight reading held, a little noise), then the flight with a 1 s jerk on top
        ts = np.arange(t0 - 3.0, flight["t"][0] - 1e-9, 0.002)
        pre = np.zeros(len(ts), _capi.IMU_DTYPE)
        pre["t"] = ts
        pre["wm"] = flight["wm"][0] + 0.001 * rng.standard_normal((len(ts), 3))
        pre["am"] = flight["am"][0] + 0.01 * rng.standard_normal((len(ts), 3))
        fl = flight.copy()
        hold = fl["t"] <= t0 + 0.07 * j                              # session j stands still a little longer (the flight alone would start all three at once)
        fl["wm"][hold], fl["am"][hold] = flight["wm"][0], flight["am"][0] + 0.01 * rng.standard_normal((int(hold.sum()), 3))
        t_j = t0 + 0.07 * j + 0.01
        m = (fl["t"] > t_j) & (fl["t"] <= t_j + 1.0)
        fl["am"][m] += 5.0 * rng.standard_normal((int(m.sum()), 3))
        imus.append(np.concatenate([pre, fl]))
        f.set_params(j, p)
        f.set_init_params(j, ip)
    ids = np.arange(K, dtype=np.int32)
    host = np.zeros(K, _capi.FILTER_STATE_DTYPE)
    inited, fed, seen = [False] * K, [0] * K, [[] for _ in range(K)]
    opened = 0
    drift = []
    for k in range(N + 1):
        tk = float(fx["t"][k])
        fr = replay.render_frame(fx, k)
        for s in (s1, s2):
            if k == 20:
                s.reset(2)
            s.push(ids, np.repeat(fr[None], K, 0), t=[tk] * K)
        chunks = []
        for j in range(K):
            upto = int(np.searchsorted(imus[j]["t"], tk, side="right")) + 1
            chunks.append(imus[j][fed[j]:upto])
            fed[j] = upto
        f.feed_imu(ids, chunks)
        dev, net, upd, status = f.advance(ids)
        # host loop (VioManager.cpp:155-275 with the header functions)
        want_status, stepped = [], []
        for j in range(K):
            hist = imus[j][:fed[j]]
            if not inited[j]:
                st = fc.c_initialize(fref, hist.view(np.float64).reshape(-1, 7), 1, height=height)
                if st is None:
                    s2.reset(j)
                    want_status.append(_capi.ADV_WAIT_INIT)
                    continue
                inited[j] = True
                host[j] = _host_propagate(ref, st, p, tk, hist)[0]
                want_status.append(_capi.ADV_INITIALIZED)
            elif s2.image_count(j) < 2:
                host[j] = _host_propagate(ref, host[j:j + 1], p, tk, hist)[0]
                want_status.append(_capi.ADV_PROPAGATED)
            else:
                host[j] = _host_propagate(ref, host[j:j + 1], p, tk, hist, reset=False)[0]
                want_status.append(_capi.ADV_STEPPED)
                stepped.append(j)
        assert list(status) == want_status, (k, list(status), want_status)
        for j in range(K):
            seen[j].append(int(status[j]))
        if stepped:
            sub = np.array(stepped, np.int32)
            hs = np.ascontiguousarray(host[sub])
            gate = np.array([int(s2.latest_time(j) == tk and s2.image_count(j) > 10) for j in sub], np.int32)
            for it in range(iters):
                prior_cam = np.ascontiguousarray(hs["offset"][:, :, :2].reshape(len(sub), 8))
                mean, cov = s2.infer(sub, prior_cam * 159.5)
                ref.ref_update_batch(C.c_void_p(hs.ctypes.data), params, len(sub), C.c_void_p(mean.ctypes.data), C.c_void_p(cov.ctypes.data),
                                     C.c_void_p(prior_cam.ctypes.data), C.c_void_p(gate.ctypes.data), int(it != iters - 1), 1)
            ref.ref_reset_batch(C.c_void_p(hs.ctypes.data), len(sub))
            host[sub] = hs
            assert [int(upd[j]) for j in sub] == [iters * int(g) for g in gate]
            assert [bool(g) for g in gate] == [s1.image_count(j) > 10 for j in sub]          # the gate opens after image 10
            opened += int(gate.sum())
        assert [s1.seq(j) for j in range(K)] == [s2.seq(j) for j in range(K)]
        assert [s1.image_count(j) for j in range(K)] == [s2.image_count(j) for j in range(K)]
        live = [j for j in range(K) if inited[j]]
        if live:
            now = f.get_state(live)
            d = max(float(np.abs(now[i][fld] - host[j][fld]).max() / max(1.0, np.abs(host[j][fld]).max())) for i, j in enumerate(live)
                    for fld in ("p", "q", "v", "ba", "bg"))
            drift.append(d)
    A = _capi
    for j in range(K):
        n_wait = seen[j].index(A.ADV_INITIALIZED)
        assert n_wait >= 1 and seen[j][:n_wait] == [A.ADV_WAIT_INIT] * n_wait
        rest = [A.ADV_STEPPED] * (N - n_wait)
        if j == 2:
            rest[20 - n_wait - 1] = A.ADV_PROPAGATED
        assert seen[j][n_wait + 1:] == rest
    print("cold start, device vs host loop, largest relative difference of the mean per frame:", " ".join(f"{d:.1e}" for d in drift))
    # measured on the MI355X: 5e-15 at the initialisation, at most 6.2e-14 over the 60 frames (default measurement scale, gate open from image 11)
    assert opened > 100
    assert len({seen[j].index(A.ADV_INITIALIZED) for j in range(K)}) > 1          # kinds were mixed within calls
    got = f.get_state(ids)
    for j in range(K):
        assert np.isfinite(got[j]["cov"]).all()
        for fld in ("t", "p", "q", "v", "ba", "bg"):
            assert np.abs(got[j][fld] - host[j][fld]).max() <= 1e-8 * max(1.0, np.abs(host[j][fld]).max()), (j, fld)
    for o in (f, s1, s2, e1, e2):
        o.close()


def _still_stream(_capi, t_from, t_to, rng, dt=0.005):
    ts = np.arange(t_from, t_to + 1e-9, dt)
    r = np.zeros(len(ts), _capi.IMU_DTYPE)
    r["t"], r["wm"], r["am"] = ts, 0.01 * rng.standard_normal((len(ts), 3)), 0.05 * rng.standard_normal((len(ts), 3)) + [0, 0, 9.81]
    return r


def test_bookkeeping(blob, ref, fref):
    _capi, HnetEngine, HnetSessions, HnetFilters = tg._mods()
    A = _capi
    e = _engine(blob, 4)
    s = HnetSessions(e, 6)
    f = HnetFilters(s, 2)
    rng = np.random.default_rng(3)
    fr = tg._frames(rng, 4)
    with pytest.raises(_capi.HnetError):                                           # feed not enabled
        f.feed_imu([0], [_still_stream(_capi, 0.0, 0.1, rng)])
    with pytest.raises(_capi.HnetError):
        f.advance([0])
    f.enable_feed(1024)
    with pytest.raises(_capi.HnetError):                                           # once
        f.enable_feed(1024)
    p = HnetFilters.default_params()
    for i in range(4):
        f.set_state(i, tg._state(_capi, rng, 1.0))
    hist = _still_stream(_capi, 0.9, 1.1051, rng)
    f.feed_imu([0, 1, 2], [hist] * 3)
    # session 0: two frames, readings past the second: STEPPED.  1: one frame: PROPAGATED.  2: a frame the readings do not pass: WAIT_IMU.  3: no frame.
    s.push([0], fr[:1], t=[1.05])
    s.push([0, 1, 2], fr[1:4], t=[1.1, 1.1, 1.2])
    ids = np.arange(4, dtype=np.int32)
    before, seq0 = f.get_state(ids), [s.seq(i) for i in ids]
    out, net, upd, status = f.advance(ids)
    assert list(status) == [A.ADV_STEPPED, A.ADV_PROPAGATED, A.ADV_WAIT_IMU, A.ADV_NO_FRAME]
    after = f.get_state(ids)
    assert [s.seq(i) for i in ids] == [seq0[0] + 2, seq0[1], seq0[2], seq0[3]]    # a PROPAGATED session's sequence number does not advance
    assert after[2].tobytes() == before[2].tobytes() and after[3].tobytes() == before[3].tobytes()
    assert after[0]["t"] == 1.1 and after[1]["t"] == 1.1 and net[:, 1:].any() == False and net[:, 0].any()
    tg._close(after[1], _host_propagate(ref, before[1:2], p, 1.1, hist)[0])
    assert len(f.last_selection(2)) == 0 and len(f.last_selection(1)) > 2
    # the same call again: nothing is pending any more
    seq1 = [s.seq(i) for i in ids]
    _, _, _, status = f.advance(ids)
    assert list(status) == [A.ADV_NO_FRAME, A.ADV_NO_FRAME, A.ADV_WAIT_IMU, A.ADV_NO_FRAME]
    assert f.get_state(ids).tobytes() == after.tobytes() and [s.seq(i) for i in ids] == seq1
    # errors change nothing: readings older than the ring's newest (for any listed session), a repeated id, too many ids, a bad id
    good = _still_stream(_capi, 1.11, 1.3, rng)
    bad = good.copy()
    bad["t"][3] = 1.0
    for call in (lambda: f.feed_imu([2, 1], [good, bad]), lambda: f.feed_imu([2], [hist[:5]]), lambda: f.feed_imu([2, 2], [good, good]),
                 lambda: f.feed_imu([9], [good]), lambda: f.advance([0, 0]), lambda: f.advance([0, 1, 2, 3, 4]), lambda: f.advance([7])):
        with pytest.raises(_capi.HnetError):
            call()
    assert f.get_state(ids).tobytes() == after.tobytes() and [s.seq(i) for i in ids] == seq1
    f.feed_imu([2], [good])                                                        # session 2's ring is as it was: its window comes out of hist + good
    _, _, _, status = f.advance(ids)
    assert list(status) == [A.ADV_NO_FRAME, A.ADV_NO_FRAME, A.ADV_PROPAGATED, A.ADV_NO_FRAME]
    _same_readings(f.last_selection(2), _host_select(fref, np.concatenate([hist, good]), 1.0, 1.2))
    tg._close(f.get_state([2])[0], _host_propagate(ref, before[2:3], p, 1.2, np.concatenate([hist, good]))[0])
    # readings more than 10 s behind the newest are not selected, although the ring still holds them
    f.set_state(3, tg._state(_capi, rng, 0.05))
    slow = _still_stream(_capi, 0.0, 12.0, rng, dt=0.1)
    f.feed_imu([3], [slow])
    s.push([3], fr[:1], t=[11.95])
    _, _, _, status = f.advance([3])
    assert list(status) == [A.ADV_PROPAGATED]
    sel = f.last_selection(3)
    _same_readings(sel, _host_select(fref, slow, 0.05, 11.95))
    assert sel["t"][0] >= 2.0 - 1e-9 and len(sel) < len(slow) - 15
    # uninitialize: the next advance initialises again from the ring (session 4: never had a state; 0: had one)
    r, wait, _ = fc.stream("still_then_jerk", 31, t_end=15.0, t_start=12.0)
    for i in (0, 4):
        assert f.initialized(i) == (i == 0)
        f.uninitialize(i)
        assert not f.initialized(i) and s.image_count(i) == 0
        f.feed_imu([i], [fc.imu_records(r)])
        _, _, _, status = f.advance([i])
        assert list(status) == [A.ADV_NO_FRAME]                                    # no frame since the restart
        s.push([i], fr[:1], t=[14.9])
        st, _, _, status = f.advance([i])
        assert list(status) == [A.ADV_INITIALIZED] and f.initialized(i) and s.image_count(i) == 1 and st[0]["t"] == 14.9
    a, b = f.get_state([0])[0], f.get_state([4])[0]
    assert a.tobytes() == b.tobytes()                                              # same readings, same parameters: the same state, whatever was there before
    for o in (f, s, e):
        o.close()


def test_mixed_call_at_full_capacity(blob, ref, fref):
    """256 sessions in one advance at max_batch = 256, all kinds present"""
    _capi, HnetEngine, HnetSessions, HnetFilters = tg._mods()
    A = _capi
    K = 256
    e = _engine(blob, K)
    s = HnetSessions(e, K)
    f = HnetFilters(s, 1)
    f.enable_feed(1024)
    rng = np.random.default_rng(6)
    ids = np.arange(K, dtype=np.int32)
    kind = np.empty(K, int)
    kind[:100], kind[100:140], kind[140:180], kind[180:200], kind[200:230], kind[230:] = (A.ADV_STEPPED, A.ADV_PROPAGATED, A.ADV_INITIALIZED,
                                                                                         A.ADV_WAIT_INIT, A.ADV_WAIT_IMU, A.ADV_NO_FRAME)
    kind = kind[rng.permutation(K)]                                                # the kinds are interleaved in the list
    p = HnetFilters.default_params()
    still = _still_stream(_capi, 2.0, 3.0, rng)
    feeds, t_frame = [], np.full(K, 2.9)
    base = tg._frames(rng, 2)
    s.push(ids[kind == A.ADV_STEPPED], np.repeat(base[:1], 100, 0), t=[2.85] * 100)
    for i in range(K):
        if kind[i] in (A.ADV_INITIALIZED, A.ADV_WAIT_INIT):
            r, wait, _ = fc.stream("still_then_jerk" if kind[i] == A.ADV_INITIALIZED else "never_moving", 1000 + i)
            feeds.append(fc.imu_records(r))
            f.set_init_params(i, fc.init_params(wait, height=1.0))     # (0.1 m above the ground plane the jerk's 0.9 s would carry the state through it)
        else:
            f.set_state(i, tg._state(_capi, rng, 2.9 if kind[i] == A.ADV_NO_FRAME else 2.8))
            feeds.append(still[still["t"] < 2.88] if kind[i] == A.ADV_WAIT_IMU else still)
    f.feed_imu(ids, feeds)
    s.push(ids, np.repeat(base[1:], K, 0), t=list(t_frame))
    before, seq0 = f.get_state(ids), [s.seq(i) for i in ids]
    out, net, upd, status = f.advance(ids)
    assert list(status) == list(kind)
    after = f.get_state(ids)
    checked = 0
    for i in range(K):
        k = kind[i]
        assert s.seq(i) == seq0[i] + (1 if k == A.ADV_STEPPED else 0)
        if k in (A.ADV_WAIT_IMU, A.ADV_NO_FRAME, A.ADV_WAIT_INIT):
            assert after[i].tobytes() == before[i].tobytes() and not net[0, i].any()
            continue
        assert after[i].tobytes() == out[i].tobytes() and after[i]["t"] == 2.9 and np.isfinite(after[i]["cov"]).all()
        assert np.all(after[i]["offset"] == 0) and net[0, i].any() == (k == A.ADV_STEPPED)
        if k == A.ADV_PROPAGATED and checked < 8:
            tg._close(after[i], _host_propagate(ref, before[i:i + 1], p, 2.9, still)[0])
            checked += 1
        if k == A.ADV_STEPPED and checked < 16:                                     # ungated (2 images): the propagation and the reset
            tg._close(after[i], _host_propagate(ref, before[i:i + 1], p, 2.9, still)[0])
            checked += 1
        if k == A.ADV_INITIALIZED:
            assert f.initialized(i) and s.image_count(i) == 1
    assert len(f.last_priors(100)) == 1
    for o in (f, s, e):
        o.close()
