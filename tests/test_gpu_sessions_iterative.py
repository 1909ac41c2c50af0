"""The IEKF's second model on the many-camera path: hnet_sessions_set_iterative_model + hnet_sessions_infer_iter, and the iteration routing of
hnet_filters_step / hnet_filters_advance (include/hnet.h).  Main model prior-3, N = 16, p = 0.05; iterative model prior-1, N = 8, p = 0.1; both from the
tests' synthetic weights with one mc_seed.  The yardsticks are code this change does not touch: the HomographyNet mirror with weights_blob_iterative (two
dedicated contexts joined by hnet_attach_images) and tests/cpp/filters_ref.cpp (the hnet_ekf header)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import test_filters_feed_cpu as fc
import test_gpu_filters as tg
import test_sessions_iterative_cpu as ic

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = dict(variant="prior3", mc_samples=16, dropout_p=0.05)
ITER = dict(variant="prior1", mc_samples=8, dropout_p=0.1)
PREC_BF16X3, PREC_F16X2 = 2, 3
INVALID, UNSUPPORTED = 1, 6          # include/hnet.h HNET_ERR_INVALID_ARG, HNET_ERR_UNSUPPORTED


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("filters_ref") / "filters_ref.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-shared", "-fPIC", "-pthread", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "filters_ref.cpp"), "-o", so], check=True)
    return C.CDLL(so)


@pytest.fixture(scope="module")
def fref(tmp_path_factory):
    return fc.build_ref(str(tmp_path_factory.mktemp("filters_feed_ref") / "filters_feed_ref.so"))


def _iter_engine(blob, max_batch, mc_seed=9, **kw):
    from cuahn_vio_amd.homography_net import HnetEngine
    return HnetEngine(blob, mc_seed=mc_seed, max_batch=max_batch, **ITER, **kw)


def _mirror(state, mc_seed):
    """the HomographyNet mirror of one camera with two weight files carrying their variant records (main / iterative), three IEKF iterations"""
    from cuahn_vio_amd import weights
    from cuahn_vio_amd.homography_net import HomographyNet
    return HomographyNet("main.hnw", "iter.hnw", use_prior=True, num_of_iteration=3, mc_seed=mc_seed,
                         weights_blob=weights.pack_state_dict(state, variant=MAIN), weights_blob_iterative=weights.pack_state_dict(state, variant=ITER))


def _mirror_seq(h):
    """the mirror's one shared sequence count (the main context's inference count)"""
    return h._eng.last_timing()["n_inferences"]


def test_sessions_match_dedicated_pairs(blob, state):
    """4 sessions with different frames, 6 frames each; per frame infer iterations 0, 1, 2 on the sessions object; per camera network_inference(prior, it)
    of a mirror fed the same frames and priors: bitwise equal, equal sequence counts"""
    from cuahn_vio_amd.homography_net import HnetEngine, HnetSessions
    K, F = 4, 6
    e = HnetEngine(blob, mc_seed=9, max_batch=K, **MAIN)
    ei = _iter_engine(blob, K)
    s = HnetSessions(e, K)
    s.set_iterative_model(ei)
    mirrors = [_mirror(state, 9) for _ in range(K)]
    rng = np.random.default_rng(31)
    frames = [tg._frames(np.random.default_rng(100 + k), F) for k in range(K)]
    ids = np.arange(K, dtype=np.int32)
    guard = False
    for j in range(F):
        s.push(ids, np.stack([frames[k][j] for k in range(K)]), t=[0.1 * j] * K)
        for k in range(K):
            mirrors[k].load_current_img(frames[k][j], 0.1 * j)
        if j == 0:
            continue
        for it in range(3):
            prior = rng.standard_normal((K, 8)) * 2.0
            seq = [s.seq(k) for k in range(K)]
            mean, cov = s.infer(ids, prior, iteration=it)
            for k in range(K):
                mirrors[k].network_inference(prior[k], it)
                assert np.array_equal(mirrors[k].get_pred_mean().astype(np.float32).reshape(8), mean[k]), (j, it, k)
                assert np.array_equal(mirrors[k].get_pred_Cov().astype(np.float32), cov[k]), (j, it, k)
                assert s.seq(k) == _mirror_seq(mirrors[k]) == seq[k] + 1
            if it == 1:                                                        # the routing is visible: the main model gives other numbers
                m3, _ = e.infer_batch(frames[0][j - 1][None], frames[0][j][None], prior[:1].astype(np.float32), pair_seq0=seq[0])
                guard = guard or not np.array_equal(m3[0], mean[0])
    assert guard
    assert [s.seq(k) for k in range(K)] == [3 * (F - 1)] * K
    for h in mirrors:
        h.close()
    s.close(); ei.close(); e.close()


def test_step_matches_host_reference_with_iterative_model(blob, ref):
    """test_step_matches_host_reference with I = 3 and the iterative model attached: 8 sessions, 0 - 40 intervals, _ref_step fed with the step's outputs"""
    _capi, _, _, HnetFilters = tg._mods()
    iters = 3
    e, s, f = tg._setup(blob, 8, iters)
    ei = _iter_engine(blob, 8)
    s.set_iterative_model(ei)
    rng = np.random.default_rng(10 + iters)
    t_frame = 1.0 + 0.1 * 11
    counts = [0, 1, 2, 16, 40, 16, 3, 7]
    ps, sts, imus = [], [], []
    for i in range(8):
        p = tg._params(HnetFilters, rng, i)
        f.set_params(i, p)
        t0 = t_frame - 0.002 * max(counts[i], 1) - 0.0004
        st = tg._state(_capi, rng, t0)
        f.set_state(i, st)
        ps.append(p)
        sts.append(st)
        imus.append(tg._imu(rng, t0 + p.cam_imu_dt, counts[i]))
    ids = np.arange(8, dtype=np.int32)
    seq0 = [s.seq(i) for i in ids]
    out, net, upd = f.step(ids, [t_frame] * 8, imus)
    got = f.get_state(ids)
    assert got.tobytes() == out.tobytes()
    assert [s.seq(i) for i in ids] == [q + iters for q in seq0]
    for i in range(8):
        want, u = tg._ref_step(ref, sts[i], ps[i], t_frame, imus[i], iters, net[:, i, :], gate=1)
        assert upd[i] == u == iters
        tg._close(got[i], want[0])
    # forwards 1 and 2 are the iterative model's: the same pairs, priors and keys through prior-1 give the step's rows bit for bit
    pri = f.last_priors(8)
    prev = np.stack([s.frame(i, 0) for i in ids])
    curr = np.stack([s.frame(i, 1) for i in ids])
    for it in range(iters):
        eng = e if it == 0 else ei
        for i in range(8):
            m, c = eng.infer_batch(prev[i:i + 1], curr[i:i + 1], pri[it, i:i + 1], pair_seq0=seq0[i] + it)
            assert np.array_equal(m[0], net[it, i, :8]) and np.array_equal(c[0].reshape(64), net[it, i, 8:]), (it, i)
    f.close(); s.close(); ei.close(); e.close()


def test_chained_replay_matches_host_loop_with_iterative_model(blob, state, ref):
    """test_chained_replay_matches_host_loop with I = 3: 60 frames of replay_indoor_forward_7, 3 sessions; the host loop runs filters_ref propagation,
    then per camera the HomographyNet mirror with the iterative file, then ref_update_batch"""
    from cuahn_vio_amd import replay
    _capi, HnetEngine, HnetSessions, HnetFilters = tg._mods()
    fx = replay.load_fixture("indoor_forward_7")
    imu, R, v = tg._synthetic_imu(fx)
    iters, K, N = 3, 3, 60
    e1 = HnetEngine(blob, mc_seed=3, max_batch=4, **MAIN)
    ei = _iter_engine(blob, 4, mc_seed=3)
    s1 = HnetSessions(e1, K)
    s1.set_iterative_model(ei)
    f = HnetFilters(s1, iters)
    mirrors = [_mirror(state, 3) for _ in range(K)]
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
        host[k] = st[0]
    params = (_capi.FilterParams * K)(*([p] * K))
    ids = np.arange(K, dtype=np.int32)
    prop_only = host.copy()
    compared = same_prior = 0
    worst_net = 0.0
    frame0 = replay.render_frame(fx, 0)
    s1.push(ids, np.repeat(frame0[None], K, 0), t=[fx["t"][0]] * K)
    for h in mirrors:
        h.load_current_img(frame0, fx["t"][0])
    for k in range(1, N + 1):
        tk = float(fx["t"][k])
        fr = replay.render_frame(fx, k)
        s1.push(ids, np.repeat(fr[None], K, 0), t=[tk] * K)
        for h in mirrors:
            h.load_current_img(fr, tk)
        win = imu[(imu["t"] > fx["t"][k - 1] - 0.01) & (imu["t"] < tk + 0.01)]
        dev, net, upd = f.step(ids, [tk] * K, [win] * K)
        pri = f.last_priors(K)
        r = np.ascontiguousarray(win)
        for j in range(K):
            assert ref.ref_propagate_with_imu(C.c_void_p(host[j:j + 1].ctypes.data), C.byref(p), C.c_double(tk), C.c_void_p(r.ctypes.data), len(r)) >= 0
            ref.ref_propagate_with_imu(C.c_void_p(prop_only[j:j + 1].ctypes.data), C.byref(p), C.c_double(tk), C.c_void_p(r.ctypes.data), len(r))
        ref.ref_reset_batch(C.c_void_p(prop_only.ctypes.data), K)
        gate = np.array([int(mirrors[j].get_latest_inference_time() == tk and mirrors[j].img_counter > 10) for j in range(K)], np.int32)
        for it in range(iters):
            prior_px = host["offset"][:, :, :2].reshape(K, 8) * 159.5
            prior_cam = np.ascontiguousarray(host["offset"][:, :, :2].reshape(K, 8))
            mean = np.zeros((K, 8), np.float32)
            cov = np.zeros((K, 8, 8), np.float32)
            for j in range(K):
                mirrors[j].network_inference(prior_px[j], it)
                mean[j] = mirrors[j].get_pred_mean().astype(np.float32).reshape(8)
                cov[j] = mirrors[j].get_pred_Cov().astype(np.float32)
            if np.array_equal(prior_px.astype(np.float32), pri[it]):
                same_prior += 1
                assert np.array_equal(mean, net[it, :, :8]) and np.array_equal(cov.reshape(K, 64), net[it, :, 8:]), (k, it)
            else:
                worst_net = max(worst_net, float(np.abs(mean - net[it, :, :8]).max()))
            compared += 1
            ref.ref_update_batch(C.c_void_p(host.ctypes.data), params, K, C.c_void_p(mean.ctypes.data), C.c_void_p(cov.ctypes.data),
                                 C.c_void_p(prior_cam.ctypes.data), C.c_void_p(gate.ctypes.data), int(it != iters - 1), 1)
        ref.ref_reset_batch(C.c_void_p(host.ctypes.data), K)
        assert list(upd) == [iters * int(g) for g in gate]
    assert same_prior >= compared // 2, (same_prior, compared)
    got = f.get_state(ids)
    worst = 0.0
    for j in range(K):
        for fld in ("p", "q", "v", "ba", "bg"):
            d = np.abs(got[j][fld] - host[j][fld]).max() / max(1.0, np.abs(host[j][fld]).max())
            worst = max(worst, float(d))
            assert d <= 1e-8, (j, fld)
        dc = np.abs(got[j]["cov"] - host[j]["cov"]).max() / np.abs(host[j]["cov"]).max()
        worst = max(worst, float(dc))
        assert dc <= 1e-8
    assert [s1.seq(j) for j in ids] == [_mirror_seq(h) for h in mirrors] == [N * iters] * K
    moved = max(np.abs(got[j][fld] - prop_only[j][fld]).max() for j in range(K) for fld in ("p", "v", "bg"))
    assert moved > 1e-3, moved
    print(f"chained (iterative model): {compared} forwards compared, {same_prior} with bitwise-equal priors; largest state difference {worst:.3g}, "
          f"largest |mean| difference where the priors differ {worst_net:.3g} px; updates moved the state by up to {moved:.3g}")
    for h in mirrors:
        h.close()
    f.close(); s1.close(); ei.close(); e1.close()


def test_feed_equals_step_with_iterative_model(blob, ref, fref):
    """test_feed_equals_step (tests/test_gpu_filters_feed.py) with the iterative model attached to both filters objects and I = 3: bit for bit"""
    import test_gpu_filters_feed as tf
    _capi, HnetEngine, HnetSessions, HnetFilters = tg._mods()
    iters = 3
    ea, sa, fa = tg._setup(blob, 8, iters)
    eb, sb, fb = tg._setup(blob, 8, iters)
    ia, ib = _iter_engine(blob, 8), _iter_engine(blob, 8)
    sa.set_iterative_model(ia)
    sb.set_iterative_model(ib)
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
        ts = t_frame[i] + p.cam_imu_dt - 0.0007 + 0.002 * np.arange(5 * 42 + 4)
        r = np.zeros(len(ts), _capi.IMU_DTYPE)
        r["t"], r["wm"], r["am"] = ts, rng.standard_normal((len(ts), 3)) * 0.3, rng.standard_normal((len(ts), 3)) * 0.5 + [0, 0, 9.81]
        hist.append(r)
    fr = tg._frames(rng, 6)
    for tick in range(5):
        t_prev, t_frame = t_frame, t_frame + 0.002 * np.maximum(counts, 0.1) + 0.0004
        for s in (sa, sb):
            s.push(ids, np.repeat(fr[tick][None], 8, 0), t=list(t_frame))
        chunks = []
        for i in range(8):
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
            tf._same_readings(fa.last_selection(i), tf._host_select(fref, hist[i][:fed[i]], t_prev[i] + ps[i].cam_imu_dt, t_frame[i] + ps[i].cam_imu_dt))
        pa, pb = fa.last_priors(8), fb.last_priors(8)
        assert sta.tobytes() == stb.tobytes() and pa.tobytes() == pb.tobytes() and neta.tobytes() == netb.tobytes(), tick
        assert fa.get_state(ids).tobytes() == sta.tobytes()
        assert [sa.seq(i) for i in ids] == [sb.seq(i) for i in ids] == [iters * (tick + 1)] * 8
    for o in (fa, fb, sa, sb, ia, ib, ea, eb):
        o.close()


def _step_inputs(_capi, HnetFilters, seed, n=4):
    rng = np.random.default_rng(seed)
    t_frame = 1.0 + 0.1 * 11
    ps = [tg._params(HnetFilters, rng, i) for i in range(n)]
    sts = [tg._state(_capi, rng, t_frame - 0.0325) for _ in range(n)]
    imus = [tg._imu(rng, t_frame - 0.0325 + ps[i].cam_imu_dt, 16) for i in range(n)]
    return t_frame, ps, sts, imus


def _load(f, s, ps, sts, seq=None):
    for i in range(len(ps)):
        f.set_params(i, ps[i])
        f.set_state(i, sts[i])
        if seq is not None:
            s.set_seq(i, seq)


def test_nothing_changes_without_it(blob):
    """I = 1 steps with and without an attached model are bitwise equal; after detaching, I = 3 steps equal those of an object that never had one"""
    _capi, _, _, HnetFilters = tg._mods()
    n = 4
    t_frame, ps, sts, imus = _step_inputs(_capi, HnetFilters, 41, n)
    ids = np.arange(n, dtype=np.int32)
    # I = 1
    e1, s1, f1 = tg._setup(blob, n, 1)
    e2, s2, f2 = tg._setup(blob, n, 1)
    i2 = _iter_engine(blob, 8)
    s2.set_iterative_model(i2)
    for f, s in ((f1, s1), (f2, s2)):
        _load(f, s, ps, sts)
    a, b = f1.step(ids, [t_frame] * n, imus), f2.step(ids, [t_frame] * n, imus)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    assert [s1.seq(i) for i in ids] == [s2.seq(i) for i in ids] == [1] * n
    assert i2.precision() == e2.precision()
    for o in (f1, f2, s1, s2, i2, e1, e2):
        o.close()
    # I = 3: attach, step, detach; then the same step on it and on a fresh object
    e1, s1, f1 = tg._setup(blob, n, 3)
    e2, s2, f2 = tg._setup(blob, n, 3)
    i1 = _iter_engine(blob, 8)
    s1.set_iterative_model(i1)
    _load(f1, s1, ps, sts)
    with_model = f1.step(ids, [t_frame] * n, imus)
    s1.set_iterative_model(None)
    assert s1.iter_engine is None
    for f, s in ((f1, s1), (f2, s2)):
        _load(f, s, ps, sts, seq=0)
    a, b = f1.step(ids, [t_frame] * n, imus), f2.step(ids, [t_frame] * n, imus)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    assert with_model[1][1:].tobytes() != b[1][1:].tobytes()             # (the attached model had really run forwards 1 and 2)
    assert with_model[1][0].tobytes() == b[1][0].tobytes()
    assert [s1.seq(i) for i in ids] == [s2.seq(i) for i in ids] == [3] * n
    for o in (f1, f2, s1, s2, i1, e1, e2):
        o.close()


def test_attachment_errors(blob):
    """every refusal returns its code and leaves the attachment, the states and the sequence numbers as they were"""
    from cuahn_vio_amd import _capi
    from cuahn_vio_amd.homography_net import HnetEngine
    _, _, _, HnetFilters = tg._mods()
    n = 4
    e, s, f = tg._setup(blob, n, 3)
    et, st_, ft = tg._setup(blob, n, 3)                                   # a twin that receives no refused call
    ie, it_ = _iter_engine(blob, 8), _iter_engine(blob, 8)
    s.set_iterative_model(ie)
    st_.set_iterative_model(it_)
    t_frame, ps, sts, imus = _step_inputs(_capi, HnetFilters, 43, n)
    for ff, ss in ((f, s), (ft, st_)):
        _load(ff, ss, ps, sts, seq=5)
    ids = np.arange(n, dtype=np.int32)
    L = _capi.lib()

    def snap():
        return f.get_state(ids).tobytes(), [s.seq(i) for i in ids]

    before = snap()
    bad = [
        (e, INVALID),                                                               # the sessions' own context
        (HnetEngine(blob, variant="full", mc_samples=8, dropout_p=0.1, mc_seed=9, max_batch=8), INVALID),     # use_prior differs
        (_iter_engine(blob, 4), INVALID),                                            # max_batch below the main context's
        (HnetEngine(blob, mc_seed=9, max_batch=8, mc_shard=(0, 4), **ITER), UNSUPPORTED),   # a sample shard
    ]
    for eng, code in bad:
        assert L.hnet_sessions_set_iterative_model(s._s, eng.handle) == code
        if eng is not e:
            eng.close()
        assert snap() == before
    mean, cov = np.zeros((n, 8), np.float32), np.zeros((n, 64), np.float32)
    pr = np.zeros((n, 8))
    assert L.hnet_sessions_infer_iter(s._s, -1, n, ids.ctypes.data, pr.ctypes.data, mean.ctypes.data, cov.ctypes.data, None) == INVALID
    err = np.zeros((n, 224, 320), np.uint8)                                          # no emit_error_map on the iterative context
    assert L.hnet_sessions_infer_iter(s._s, 1, n, ids.ctypes.data, pr.ctypes.data, mean.ctypes.data, cov.ctypes.data, err.ctypes.data) == INVALID
    assert snap() == before
    # the attachment is intact: iteration 1 and a step give the twin's bits
    a, b = s.infer(ids, pr, iteration=1), st_.infer(ids, pr, iteration=1)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    a, b = f.step(ids, [t_frame] * n, imus), ft.step(ids, [t_frame] * n, imus)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    assert [s.seq(i) for i in ids] == [st_.seq(i) for i in ids] == [9] * n
    for o in (f, ft, s, st_, ie, it_, e, et):
        o.close()


def test_attachment_refuses_another_device(blob):
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("one device visible")
    from cuahn_vio_amd import _capi
    e, s, f = tg._setup(blob, 2, 3)
    other = _iter_engine(blob, 8, device_id=1)
    assert _capi.lib().hnet_sessions_set_iterative_model(s._s, other.handle) == INVALID
    for o in (other, f, s, e):
        o.close()


def test_repair_on_the_iterative_context(blob, ref):
    """an iterative model whose block-4 activations overflow the fp16 planes (tests/test_sessions_iterative_cpu.py builds and checks it with the
    oracle): one step demotes the iterative context only, advances the sequence numbers by I, and equals a step of fresh objects whose iterative engine
    runs HNET_PREC_BF16X3 from the start"""
    _capi, _, _, HnetFilters = tg._mods()
    iters, n = 3, 4
    ov = ic.overflow_iterative_blob()
    t_frame, ps, sts, imus = _step_inputs(_capi, HnetFilters, 47, n)
    ids = np.arange(n, dtype=np.int32)
    e, s, f = tg._setup(blob, n, iters, precision=PREC_F16X2)
    ie = _iter_engine(ov, 8, precision=PREC_F16X2)
    assert ie.precision() == PREC_F16X2 and e.precision() == PREC_F16X2
    s.set_iterative_model(ie)
    _load(f, s, ps, sts)
    out, net, upd = f.step(ids, [t_frame] * n, imus)
    assert ie.precision() == PREC_BF16X3 and e.precision() == PREC_F16X2
    assert [s.seq(i) for i in ids] == [iters] * n
    assert np.all(np.isfinite(net))
    e2, s2, f2 = tg._setup(blob, n, iters, precision=PREC_F16X2)
    ie2 = _iter_engine(ov, 8, precision=PREC_BF16X3)
    s2.set_iterative_model(ie2)
    _load(f2, s2, ps, sts)
    out2, net2, upd2 = f2.step(ids, [t_frame] * n, imus)
    assert list(upd) == list(upd2)
    for i in range(n):
        tg._close(out[i], out2[i])
    print(f"repair: bitwise equal to the fresh BF16X3 step: {out.tobytes() == out2.tobytes() and net.tobytes() == net2.tobytes()}")
    for o in (f, f2, s, s2, ie, ie2, e, e2):
        o.close()
