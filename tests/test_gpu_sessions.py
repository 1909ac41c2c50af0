"""hnet_sessions (include/hnet.h): many camera streams on one context.  The per-pair mask sequence table must give the bits of the contiguous run it generalises;
a sessions call must give the bits of the seq-table forward on the frames the caller pushed (ring, gather and bookkeeping exact), agree with one dedicated context
per camera within the cross-order gate of test_gpu_latency_path.py (5e-5 px, 1e-5 relative covariance, error map <= 1 grey level on < 0.1 % of the pixels),
and equal it bit for bit at n = 1 (both run the batch-1 latency path with the same key)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL_PX_PATHS, TOL_COV_PATHS = 5e-5, 1e-5
K_UZH = (275.46015578667294, 274.9948095922592, 315.958384100568, 242.7123497822731)
D_UZH = (-6.545154718304953e-06, -0.010379525898159981, 0.014935312423953146, -0.005639061406567785)
D_RADTAN = (-0.28, 0.07, 1e-3, -5e-4)


def _gate(a, b):
    """(mean, cov[, err u8]) within the cross-order gate"""
    ok = np.abs(a[0] - b[0]).max() < TOL_PX_PATHS and np.abs(a[1] - b[1]).max() / np.abs(b[1]).max() < TOL_COV_PATHS
    if len(a) > 2 and a[2] is not None:
        de = np.abs(a[2].astype(np.int64) - b[2].astype(np.int64))
        ok = ok and de.max() <= 1 and float((de > 0).mean()) < 1e-3
    return ok


def _seqs_call(e, prev, curr, prior, seqs, want_err=False):
    """infer_batch_seqs_packed_device on host arrays -> (mean [B,8], cov [B,8,8], err float [B,224,320] or None)"""
    import torch
    from cuahn_vio_amd.homography_net import PIX_U8
    dev = torch.device("cuda:0")
    b = prev.shape[0]
    p, c = torch.from_numpy(np.ascontiguousarray(prev)).to(dev), torch.from_numpy(np.ascontiguousarray(curr)).to(dev)
    pr = None if prior is None else torch.from_numpy(np.ascontiguousarray(prior, dtype=np.float32)).to(dev)
    sq = torch.from_numpy(np.asarray(seqs, dtype=np.uint64).view(np.int64).copy()).to(dev)
    out = torch.zeros(b, 72, device=dev)
    err = torch.zeros(b, 224, 320, device=dev) if want_err else None
    torch.cuda.synchronize()                                   # torch's fills before the context's own stream writes the buffers
    e.infer_batch_seqs_packed_device(p.data_ptr(), c.data_ptr(), PIX_U8, pr.data_ptr() if pr is not None else None, b, sq.data_ptr(), out.data_ptr(),
                                     err.data_ptr() if want_err else None)
    e.synchronize()
    o = out.cpu().numpy()
    return o[:, :8].copy(), o[:, 8:].reshape(b, 8, 8).copy(), (err.cpu().numpy() if want_err else None)


def _packed_call(e, prev, curr, prior, seq0, want_err=False):
    import torch
    from cuahn_vio_amd.homography_net import PIX_U8
    dev = torch.device("cuda:0")
    b = prev.shape[0]
    p, c = torch.from_numpy(prev).to(dev), torch.from_numpy(curr).to(dev)
    pr = None if prior is None else torch.from_numpy(np.ascontiguousarray(prior, dtype=np.float32)).to(dev)
    out = torch.zeros(b, 72, device=dev)
    err = torch.zeros(b, 224, 320, device=dev) if want_err else None
    torch.cuda.synchronize()                                   # torch's fills before the context's own stream writes the buffers
    e.infer_batch_packed_device(p.data_ptr(), c.data_ptr(), PIX_U8, pr.data_ptr() if pr is not None else None, b, seq0, out.data_ptr(),
                                err.data_ptr() if want_err else None)
    e.synchronize()
    o = out.cpu().numpy()
    return o[:, :8].copy(), o[:, 8:].reshape(b, 8, 8).copy(), (err.cpu().numpy() if want_err else None)


def _u8(err_f):
    return np.clip(err_f, 0.0, 255.0).astype(np.uint8)        # errmap_kernel's u8 copy: clamp, truncate


class _Dedicated:
    """one context per camera, driven as the reference drives its HomographyNet object: hnet_push_image / hnet_push_raw_image + hnet_infer"""

    def __init__(self, blob, **kw):
        from cuahn_vio_amd.homography_net import HnetEngine
        self.e = HnetEngine(blob, **kw)
        self.L, self.h = self.e._L, self.e.handle

    def push(self, frame, t):
        f = np.ascontiguousarray(frame)
        assert self.L.hnet_push_image(self.h, f.ctypes.data, 224, 320, 320, float(t)) == 0

    def infer(self, prior):
        want_err = bool(self.e.config().emit_error_map)
        mean, cov, err = np.zeros(8, np.float32), np.zeros((8, 8), np.float32), np.zeros((224, 320), np.uint8)
        pr = (C.c_double * 8)(*[float(x) for x in prior]) if prior is not None else None
        fp = C.POINTER(C.c_float)
        rc = self.L.hnet_infer(self.h, pr, 0, mean.ctypes.data_as(fp), cov.ctypes.data_as(fp), err.ctypes.data_as(C.POINTER(C.c_uint8)) if want_err else None)
        assert rc == 0, self.L.hnet_last_error(self.h)
        return (mean, cov, err) if want_err else (mean, cov)

    def count(self):
        return int(self.L.hnet_image_count(self.h))

    def time(self):
        return float(self.L.hnet_latest_time(self.h))


# ---- 1. the seq table with a contiguous run is the pair_seq0 forward, bit for bit ------------------------------------------------------------------
@pytest.mark.parametrize("precision", [pytest.param(3, id="f16x2"), pytest.param(2, id="bf16x3")])
@pytest.mark.parametrize("variant", ["full", "prior3"])
def test_seq_table_contiguous_run_is_pair_seq0(blob, precision, variant):
    from cuahn_vio_amd import synth
    from cuahn_vio_amd.homography_net import HnetEngine
    e = HnetEngine(blob, variant=variant, mc_samples=16, dropout_p=0.05, mc_seed=21, max_batch=64, emit_error_map=True, precision=precision)
    for b in (1, 3, 8, 9, 64):
        prev, curr, prior, _ = synth.make_batch(700 + b, min(b, 32))
        reps = (b + 31) // 32
        prev, curr, prior = (np.tile(a, (reps,) + (1,) * (a.ndim - 1))[:b].copy() for a in (prev, curr, prior))
        pr = None if variant == "full" else prior
        s0 = 1000 + 37 * b
        ref = _packed_call(e, prev, curr, pr, s0, want_err=True)
        got = _seqs_call(e, prev, curr, pr, np.arange(s0, s0 + b, dtype=np.uint64), want_err=True)
        for x, y in zip(got, ref):
            assert np.array_equal(x, y), f"batch {b}"
    assert e.precision() == precision
    e.close()


# ---- 2. any table: every pair is the oracle with its own key; permuting inputs and table permutes the outputs bitwise --------------------------------
def test_seq_table_any_values_match_oracle_and_permute(blob, oracle):
    from conftest import TOL_COV_REL, tol_px_vs_oracle
    from cuahn_vio_amd import synth
    from cuahn_vio_amd.homography_net import HnetEngine
    e = HnetEngine(blob, variant="prior3", mc_samples=16, dropout_p=0.05, mc_seed=5, max_batch=64, precision=3)
    prev, curr, prior, _ = synth.make_batch(811, 5)
    seqs = np.array([7, 7, 2 ** 63 - 3, 2 ** 63 + 11, 2 ** 64 - 1], dtype=np.uint64)
    m, c, _ = _seqs_call(e, prev, curr, prior, seqs)
    for b in range(5):
        ref = oracle.forward(prev[b], curr[b], prior[b], blocks_to_run=3, n_mc=16, p=0.05, mc_seed=5, pair_seq=int(seqs[b]))
        assert np.abs(m[b] - ref["mean"]).max() < tol_px_vs_oracle(3), b
        assert np.abs(c[b] - ref["cov"]).max() / np.abs(ref["cov"]).max() < TOL_COV_REL, b
    rng = np.random.default_rng(3)
    for b in (5, 64):
        pv, cu, pr, _ = synth.make_batch(900 + b, min(b, 32))
        reps = (b + 31) // 32
        pv, cu, pr = (np.tile(a, (reps,) + (1,) * (a.ndim - 1))[:b].copy() for a in (pv, cu, pr))
        sq = rng.integers(0, 2 ** 63, size=b, dtype=np.int64).astype(np.uint64)
        sq[:2] = [2 ** 64 - 2, 2 ** 64 - 2]
        m0, c0, _ = _seqs_call(e, pv, cu, pr, sq)
        perm = rng.permutation(b)
        m1, c1, _ = _seqs_call(e, pv[perm], cu[perm], pr[perm], sq[perm])
        assert np.array_equal(m1, m0[perm]) and np.array_equal(c1, c0[perm]), f"batch {b}"
    e.close()


# ---- 3. sessions match the seq-table forward (bitwise) and dedicated contexts (gate; bitwise at n = 1) ---------------------------------------------------
def _session_frames(k_sessions, n_frames):
    """per session a sequence of frames and priors: the replay fixture at different offsets, plus synthetic frames"""
    from cuahn_vio_amd import replay, synth
    fx = replay.load_fixture("indoor_forward_7")
    frames, priors = [], []
    for i in range(k_sessions):
        if i < 3:
            off = 40 + 150 * i
            frames.append([replay.render_frame(fx, off + j) for j in range(n_frames)])
            priors.append([replay.prior_offsets(fx, off + j - 1) for j in range(n_frames)])      # prior of the pair (j - 1, j)
        else:
            pv, cu, pr, _ = synth.make_batch(60 + 10 * i, n_frames)
            frames.append([pv[0]] + [cu[j] for j in range(n_frames - 1)])
            priors.append([pr[max(j - 1, 0)] for j in range(n_frames)])
    return frames, priors


def test_sessions_match_seq_table_and_dedicated_contexts(blob):
    from cuahn_vio_amd.homography_net import HnetEngine, HnetSessions
    K, ticks = 5, 12
    kw = dict(variant="prior3", mc_samples=16, dropout_p=0.05, mc_seed=13, emit_error_map=True, precision=3)
    e = HnetEngine(blob, max_batch=8, **kw)
    s = HnetSessions(e, K)
    ded = [_Dedicated(blob, max_batch=1, **kw) for _ in range(K)]
    frames, priors = _session_frames(K, ticks + 2)
    pushed = [[] for _ in range(K)]            # frames the test pushed, per session
    seq = [0] * K
    rng = np.random.default_rng(2024)
    n_single = 0
    for tick in range(ticks):
        push = sorted(rng.choice(K, size=int(rng.integers(1, K + 1)), replace=False).tolist()) if tick > 1 else list(range(K))
        fr = np.stack([frames[i][len(pushed[i])] for i in push])
        ts = [0.05 * tick + 0.001 * i for i in push]
        s.push(push, fr, ts)
        for j, i in enumerate(push):
            ded[i].push(fr[j], ts[j])
            pushed[i].append(fr[j])
        for i in range(K):
            assert s.image_count(i) == ded[i].count() and s.latest_time(i) == ded[i].time()
        ready = [i for i in range(K) if len(pushed[i]) >= 2]
        if not ready:
            continue
        n = 1 if tick in (3, 7) else int(rng.integers(1, len(ready) + 1))
        ids = sorted(rng.choice(ready, size=n, replace=False).tolist())
        pr = np.stack([priors[i][len(pushed[i]) - 1] for i in ids]).astype(np.float64)
        m, c, err = s.infer(ids, pr, want_err=True)
        # (i) the seq-table forward on the frames the test pushed, each session's own count as its key
        ref = _seqs_call(e, np.stack([pushed[i][-2] for i in ids]), np.stack([pushed[i][-1] for i in ids]), pr.astype(np.float32),
                         [seq[i] for i in ids], want_err=True)
        assert np.array_equal(m, ref[0]) and np.array_equal(c, ref[1]) and np.array_equal(err, _u8(ref[2])), f"tick {tick}"
        for j, i in enumerate(ids):
            d = ded[i].infer(pr[j])
            seq[i] += 1
            assert s.seq(i) == seq[i]
            # (ii) each session against its own dedicated context
            assert _gate((m[j], c[j], err[j]), d), f"tick {tick} session {i}"
            # (iii) n = 1: both run the batch-1 latency path with the same key
            if n == 1:
                n_single += 1
                assert np.array_equal(m[0], d[0]) and np.array_equal(c[0], d[1]) and np.array_equal(err[0], d[2]), f"tick {tick}"
    assert n_single >= 2 and sum(seq) > 10
    t = s.last_timing()
    assert t["n_inferences"] > 0 and t["device_ms"] > 0
    assert e.last_timing()["n_inferences"] == 0                         # the context's own counters are untouched
    s.close()
    e.close()
    for d in ded:
        d.e.close()


# ---- 4. raw frames: the remap into the ring is hnet_op_undistort's, bit for bit; push_raw -> infer agrees with the dedicated path -----------------------
def _raw(seed, rows=480, cols=640):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:rows, 0:cols]
    img = 128 + 60 * np.sin(x / 23.0 + seed) * np.cos(y / 17.0) + 40 * np.sin((x + 2 * y) / 41.0) + rng.integers(-12, 13, (rows, cols))
    return np.clip(img, 0, 255).astype(np.uint8)


def test_sessions_raw_push_matches_single_frame_remap(blob):
    from cuahn_vio_amd.homography_net import HnetEngine, HnetError, HnetSessions
    kw = dict(variant="prior3", mc_samples=16, dropout_p=0.05, mc_seed=3, emit_error_map=True, precision=3)
    e = HnetEngine(blob, max_batch=4, **kw)
    s = HnetSessions(e, 3)
    cams = [s.add_camera(K_UZH, D_UZH, 480, 640, fisheye=True), s.add_camera(K_UZH, D_RADTAN, 480, 640, fisheye=False)]
    assert cams == [0, 1]
    s.bind_camera(0, cams[0])
    s.bind_camera(2, cams[1])
    ded = []
    for fish, d in ((True, D_UZH), (False, D_RADTAN)):
        x = _Dedicated(blob, max_batch=1, **kw)
        x.e.set_camera(K_UZH, d, 480, 640, fisheye=fish)
        ded.append(x)
    with pytest.raises(HnetError):
        s.push_raw([1], _raw(1)[None])                               # session 1 has no camera
    prior = np.zeros((2, 8))
    for step in range(3):
        raws = np.stack([_raw(10 + 2 * step), _raw(11 + 2 * step)])
        s.push_raw([0, 2], raws, [0.1 * step, 0.1 * step])
        for j, sid in enumerate((0, 2)):
            assert np.array_equal(s.frame(sid, 1), ded[j].e.op_undistort(raws[j])), f"step {step} session {sid}"
            ded[j].e.push_raw_image(raws[j], 0.1 * step)
        if step >= 1:
            m, c, err = s.infer([0, 2], prior, want_err=True)
            for j in range(2):
                assert _gate((m[j], c[j], err[j]), ded[j].infer(prior[j])), f"step {step}"
    with pytest.raises(HnetError):
        s.push_raw([0], _raw(1, 100, 100)[None])                     # a raw size other than the camera's
    assert s.image_count(0) == 3 and s.image_count(1) == 0
    s.close()
    e.close()
    for d in ded:
        d.e.close()


# ---- 5. bookkeeping: counts, times, set_seq, reset, every error code without a state change, the context's own sequence --------------------------------
def test_sessions_bookkeeping_and_errors(blob):
    from cuahn_vio_amd import synth
    from cuahn_vio_amd.homography_net import HnetEngine, HnetError, HnetSessions
    kw = dict(variant="prior3", mc_samples=16, dropout_p=0.05, mc_seed=8, precision=3)
    e = HnetEngine(blob, max_batch=4, **kw)
    s = HnetSessions(e, 6)
    prev, curr, prior, _ = synth.make_batch(400, 4)
    s.push([0, 1, 2, 3], prev, [1.0, 2.0, 3.0, 4.0])
    assert [s.image_count(i) for i in range(6)] == [1, 1, 1, 1, 0, 0] and s.latest_time(0) == -1.0
    s.push([0, 1, 2, 3], curr, [1.5, 2.5, 3.5, 4.5])
    assert s.image_count(0) == 2 and s.latest_time(3) == 4.5
    assert np.array_equal(s.frame(1, 0), prev[1]) and np.array_equal(s.frame(1, 1), curr[1])
    pr = prior.astype(np.float64)

    def state():
        return [(s.image_count(i), s.seq(i), s.latest_time(i)) for i in range(6)]

    def expect(status, fn):
        before = state()
        with pytest.raises(HnetError) as ex:
            fn()
        assert ex.value.status == status and state() == before

    expect(4, lambda: s.infer([0, 4], pr[:2]))                                    # NOT_READY
    expect(1, lambda: s.infer([0, 6], pr[:2]))                                    # id out of range
    expect(1, lambda: s.infer([0, 0], pr[:2]))                                    # repeated
    expect(1, lambda: s.infer([0, 1], None))                                      # prior required
    expect(1, lambda: s.infer([0], pr[:1], want_err=True))                        # no emit_error_map
    expect(5, lambda: s.infer([0, 1, 2, 3, 4], np.zeros((5, 8))))                 # n > max_batch
    expect(1, lambda: s.push([2, 2], curr[:2]))
    expect(1, lambda: s.push([7], curr[:1]))
    expect(5, lambda: s.push([0, 1, 2, 3, 4], np.concatenate([curr, curr[:1]])))
    expect(1, lambda: s.push_raw([0], np.zeros((1, 480, 640), np.uint8)))       # no camera bound
    with pytest.raises(HnetError):
        s.bind_camera(0, 0)                                                       # no such camera
    # the next good call gives the expected bits
    m, c = s.infer([0, 1, 2, 3], pr)
    ref = _seqs_call(e, prev, curr, prior, [0, 0, 0, 0])
    assert np.array_equal(m, ref[0]) and np.array_equal(c, ref[1])
    # set_seq: the next result is the seq-table call with that key
    s.set_seq(2, 10 ** 12)
    m, c = s.infer([2], pr[2:3])
    ref = _seqs_call(e, prev[2:3], curr[2:3], prior[2:3], [10 ** 12])
    assert np.array_equal(m, ref[0]) and np.array_equal(c, ref[1]) and s.seq(2) == 10 ** 12 + 1
    # reset: NOT_READY until two new frames have arrived, the sequence number is kept
    s.reset(1)
    assert s.image_count(1) == 0 and s.seq(1) == 1
    expect(4, lambda: s.infer([1], pr[1:2]))
    s.push([1], prev[3:4])
    expect(4, lambda: s.infer([1], pr[1:2]))
    s.push([1], curr[3:4])
    m, c = s.infer([1], pr[3:4])
    ref = _seqs_call(e, prev[3:4], curr[3:4], prior[3:4], [1])
    assert np.array_equal(m, ref[0]) and np.array_equal(c, ref[1])
    # hnet_infer on the same context, interleaved with session calls, = a fresh context; its own sequence is untouched
    fresh = _Dedicated(blob, max_batch=4, **kw)
    mine = _Dedicated.__new__(_Dedicated)
    mine.e, mine.L, mine.h = e, e._L, e.handle
    outs = []
    for k, x in enumerate((mine, fresh)):
        got = []
        for j in range(3):
            x.push(prev[j] if j % 2 == 0 else curr[j], float(j))
            if x is mine:
                s.push([0], curr[j:j + 1])
                s.infer([0, 3], pr[:2])
            if j >= 1:
                got.append(x.infer(pr[j]))
        outs.append(got)
    for a, b in zip(*outs):
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert e.last_timing()["n_inferences"] == 2
    s.close()
    e.close()
    fresh.e.close()


def test_sessions_refuse_a_sample_shard_context(blob):
    from cuahn_vio_amd.homography_net import HnetEngine, HnetError, HnetSessions
    e = HnetEngine(blob, variant="full", mc_samples=16, dropout_p=0.05, max_batch=2, mc_shard=(0, 8))
    with pytest.raises(HnetError) as ex:
        HnetSessions(e, 4)
    assert ex.value.status == 6
    e.close()


# ---- 6. capacity: max_batch = 256 pairs over 300 sessions, two ticks ----------------------------------------------------------------------------------------
def test_sessions_full_capacity(blob, oracle):
    from conftest import TOL_COV_REL, tol_px_vs_oracle
    from cuahn_vio_amd import synth
    from cuahn_vio_amd.homography_net import HnetEngine, HnetSessions
    K, B = 300, 256
    e = HnetEngine(blob, variant="full", mc_samples=16, dropout_p=0.05, mc_seed=17, max_batch=B, precision=3)
    s = HnetSessions(e, K)
    pv, cu, _, _ = synth.make_batch(1300, 32)
    pool = np.concatenate([pv, cu])                                   # 64 distinct frames
    rng = np.random.default_rng(9)
    last = {}
    for ids in (list(range(0, B)), list(range(B, K))):                # every session holds one frame
        f = pool[rng.integers(0, 64, len(ids))]
        s.push(ids, f)
        for j, i in enumerate(ids):
            last[i] = [f[j]]
    seqs = {i: 0 for i in range(K)}
    for tick in range(2):
        ids = sorted(rng.choice(K, size=B, replace=False).tolist())
        f = pool[rng.integers(0, 64, B)]
        s.push(ids, f)
        for j, i in enumerate(ids):
            last[i].append(f[j])
        ready = sorted(rng.choice([i for i in range(K) if len(last[i]) >= 2], size=B, replace=False).tolist())
        m, c = s.infer(ready)
        prev = np.stack([last[i][-2] for i in ready])
        curr = np.stack([last[i][-1] for i in ready])
        ref = _seqs_call(e, prev, curr, None, [seqs[i] for i in ready])
        assert np.array_equal(m, ref[0]) and np.array_equal(c, ref[1]), f"tick {tick}"
        for j in range(tick, B, 8):                                  # the oracle on every 8th slot (the CPU oracle takes ~1 s per pair)
            o = oracle.forward(prev[j], curr[j], None, n_mc=16, p=0.05, mc_seed=17, pair_seq=seqs[ready[j]])
            assert np.abs(m[j] - o["mean"]).max() < tol_px_vs_oracle(3, worst_slot=True), (tick, j)
            assert np.abs(c[j] - o["cov"]).max() / np.abs(o["cov"]).max() < TOL_COV_REL, (tick, j)
        for i in ready:
            seqs[i] += 1
            assert s.seq(i) == seqs[i]
    s.close()
    e.close()
