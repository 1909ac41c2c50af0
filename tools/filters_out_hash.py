#!/usr/bin/env python3
"""sha256 of what the hnet_filters_* calls return in one fixed scenario, one line per kind of call - before / after a change of the filter kernels
or their host code that must not alter a single bit (tools/out_hash.py does the same for the network).  Run it once per library in a fresh process
(HNET_LIB_PATH selects the library) and compare the lines.
   python tools/filters_out_hash.py
Per max_iekf_iteration in (1, 3), 8 sessions at max_batch 8:
 fed:  rings of 64 readings that wrap, 6 ticks of feed_imu + push + advance.  Sessions 0 - 6 fly from a set state: 6 starts with readings more than 10 s
       old in its ring, 2 and 3 have a NIS gate that rejects, 5 has seen no image (it propagates only, with the offsets' reset, then steps with a closed
       reference gate).  Session 7 starts cold: the initialiser refuses it on quiet readings and accepts it after a jerk.  predict and predict_cov(full)
       before every advance at a time between the frames, after it at the frame's time and just past it.
 step: two hnet_filters_step calls on host windows.  Session 0 has a zero offset covariance and k_net_cov = 0 (S singular to the bit), session 1 an S
       whose first pivot is not on the diagonal; both get no readings in the first call, so that S is exactly what was set."""
import hashlib, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cuahn_vio_amd import _capi, weights
from cuahn_vio_amd.homography_net import HnetEngine, HnetFilters, HnetSessions

N, CAP, TICKS, RATE = 8, 64, 6, 0.005
SEL = [15, 16, 18, 19, 21, 22, 24, 25]                       # the rows of the state the measurement selects (hnet_ekf::update)


def frame_time(k):
    return 1.0 + 0.1 * k


class Hashes(dict):
    def add(self, kind, *arrays):
        h = self.setdefault(kind, hashlib.sha256())
        for a in arrays:
            h.update(np.ascontiguousarray(a).tobytes())


def state(rng, t):
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


def params(i):
    p = HnetFilters.default_params()
    p.imu_avg = 0 if i == 4 else 1
    p.cam_imu_dt = 0.001 * (i % 3)
    return p


def readings(rng, ts, noise):
    r = np.zeros(len(ts), _capi.IMU_DTYPE)
    r["t"] = ts
    r["wm"] = rng.standard_normal((len(ts), 3)) * 0.3 * noise
    r["am"] = rng.standard_normal((len(ts), 3)) * 0.5 * noise + [0, 0, 9.81]
    return r


def setup(blob, iters, rng):
    e = HnetEngine(blob, variant="prior3", mc_samples=16, dropout_p=0.05, mc_seed=9, max_batch=N)
    s = HnetSessions(e, N)
    f = HnetFilters(s, iters)
    base = rng.integers(0, 256, (224, 320), dtype=np.uint8)
    frames = np.stack([np.roll(base, (i % 7) - 3, axis=1) for i in range(11 + TICKS)])
    return e, s, f, frames


def fed(blob, iters, H):
    rng = np.random.default_rng(100 + iters)
    e, s, f, frames = setup(blob, iters, rng)
    ids = np.arange(N, dtype=np.int32)
    seen = np.array([0, 1, 2, 3, 4, 6], np.int32)
    for k in range(11):                                      # these have seen more than 10 images: the reference gate is open
        s.push(seen, np.repeat(frames[k][None], len(seen), 0), t=[frame_time(k)] * len(seen))
    f.enable_feed(CAP)
    f.enable_innovations()
    for i in ids[:7]:
        f.set_params(i, params(i))
        f.set_state(i, state(rng, frame_time(10)))
    f.set_nis_gate(2, 1e-3)
    f.set_nis_gate(3, 1e-3)
    ip = HnetFilters.default_init_params()
    ip.window_time, ip.imu_thresh, ip.init_height, ip.wait_for_jerk = 0.05, 0.5, 0.1, 1
    f.set_init_params(7, ip)
    old = readings(rng, 1.9 - 15.0 + RATE * np.arange(5), 1.0)          # more than 10 s behind the newest reading: trimmed, never selected
    f.feed_imu([6], [old])
    fed_to = 1.9
    for k in range(TICKS):
        tf = frame_time(11 + k)
        ts = np.arange(fed_to + RATE, tf + 0.0125, RATE)
        fed_to = ts[-1]
        per = []
        for i in ids:
            noise = np.ones(len(ts))
            if i == 7:                                       # quiet, then (tick 2 on) a jerk inside the newest initialiser window
                noise[:] = 0.01
                if k >= 2:
                    noise[ts > fed_to - 0.05] = 4.0
            per.append(readings(rng, ts, noise[:, None]))
        f.feed_imu(ids, per)
        for tq in (tf - 0.04,):
            H.add("predict", f.predict(ids, [tq] * N))
            H.add("predict_cov", *f.predict_cov(ids, [tq] * N, full=True))
        s.push(ids, np.repeat(frames[11 + k][None], N, 0), t=[tf] * N)
        out, net, upd, status = f.advance(ids)
        print(f"filters_out_hash iters={iters} tick {k}: status {status.tolist()} updates {upd.tolist()}")
        H.add("advance", out, net, upd, status)
        H.add("get_state", f.get_state(ids))
        n_s = int((status == _capi.ADV_STEPPED).sum())
        if n_s:
            H.add("last_priors", f.last_priors(n_s))
            H.add("last_innovations", f.last_innovations(n_s))
        for i in ids:
            H.add("last_selection", f.last_selection(i))
        for tq in (tf, tf + 0.006):
            H.add("predict", f.predict(ids, [tq] * N))
            H.add("predict_cov", *f.predict_cov(ids, [tq] * N, full=True))
    f.close(); s.close(); e.close()


def step(blob, iters, H):
    rng = np.random.default_rng(200 + iters)
    e, s, f, frames = setup(blob, iters, rng)
    ids = np.arange(N, dtype=np.int32)
    for k in range(12):
        s.push(ids, np.repeat(frames[k][None], N, 0), t=[frame_time(k)] * N)
    f.enable_innovations()
    f.set_nis_gate(2, 1e-3)
    for i in ids:
        p = params(i)
        st = state(rng, frame_time(10))
        if i == 0:                                           # S = 0 to the bit
            p.k_net_cov = 0.0
            st["cov"][0][15:, :] = 0.0
            st["cov"][0][:, 15:] = 0.0
        if i == 1:                                           # |S[1][0]| > |S[0][0]|: the first column's pivot is row 1
            p.k_net_cov = 0.0
            blk = np.diag(np.linspace(2e-4, 9e-4, 8))
            blk[0, 0], blk[0, 1], blk[1, 0] = 1e-5, 3e-4, 3e-4
            st["cov"][0][np.ix_(SEL, SEL)] = blk
        f.set_params(i, p)
        f.set_state(i, st)
    for k in range(2):
        tf = frame_time(11 + k)
        ts = np.arange(tf - 0.1 - 2 * RATE, tf + 2.5 * RATE, RATE)
        imu = [readings(rng, ts, 1.0)[:0 if (k == 0 and i < 2) else None] for i in ids]
        out, net, upd = f.step(ids, [tf] * N, imu)
        print(f"filters_out_hash iters={iters} step {k}: updates {upd.tolist()} flags {f.last_innovations(N)['flag'].tolist()}")
        H.add("step", out, net, upd)
        H.add("get_state", f.get_state(ids))
        H.add("last_priors", f.last_priors(N))
        H.add("last_innovations", f.last_innovations(N))
        if k == 0:
            s.push(ids, np.repeat(frames[12][None], N, 0), t=[frame_time(12)] * N)
    f.close(); s.close(); e.close()


blob = weights.pack_state_dict(weights.synthetic_state(0))
for iters in (1, 3):
    for name, run in (("fed", fed), ("step", step)):
        H = Hashes()
        run(blob, iters, H)
        for kind in sorted(H):
            print(f"filters_out_hash iters={iters} {name} {kind}: {H[kind].hexdigest()[:16]}")
