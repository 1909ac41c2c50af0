#!/usr/bin/env python3
"""Device filters (hnet_filters, include/hnet.h) against the host loop of INTEGRATION.md §6, in one process, over the replay fixture.
Per tick every one of K sessions pushes one frame and gets 16 IMU intervals of 2 ms; then
  device: one hnet_filters_step (propagation, max_iekf_iteration forwards + updates, reset; one synchronisation),
  host:   hnet_ekf::propagate_with_imu on T threads, then per iteration the priors, hnet_sessions_infer and hnet_ekf::update on T threads, then the
          reset (tests/cpp/filters_ref.cpp, built here with g++ -O2), on a second sessions object of the same blob.
One JSON line per (K, iterations): ticks/s and ms per tick of both (median, p10, p90 over the ticks), the step's device ms (upload .. last
update, HIP events).
--feed adds a third filters object on its own context that runs the same ticks through hnet_filters_feed_imu + hnet_filters_advance (rings of 256
readings): per tick the readings newer than the ring's newest are handed over once and one advance steps all K sessions; reported are the feed
call, the advance call and their sum, next to the step column of the same process and inputs (the step call's time includes packing K windows).
--iter-variant V (with --iter-mc N, --iter-p P) adds the IEKF's second model (hnet_sessions_set_iterative_model): a fourth filters object on its own
context whose sessions have an iterative engine of variant V attached, so its forwards 1 .. I-1 run on that model ("iter_step" columns, and
iter_over_main = its median over the device step's, which runs every iteration on the main model); the host loop then runs iterations > 0 through
hnet_sessions_infer_iter on an iterative engine attached to its sessions.
--predict is a mode of its own (hnet_filters_predict): one fed filters object per K with the same 16-interval ticks; per tick, once the
frame is pushed and the readings are fed, one predict of all K sessions to the frame's time (wall time of the call and the event time of its launch),
the host alternative on the same inputs (hnet_filters_get_state of the K sessions + hnet_ekf::propagate_mean_with_imu / odometry_from_state over a
host copy of the histories, tests/cpp/filters_predict_ref.cpp, on T threads), then the advance of the same sessions, which is the reference point.
--predict-cov is a mode beside --predict (hnet_filters_predict_cov) with the same ticks: per tick, once the frame is pushed and the readings
are fed, one predict_cov of all K sessions to the frame's time without and one with the full covariances (wall time of each call, event time of each
launch), one predict, the host alternative (hnet_filters_get_state + hnet_ekf::propagate_with_imu / odometry_from_state / odometry_cov_from_state over a
host copy of the histories, tests/cpp/filters_predict_cov_ref.cpp, on T threads), then the advance of the same sessions.
--innov is a mode of its own (innovation records and the NIS gate): per (K, iterations) three filters objects for hnet_filters_step and three
fed ones for hnet_filters_advance, each on its own context, with innovations off, on, and on with a gate that never rejects (1e300); every tick runs the
same inputs through all six in turn (the order rotates with the tick), reported are the wall time of the call and its event time.  "host_gated" is the host
path on one thread: filters_ref's propagation, then hnet_ekf::iterated_update_gated (tests/cpp/filters_innov_ref.cpp) around
hnet_sessions_infer, the prior of forward `it` being the one the header hands its network after the first `it` outputs.
   python tools/filters_bench.py [--k 1,8,64,256] [--iters 1,3] [--ticks 20] [--warmup 3] [--threads 1,16] [--feed]
                                 [--iter-variant prior1 --iter-mc 8 --iter-p 0.1]
   python tools/filters_bench.py --predict [--k 1,8,64,256] [--ticks 20] [--warmup 3] [--threads 1,16]
   python tools/filters_bench.py --predict-cov [--k 1,8,64,256] [--ticks 20] [--warmup 3] [--threads 1,16]
   python tools/filters_bench.py --innov [--k 1,8,64,256] [--iters 1,3] [--ticks 20] [--warmup 3]
--photo is a mode of its own (photometric residual records): step and advance with the records off and on, in one process on the same inputs.
   python tools/filters_bench.py --photo [--k 1,8,64,256] [--iters 1,3] [--ticks 20] [--warmup 3]
--photo-gate runs the same ticks with the photometric gate next to them: records off, records on, a gate that never rejects (max_ratio 1e30)
with the single-candidate launches reading img2 through LDS (pass) and from global memory (pass_global), and a gate that rejects every update.
   python tools/filters_bench.py --photo-gate [--k 1,8,64,256] [--iters 1,3] [--ticks 20] [--warmup 3]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build_ref():
    so = os.path.join(tempfile.mkdtemp(prefix="filters_ref_"), "filters_ref.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-shared", "-fPIC", "-pthread", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "filters_ref.cpp"), "-o", so], check=True)
    return C.CDLL(so)


def imu_window(rng, t0, n_int=16, dt=0.002):
    r = np.zeros(n_int + 2, np.dtype([("t", "<f8"), ("wm", "<f8", 3), ("am", "<f8", 3)]))
    r["t"] = t0 - 0.0005 + dt * np.arange(n_int + 2)
    r["wm"] = rng.standard_normal((n_int + 2, 3)) * 0.2
    r["am"] = rng.standard_normal((n_int + 2, 3)) * 0.3 + [0, 0, 9.81]
    return r


def predict_mode(a):
    from cuahn_vio_amd import _capi, replay, weights
    from cuahn_vio_amd.homography_net import HnetEngine, HnetFilters, HnetSessions
    so = os.path.join(tempfile.mkdtemp(prefix="filters_predict_ref_"), "filters_predict_ref.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-shared", "-fPIC", "-pthread", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "filters_predict_ref.cpp"), "-o", so], check=True)
    ref = C.CDLL(so)
    ref.pred_ref_predict_batch.restype = None
    blob = weights.pack_state_dict(weights.synthetic_state(0))
    fx = replay.load_fixture("indoor_forward_7")
    pool = np.stack([replay.render_frame(fx, 100 + j) for j in range(16)])
    threads = [int(x) for x in a.threads.split(",")]

    def pct(x, q):
        return round(float(np.percentile(x, q)), 3)

    for K in [int(x) for x in a.k.split(",")]:
        e = HnetEngine(blob, max_batch=K, variant="prior3", mc_samples=16, dropout_p=0.05, mc_seed=1)
        s = HnetSessions(e, K)
        f = HnetFilters(s, 1)
        f.enable_feed(256)
        f.last_predict_device_ms()                               # switches the predict's event timing on
        p = HnetFilters.default_params()
        params = (_capi.FilterParams * K)(*([p] * K))
        ids = np.arange(K, dtype=np.int32)
        st0 = np.zeros(1, _capi.FILTER_STATE_DTYPE)
        st0["q"] = [1, 0, 0, 0]
        st0["p"] = [0, 0, -1.0]
        st0["cov"] = np.diag(np.r_[np.full(15, 1e-3), np.full(12, 1e-6)])
        for i in range(K):
            f.set_state(i, st0[0])
        rng = np.random.default_rng(K)
        hist = np.zeros(0, _capi.IMU_DTYPE)                      # the host alternative's copy of one session's history (all K are fed the same)
        newest, t = -np.inf, 0.0
        pred_ms, pred_dev, adv_ms, adv_dev, host_ms = [], [], [], [], {T: [] for T in threads}
        for tick in range(a.warmup + a.ticks + 1):
            t_new = t + 0.0325
            s.push(ids, np.repeat(pool[tick % len(pool)][None], K, 0), t=[t_new] * K)
            win = imu_window(rng, t)
            new = win[win["t"] > newest]
            newest = float(new["t"][-1])
            f.feed_imu(ids, [new] * K)
            hist = np.concatenate([hist, new])[-256:]
            tq = np.full(K, t_new)
            t0 = time.perf_counter()
            o = f.predict(ids, tq)
            d = (time.perf_counter() - t0) * 1e3
            assert (o["status"] == _capi.PRED_OK).all() and (o["intervals"] == o["intervals"][0]).all(), (o["status"], o["intervals"])
            keep = tick > a.warmup
            if keep:
                pred_ms.append(d)
                pred_dev.append(f.last_predict_device_ms())
            imu = np.ascontiguousarray(np.tile(hist, K))
            off = (np.arange(K + 1) * len(hist)).astype(np.int64)
            for T in threads:
                out = np.zeros(K, _capi.ODOMETRY_DTYPE)
                t0 = time.perf_counter()
                st = f.get_state(ids)
                ref.pred_ref_predict_batch(C.c_void_p(st.ctypes.data), params, K, C.c_void_p(tq.ctypes.data), C.c_void_p(imu.ctypes.data),
                                           C.c_void_p(off.ctypes.data), T, C.c_void_p(out.ctypes.data))
                if keep:
                    host_ms[T].append((time.perf_counter() - t0) * 1e3)
                assert np.abs(out["p"] - o["p"]).max() < 1e-9 and (out["intervals"] == o["intervals"]).all()
            if tick > 0:                                          # (one image per session at tick 0: that advance propagates only)
                t0 = time.perf_counter()
                _, _, _, status = f.advance(ids)
                d = (time.perf_counter() - t0) * 1e3
                assert (status == _capi.ADV_STEPPED).all(), status
                if keep:
                    adv_ms.append(d)
                    adv_dev.append(f.last_timing()["device_ms"])
            else:
                f.advance(ids)
            t = t_new
        rec = {"K": K, "intervals": int(o["intervals"][0]), "ticks": len(pred_ms)}
        for name, v in (("predict_ms", pred_ms), ("predict_event_ms", pred_dev), ("advance_ms", adv_ms), ("advance_event_ms", adv_dev)):
            rec[f"{name}_p50"], rec[f"{name}_p10"], rec[f"{name}_p90"] = pct(v, 50), pct(v, 10), pct(v, 90)
        for T in threads:
            rec[f"host_predict_{T}t_ms_p50"], rec[f"host_predict_{T}t_ms_p10"], rec[f"host_predict_{T}t_ms_p90"] = (pct(host_ms[T], 50), pct(host_ms[T], 10),
                                                                                                               pct(host_ms[T], 90))
        rec["predict_over_advance"] = round(float(np.median(pred_ms)) / float(np.median(adv_ms)), 4)
        print(json.dumps(rec), flush=True)
        f.close(); s.close(); e.close()


def predict_cov_mode(a):
    from cuahn_vio_amd import _capi, replay, weights
    from cuahn_vio_amd.homography_net import HnetEngine, HnetFilters, HnetSessions
    so = os.path.join(tempfile.mkdtemp(prefix="filters_predict_cov_ref_"), "filters_predict_cov_ref.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-shared", "-fPIC", "-pthread", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "filters_predict_cov_ref.cpp"), "-o", so], check=True)
    ref = C.CDLL(so)
    ref.pcov_ref_predict_batch.restype = None
    blob = weights.pack_state_dict(weights.synthetic_state(0))
    fx = replay.load_fixture("indoor_forward_7")
    pool = np.stack([replay.render_frame(fx, 100 + j) for j in range(16)])
    threads = [int(x) for x in a.threads.split(",")]

    def pct(x, q):
        return round(float(np.percentile(x, q)), 3)

    for K in [int(x) for x in a.k.split(",")]:
        e = HnetEngine(blob, max_batch=K, variant="prior3", mc_samples=16, dropout_p=0.05, mc_seed=1)
        s = HnetSessions(e, K)
        f = HnetFilters(s, 1)
        f.enable_feed(256)
        f.last_predict_device_ms()                               # switches the event timing of both calls on
        f.last_predict_cov_device_ms()
        p = HnetFilters.default_params()
        params = (_capi.FilterParams * K)(*([p] * K))
        ids = np.arange(K, dtype=np.int32)
        st0 = np.zeros(1, _capi.FILTER_STATE_DTYPE)
        st0["q"] = [1, 0, 0, 0]
        st0["p"] = [0, 0, -1.0]
        st0["cov"] = np.diag(np.r_[np.full(15, 1e-3), np.full(12, 1e-6)])
        for i in range(K):
            f.set_state(i, st0[0])
        rng = np.random.default_rng(K)
        hist = np.zeros(0, _capi.IMU_DTYPE)                      # the host alternative's copy of one session's history (all K are fed the same)
        newest, t = -np.inf, 0.0
        names = ("predict_cov_ms", "predict_cov_event_ms", "predict_cov_full_ms", "predict_cov_full_event_ms", "predict_ms", "predict_event_ms", "advance_ms",
                 "advance_event_ms")
        v = {k: [] for k in names}
        host_ms = {T: [] for T in threads}
        for tick in range(a.warmup + a.ticks + 1):
            t_new = t + 0.0325
            s.push(ids, np.repeat(pool[tick % len(pool)][None], K, 0), t=[t_new] * K)
            win = imu_window(rng, t)
            new = win[win["t"] > newest]
            newest = float(new["t"][-1])
            f.feed_imu(ids, [new] * K)
            hist = np.concatenate([hist, new])[-256:]
            tq = np.full(K, t_new)
            keep = tick > a.warmup
            t0 = time.perf_counter()
            o, oc = f.predict_cov(ids, tq)
            d = (time.perf_counter() - t0) * 1e3
            d_ev = f.last_predict_cov_device_ms()
            t0 = time.perf_counter()
            o2, oc2, full = f.predict_cov(ids, tq, full=True)
            d_full = (time.perf_counter() - t0) * 1e3
            d_full_ev = f.last_predict_cov_device_ms()
            t0 = time.perf_counter()
            o3 = f.predict(ids, tq)
            d_pred = (time.perf_counter() - t0) * 1e3
            assert (o["status"] == _capi.PRED_OK).all() and (o["intervals"] == o["intervals"][0]).all(), (o["status"], o["intervals"])
            assert o.tobytes() == o2.tobytes() == o3.tobytes() and oc.tobytes() == oc2.tobytes()
            if keep:
                for k, x in zip(names[:6], (d, d_ev, d_full, d_full_ev, d_pred, f.last_predict_device_ms())):
                    v[k].append(x)
            imu = np.ascontiguousarray(np.tile(hist, K))
            off = (np.arange(K + 1) * len(hist)).astype(np.int64)
            for T in threads:
                out, cov, hfull = np.zeros(K, _capi.ODOMETRY_DTYPE), np.zeros(K, _capi.ODOMETRY_COV_DTYPE), np.zeros((K, 27, 27))
                t0 = time.perf_counter()
                st = f.get_state(ids)
                ref.pcov_ref_predict_batch(C.c_void_p(st.ctypes.data), params, K, C.c_void_p(tq.ctypes.data), C.c_void_p(imu.ctypes.data),
                                           C.c_void_p(off.ctypes.data), T, C.c_void_p(out.ctypes.data), C.c_void_p(cov.ctypes.data), C.c_void_p(hfull.ctypes.data))
                if keep:
                    host_ms[T].append((time.perf_counter() - t0) * 1e3)
                assert np.abs(out["p"] - o["p"]).max() < 1e-9 and (out["intervals"] == o["intervals"]).all()
                assert np.abs(hfull - full).max() <= 1e-10 * np.abs(hfull).max()
            if tick > 0:                                          # (one image per session at tick 0: that advance propagates only)
                t0 = time.perf_counter()
                sta, _, _, status = f.advance(ids)
                d = (time.perf_counter() - t0) * 1e3
                assert (status == _capi.ADV_STEPPED).all(), status
                if keep:
                    v["advance_ms"].append(d)
                    v["advance_event_ms"].append(f.last_timing()["device_ms"])
            else:
                f.advance(ids)
            t = t_new
        rec = {"K": K, "intervals": int(o["intervals"][0]), "ticks": len(v["predict_ms"])}
        for name in names:
            rec[f"{name}_p50"], rec[f"{name}_p10"], rec[f"{name}_p90"] = pct(v[name], 50), pct(v[name], 10), pct(v[name], 90)
        for T in threads:
            rec[f"host_predict_cov_{T}t_ms_p50"], rec[f"host_predict_cov_{T}t_ms_p10"], rec[f"host_predict_cov_{T}t_ms_p90"] = (
                pct(host_ms[T], 50), pct(host_ms[T], 10), pct(host_ms[T], 90))
        med = {k: float(np.median(x)) for k, x in v.items()}
        rec["predict_cov_over_predict"] = round(med["predict_cov_ms"] / med["predict_ms"], 4)
        rec["predict_cov_over_advance"] = round(med["predict_cov_ms"] / med["advance_ms"], 4)
        rec["predict_cov_full_over_advance"] = round(med["predict_cov_full_ms"] / med["advance_ms"], 4)
        rec["predict_cov_event_us_per_interval"] = round(1e3 * med["predict_cov_event_ms"] / max(rec["intervals"], 1), 3)
        print(json.dumps(rec), flush=True)
        f.close(); s.close(); e.close()


def innov_mode(a):
    from cuahn_vio_amd import _capi, replay, weights
    from cuahn_vio_amd.homography_net import HnetEngine, HnetFilters, HnetSessions
    ref = build_ref()
    so = os.path.join(tempfile.mkdtemp(prefix="filters_innov_ref_"), "filters_innov_ref.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-shared", "-fPIC", "-pthread", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "filters_innov_ref.cpp"), "-o", so], check=True)
    iref = C.CDLL(so)
    iref.innov_ref_step.restype = None
    blob = weights.pack_state_dict(weights.synthetic_state(0))
    fx = replay.load_fixture("indoor_forward_7")
    pool = np.stack([replay.render_frame(fx, 100 + j) for j in range(16)])
    kw = dict(variant="prior3", mc_samples=16, dropout_p=0.05, mc_seed=1)
    modes = ("off", "on", "gate")

    def pct(x, q):
        return round(float(np.percentile(x, q)), 3)

    for K in [int(x) for x in a.k.split(",")]:
        for iters in [int(x) for x in a.iters.split(",")]:
            p = HnetFilters.default_params()
            params = (_capi.FilterParams * K)(*([p] * K))
            ids = np.arange(K, dtype=np.int32)
            st0 = np.zeros(1, _capi.FILTER_STATE_DTYPE)
            st0["q"] = [1, 0, 0, 0]
            st0["p"] = [0, 0, -1.0]
            st0["cov"] = np.diag(np.r_[np.full(15, 1e-3), np.full(12, 1e-6)])
            objs = {}
            for kind in ("step", "advance"):
                for m in modes:
                    e = HnetEngine(blob, max_batch=K, **kw)
                    s = HnetSessions(e, K)
                    f = HnetFilters(s, iters)
                    if m != "off":
                        f.enable_innovations()
                    if kind == "advance":
                        f.enable_feed(256)
                    for i in range(K):
                        f.set_state(i, st0[0])
                        if m == "gate":
                            f.set_nis_gate(i, 1e300)
                    objs[kind, m] = (e, s, f)
            eh = HnetEngine(blob, max_batch=K, **kw)
            sh = HnetSessions(eh, K)
            host = np.repeat(st0, K)
            rng = np.random.default_rng(K)
            wall = {k: [] for k in objs}
            event = {k: [] for k in objs}
            host_ms, rejected, nis = [], 0, []
            newest, t = -np.inf, 0.0
            order = list(objs)
            for tick in range(a.warmup + a.ticks):
                t_new = t + 0.0325
                fr = np.repeat(pool[tick % len(pool)][None], K, 0)
                for (_, s, _) in list(objs.values()) + [(None, sh, None)]:
                    s.push(ids, fr, t=[t_new] * K)
                win = imu_window(rng, t)
                new = win[win["t"] > newest]
                newest = float(new["t"][-1])
                for m in modes:
                    objs["advance", m][2].feed_imu(ids, [new] * K)
                keep = tick > a.warmup
                for key in order[tick % len(order):] + order[:tick % len(order)]:
                    f = objs[key][2]
                    if key[0] == "step" and tick == 0:              # one image per session so far: nothing to step
                        continue
                    t0 = time.perf_counter()
                    if key[0] == "step":
                        f.step(ids, [t_new] * K, [win] * K)
                    else:
                        status = f.advance(ids)[3]
                    d = (time.perf_counter() - t0) * 1e3
                    if key[0] == "advance" and tick > 0:
                        assert (status == _capi.ADV_STEPPED).all(), status
                    if keep:
                        wall[key].append(d)
                        event[key].append(f.last_timing()["device_ms"])
                    if keep and key == ("step", "gate"):
                        r = f.last_innovations(K)
                        rejected += int((r["flag"] == _capi.INNOV_REJECTED).sum())
                        nis += [float(x) for x in r["nis"][r["flag"] == _capi.INNOV_USED]]
                if tick > 0:
                    imu = np.ascontiguousarray(np.tile(win, K))
                    off = (np.arange(K + 1) * len(win)).astype(np.int64)
                    tf = np.full(K, t_new)
                    t0 = time.perf_counter()
                    ref.ref_propagate_batch(C.c_void_p(host.ctypes.data), params, K, C.c_void_p(tf.ctypes.data), C.c_void_p(imu.ctypes.data),
                                            C.c_void_p(off.ctypes.data), 1)
                    gate = np.array([int(sh.latest_time(j) == t_new and sh.image_count(j) > 10) for j in range(K)], np.int32)
                    mx = np.full(K, 1e300)
                    net = np.zeros((iters, K, 72), np.float32)
                    rec = np.zeros((iters, K), _capi.INNOVATION_DTYPE)
                    upd = np.zeros(K, np.int32)
                    pri = np.zeros((iters, K, 8))
                    for it in range(iters + 1):                     # pass `it` < iters yields the prior of forward `it`; the last pass commits
                        iref.innov_ref_step(C.c_void_p(host.ctypes.data), params, K, iters, C.c_void_p(net.ctypes.data), C.c_void_p(gate.ctypes.data),
                                            C.c_void_p(mx.ctypes.data), C.c_void_p(rec.ctypes.data), C.c_void_p(upd.ctypes.data),
                                            C.c_void_p(pri.ctypes.data), int(it == iters))
                        if it < iters:
                            mean, cov = sh.infer(ids, np.ascontiguousarray(pri[it]))
                            net[it, :, :8], net[it, :, 8:] = mean, cov.reshape(K, 64)
                    if keep:
                        host_ms.append((time.perf_counter() - t0) * 1e3)
                t = t_new
            out = {"K": K, "max_iekf_iteration": iters, "intervals": 16, "ticks": len(wall["step", "off"]),
                   "record_bytes_per_call": _capi.INNOVATION_DTYPE.itemsize * iters * K}
            for (kind, m), v in wall.items():
                out[f"{kind}_{m}_ms_p50"], out[f"{kind}_{m}_ms_p10"], out[f"{kind}_{m}_ms_p90"] = pct(v, 50), pct(v, 10), pct(v, 90)
                ev = event[kind, m]
                out[f"{kind}_{m}_event_ms_p50"], out[f"{kind}_{m}_event_ms_p10"], out[f"{kind}_{m}_event_ms_p90"] = pct(ev, 50), pct(ev, 10), pct(ev, 90)
            for kind in ("step", "advance"):
                for m in ("on", "gate"):
                    out[f"{kind}_{m}_minus_off_event_us"] = round(1e3 * (float(np.median(event[kind, m])) - float(np.median(event[kind, "off"]))), 1)
            out["host_gated_1t_ms_p50"], out["host_gated_1t_ms_p10"], out["host_gated_1t_ms_p90"] = pct(host_ms, 50), pct(host_ms, 10), pct(host_ms, 90)
            out["rejected"], out["mean_nis_used"] = rejected, (round(float(np.mean(nis)), 4) if nis else None)
            print(json.dumps(out), flush=True)
            for (e, s, f) in objs.values():
                f.close(); s.close(); e.close()
            sh.close(); eh.close()


def photo_mode(a, gate=False):
    """photometric residual records: per (K, iterations) two filters objects for hnet_filters_step and two fed ones for hnet_filters_advance, each
    on its own context, with the records off and on; every tick runs all four on the same frames and IMU window, in rotating order.  The records are
    launched behind the event that closes hnet_filters_last_timing's window, so the wall time of the call (it ends in the call's synchronisation) is the
    figure that contains them; the event time shows that the window itself did not move.
    gate: three more objects per call - every session with a gate of max_ratio 1e30 (never rejects; the records are then formed per iteration,
    inside the window) in both tap forms, and with a gate of 1e-30 (every estimate whose reference gate is open is refused at iteration 0)."""
    from cuahn_vio_amd import _capi, replay, weights
    from cuahn_vio_amd.homography_net import HnetEngine, HnetFilters, HnetSessions
    blob = weights.pack_state_dict(weights.synthetic_state(0))
    fx = replay.load_fixture("indoor_forward_7")
    pool = np.stack([replay.render_frame(fx, 100 + j) for j in range(16)])
    kw = dict(variant="prior3", mc_samples=16, dropout_p=0.05, mc_seed=1)
    modes = ("off", "on", "pass", "pass_global", "reject") if gate else ("off", "on")
    ratio = {"pass": 1e30, "pass_global": 1e30, "reject": 1e-30}

    def pct(x, q):
        return round(float(np.percentile(x, q)), 3)

    for K in [int(x) for x in a.k.split(",")]:
        for iters in [int(x) for x in a.iters.split(",")]:
            ids = np.arange(K, dtype=np.int32)
            st0 = np.zeros(1, _capi.FILTER_STATE_DTYPE)
            st0["q"] = [1, 0, 0, 0]
            st0["p"] = [0, 0, -1.0]
            st0["cov"] = np.diag(np.r_[np.full(15, 1e-3), np.full(12, 1e-6)])
            objs = {}
            for kind in ("step", "advance"):
                for m in modes:
                    e = HnetEngine(blob, max_batch=K, **kw)
                    s = HnetSessions(e, K)
                    f = HnetFilters(s, iters)
                    if m != "off":
                        f.enable_photometric()
                    if m in ratio:
                        f.set_photo_gate_taps(m == "pass_global")
                        for i in range(K):
                            f.set_photo_gate(i, ratio[m])
                    if kind == "advance":
                        f.enable_feed(256)
                    for i in range(K):
                        f.set_state(i, st0[0])
                    objs[kind, m] = (e, s, f)
            rng = np.random.default_rng(K)
            wall = {k: [] for k in objs}
            event = {k: [] for k in objs}
            res = []
            newest, t = -np.inf, 0.0
            order = list(objs)
            for tick in range(a.warmup + a.ticks):
                t_new = t + 0.0325
                fr = np.repeat(pool[tick % len(pool)][None], K, 0)
                for (_, s, _) in objs.values():
                    s.push(ids, fr, t=[t_new] * K)
                win = imu_window(rng, t)
                new = win[win["t"] > newest]
                newest = float(new["t"][-1])
                for m in modes:
                    objs["advance", m][2].feed_imu(ids, [new] * K)
                keep = tick > a.warmup
                for key in order[tick % len(order):] + order[:tick % len(order)]:
                    f = objs[key][2]
                    if key[0] == "step" and tick == 0:              # one image per session so far: nothing to step
                        continue
                    t0 = time.perf_counter()
                    if key[0] == "step":
                        f.step(ids, [t_new] * K, [win] * K)
                    else:
                        status = f.advance(ids)[3]
                    d = (time.perf_counter() - t0) * 1e3
                    if key[0] == "advance" and tick > 0:
                        assert (status == _capi.ADV_STEPPED).all(), status
                    if keep:
                        wall[key].append(d)
                        event[key].append(f.last_timing()["device_ms"])
                    if keep and key == ("step", "on"):
                        r = f.last_photometric(K)
                        res.append((r["sum_inside"] / np.maximum(r["n_inside"], 1)).mean(axis=0))
                t = t_new
            out = {"K": K, "max_iekf_iteration": iters, "intervals": 16, "ticks": len(wall["step", "off"]), "candidates": 2 + iters,
                   "record_bytes_per_call": _capi.PHOTO_RESIDUAL_DTYPE.itemsize * (2 + iters) * K}
            for (kind, m), v in wall.items():
                out[f"{kind}_{m}_ms_p50"], out[f"{kind}_{m}_ms_p10"], out[f"{kind}_{m}_ms_p90"] = pct(v, 50), pct(v, 10), pct(v, 90)
                ev = event[kind, m]
                out[f"{kind}_{m}_event_ms_p50"], out[f"{kind}_{m}_event_ms_p10"], out[f"{kind}_{m}_event_ms_p90"] = pct(ev, 50), pct(ev, 10), pct(ev, 90)
            for kind in ("step", "advance"):
                out[f"{kind}_on_minus_off_wall_us"] = round(1e3 * (float(np.median(wall[kind, "on"])) - float(np.median(wall[kind, "off"]))), 1)
            if gate:
                for kind in ("step", "advance"):
                    on = float(np.median(wall[kind, "on"]))
                    for m in ("pass", "pass_global", "reject"):
                        out[f"{kind}_{m}_minus_on_wall_us"] = round(1e3 * (float(np.median(wall[kind, m])) - on), 1)
                out["rejected_per_session"] = {m: objs["step", m][2].photo_stats(0)["rejected"] for m in ("on", "pass", "reject")}
                out["judged_per_session"] = {m: objs["step", m][2].photo_stats(0)["judged"] for m in ("on", "pass", "reject")}
            out["mean_inside_residual_identity_prior_estimates"] = [round(float(x), 3) for x in np.mean(res, axis=0)]
            print(json.dumps(out), flush=True)
            for (e, s, f) in objs.values():
                f.close(); s.close(); e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", default="1,8,64,256")
    ap.add_argument("--iters", default="1,3")
    ap.add_argument("--ticks", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--threads", default="1,16")
    ap.add_argument("--feed", action="store_true")
    ap.add_argument("--predict", action="store_true")
    ap.add_argument("--predict-cov", action="store_true")
    ap.add_argument("--innov", action="store_true")
    ap.add_argument("--photo", action="store_true")
    ap.add_argument("--photo-gate", action="store_true")
    ap.add_argument("--iter-variant", default=None)
    ap.add_argument("--iter-mc", type=int, default=8)
    ap.add_argument("--iter-p", type=float, default=0.1)
    a = ap.parse_args()
    if a.predict:
        return predict_mode(a)
    if a.predict_cov:
        return predict_cov_mode(a)
    if a.innov:
        return innov_mode(a)
    if a.photo or a.photo_gate:
        return photo_mode(a, gate=a.photo_gate)
    from cuahn_vio_amd import _capi, replay, weights
    from cuahn_vio_amd.homography_net import HnetEngine, HnetFilters, HnetSessions
    ref = build_ref()
    blob = weights.pack_state_dict(weights.synthetic_state(0))
    fx = replay.load_fixture("indoor_forward_7")
    pool = np.stack([replay.render_frame(fx, 100 + j) for j in range(16)])
    threads = [int(x) for x in a.threads.split(",")]
    kw = dict(variant="prior3", mc_samples=16, dropout_p=0.05, mc_seed=1)
    for K in [int(x) for x in a.k.split(",")]:
        for iters in [int(x) for x in a.iters.split(",")]:
            e1, e2 = HnetEngine(blob, max_batch=K, **kw), HnetEngine(blob, max_batch=K, **kw)
            s1, s2 = HnetSessions(e1, K), HnetSessions(e2, K)
            f = HnetFilters(s1, iters)
            p = HnetFilters.default_params()
            params = (_capi.FilterParams * K)(*([p] * K))
            ids = np.arange(K, dtype=np.int32)
            st0 = np.zeros(1, _capi.FILTER_STATE_DTYPE)
            st0["q"] = [1, 0, 0, 0]
            st0["p"] = [0, 0, -1.0]
            st0["cov"] = np.diag(np.r_[np.full(15, 1e-3), np.full(12, 1e-6)])
            for i in range(K):
                f.set_state(i, st0[0])
            hosts = {T: np.repeat(st0, K) for T in threads}
            if a.iter_variant:
                ikw = dict(variant=a.iter_variant, mc_samples=a.iter_mc, dropout_p=a.iter_p, mc_seed=kw["mc_seed"], max_batch=K)
                e4, ei4, ei2 = HnetEngine(blob, max_batch=K, **kw), HnetEngine(blob, **ikw), HnetEngine(blob, **ikw)
                s4 = HnetSessions(e4, K)
                s4.set_iterative_model(ei4)
                s2.set_iterative_model(ei2)
                f4 = HnetFilters(s4, iters)
                for i in range(K):
                    f4.set_state(i, st0[0])
                it_ms, it_dev = [], []
            if a.feed:
                e3 = HnetEngine(blob, max_batch=K, **kw)
                s3 = HnetSessions(e3, K)
                f3 = HnetFilters(s3, iters)
                f3.enable_feed(256)
                for i in range(K):
                    f3.set_state(i, st0[0])
                newest, feed_ms, adv_ms, adv_dev = -np.inf, [], [], []
            rng = np.random.default_rng(K)
            dev_ms, dev_dev, host_ms = [], [], {T: [] for T in threads}
            t = 0.0
            for tick in range(a.warmup + a.ticks):
                t_new = t + 0.0325
                fr = np.repeat(pool[tick % len(pool)][None], K, 0)
                for s in (s1, s2) + ((s4,) if a.iter_variant else ()):
                    s.push(ids, fr, t=[t_new] * K)
                win = imu_window(rng, t)
                if a.feed:
                    s3.push(ids, fr, t=[t_new] * K)
                    new = win[win["t"] > newest]                # the windows of consecutive ticks overlap: a reading is handed over once
                    newest = float(new["t"][-1])
                    t0 = time.perf_counter()
                    f3.feed_imu(ids, [new] * K)
                    t1 = time.perf_counter()
                    if tick > 0:
                        _, _, _, status = f3.advance(ids)
                        t2 = time.perf_counter()
                        assert (status == _capi.ADV_STEPPED).all(), status
                        if tick > a.warmup:
                            feed_ms.append((t1 - t0) * 1e3)
                            adv_ms.append((t2 - t1) * 1e3)
                            adv_dev.append(f3.last_timing()["device_ms"])
                if tick == 0:                                   # one image per session so far: nothing to step
                    t = t_new
                    continue
                t0 = time.perf_counter()
                f.step(ids, [t_new] * K, [win] * K)
                d = (time.perf_counter() - t0) * 1e3
                if tick > a.warmup:
                    dev_ms.append(d)
                    dev_dev.append(f.last_timing()["device_ms"])
                if a.iter_variant:
                    t0 = time.perf_counter()
                    f4.step(ids, [t_new] * K, [win] * K)
                    d = (time.perf_counter() - t0) * 1e3
                    if tick > a.warmup:
                        it_ms.append(d)
                        it_dev.append(f4.last_timing()["device_ms"])
                imu = np.ascontiguousarray(np.tile(win, K))
                off = (np.arange(K + 1) * len(win)).astype(np.int64)
                tf = np.full(K, t_new)
                for T in threads:
                    h = hosts[T]
                    t0 = time.perf_counter()
                    ref.ref_propagate_batch(C.c_void_p(h.ctypes.data), params, K, C.c_void_p(tf.ctypes.data), C.c_void_p(imu.ctypes.data),
                                            C.c_void_p(off.ctypes.data), T)
                    gate = np.array([int(s2.latest_time(j) == t_new and s2.image_count(j) > 10) for j in range(K)], np.int32)
                    for it in range(iters):
                        prior_px = h["offset"][:, :, :2].reshape(K, 8) * 159.5
                        prior_cam = np.ascontiguousarray(h["offset"][:, :, :2].reshape(K, 8))
                        mean, cov = s2.infer(ids, prior_px, iteration=it) if a.iter_variant else s2.infer(ids, prior_px)
                        ref.ref_update_batch(C.c_void_p(h.ctypes.data), params, K, C.c_void_p(mean.ctypes.data), C.c_void_p(cov.ctypes.data),
                                             C.c_void_p(prior_cam.ctypes.data), C.c_void_p(gate.ctypes.data), int(it != iters - 1), T)
                    ref.ref_reset_batch(C.c_void_p(h.ctypes.data), K)
                    if tick > a.warmup:
                        host_ms[T].append((time.perf_counter() - t0) * 1e3)
                t = t_new
            def pct(x, q):
                return round(float(np.percentile(x, q)), 3)
            rec = {"K": K, "max_iekf_iteration": iters, "intervals": 16, "ticks": len(dev_ms),
                   "device_step_ms_p50": pct(dev_ms, 50), "device_step_ms_p10": pct(dev_ms, 10), "device_step_ms_p90": pct(dev_ms, 90),
                   "device_step_ticks_per_s": round(1e3 / float(np.median(dev_ms)), 1),
                   "device_step_event_ms_p50": pct(dev_dev, 50), "device_step_event_ms_p10": pct(dev_dev, 10), "device_step_event_ms_p90": pct(dev_dev, 90)}
            for T in threads:
                m = float(np.median(host_ms[T]))
                rec[f"host_loop_{T}t_ms_p50"] = round(m, 3)
                rec[f"host_loop_{T}t_ms_p10"] = pct(host_ms[T], 10)
                rec[f"host_loop_{T}t_ms_p90"] = pct(host_ms[T], 90)
                rec[f"host_loop_{T}t_ticks_per_s"] = round(1e3 / m, 1)
            if a.iter_variant:
                rec["iter_model"] = f"{a.iter_variant} N={a.iter_mc} p={a.iter_p:g}"
                for name, v in (("iter_step_ms", it_ms), ("iter_step_event_ms", it_dev)):
                    rec[f"{name}_p50"], rec[f"{name}_p10"], rec[f"{name}_p90"] = pct(v, 50), pct(v, 10), pct(v, 90)
                rec["iter_over_main"] = round(float(np.median(it_ms)) / float(np.median(dev_ms)), 3)
                f4.close(); s4.close(); ei4.close(); e4.close()
            if a.feed:
                tot = [x + y for x, y in zip(feed_ms, adv_ms)]
                for name, v in (("feed_imu_ms", feed_ms), ("advance_ms", adv_ms), ("feed_tick_ms", tot), ("advance_event_ms", adv_dev)):
                    rec[f"{name}_p50"], rec[f"{name}_p10"], rec[f"{name}_p90"] = pct(v, 50), pct(v, 10), pct(v, 90)
                rec["feed_tick_over_step"] = round(float(np.median(tot)) / float(np.median(dev_ms)), 3)
                f3.close(); s3.close(); e3.close()
            print(json.dumps(rec), flush=True)
            f.close(); s1.close(); s2.close(); e1.close(); e2.close()
            if a.iter_variant:
                ei2.close()


if __name__ == "__main__":
    main()
