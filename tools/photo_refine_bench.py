"""The cost of the photometric fallback of hnet_filters (include/hnet.h hnet_filters_set_photo_refine): hnet_filters_step of K sessions,
max_iekf_iteration 3, 16 IMU intervals, on rendered frames of the replay fixture, alignment options levels = 3 and 6 trials; medians over --ticks ticks
after --warmup.  Per K, in one process on the same inputs, in rotating order:
  gated        every session under a photometric gate that never refuses (max_ratio 1e30), refinement off: the tick this API must leave alone
  idle         the same with refinement on for every session: nothing is refused, the always-enqueued launch sequence runs on NaN starts
  one_in_8     refinement on, every eighth session's gate refuses everything (max_ratio 1e-30): that session falls back
  operator     what an operator has without the API for the same one in eight: the gated step, then hnet_sessions_photo_align_robust on the refused
               sessions from hnet_filters_last_priors, hnet_filters_get_state, the host header's measurement and update
               (tests/cpp/filters_photo_refine_ref.cpp), hnet_filters_set_state - a second synchronisation and a state round trip
Reported: wall time of the call(s) and hnet_filters_last_timing's device window.
   python tools/photo_refine_bench.py [--k 8,64] [--ticks 40] [--warmup 5] [--modes gated,idle,one_in_8,operator]
--modes gated uses nothing this API added: with HNET_PY_ROOT naming the python tree of another commit and HNET_LIB_PATH its library (or this tree's) it
is the A/B of the untouched path."""
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
sys.path.insert(0, os.environ.get("HNET_PY_ROOT") or ROOT)


def build_refine_ref():
    so = os.path.join(tempfile.mkdtemp(prefix="filters_photo_refine_ref_"), "filters_photo_refine_ref.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-pthread", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "filters_photo_refine_ref.cpp"), "-o", so], check=True)
    return C.CDLL(so)


def imu_window(rng, t0, n_int=16, dt=0.002):
    r = np.zeros(n_int + 2, np.dtype([("t", "<f8"), ("wm", "<f8", 3), ("am", "<f8", 3)]))
    r["t"] = t0 - 0.0005 + dt * np.arange(n_int + 2)
    r["wm"] = rng.standard_normal((n_int + 2, 3)) * 0.2
    r["am"] = rng.standard_normal((n_int + 2, 3)) * 0.3 + [0, 0, 9.81]
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", default="8,64")
    ap.add_argument("--ticks", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--modes", default="gated,idle,one_in_8,operator")
    ap.add_argument("--levels", type=int, default=3)
    ap.add_argument("--trials", type=int, default=6)
    a = ap.parse_args()
    from cuahn_vio_amd import _capi, replay, weights
    from cuahn_vio_amd.homography_net import HnetEngine, HnetFilters, HnetSessions
    modes = a.modes.split(",")
    iters = 3
    blob = weights.pack_state_dict(weights.synthetic_state(0))
    fx = replay.load_fixture("indoor_forward_7")
    pool = np.stack([replay.render_frame(fx, 100 + j) for j in range(16)])
    kw = dict(variant="prior3", mc_samples=16, dropout_p=0.05, mc_seed=1)
    rref = build_refine_ref() if "operator" in modes else None

    def pct(x, q):
        return round(float(np.percentile(x, q)), 3)

    for K in [int(x) for x in a.k.split(",")]:
        ids = np.arange(K, dtype=np.int32)
        refused = np.arange(0, K, 8, dtype=np.int32)
        st0 = np.zeros(1, _capi.FILTER_STATE_DTYPE)
        st0["q"] = [1, 0, 0, 0]
        st0["p"] = [0, 0, -1.0]
        st0["cov"] = np.diag(np.r_[np.full(15, 1e-3), np.full(12, 1e-6)])
        params = HnetFilters.default_params()
        objs = {}
        for m in modes:
            e = HnetEngine(blob, max_batch=K, **kw)
            s = HnetSessions(e, K)
            f = HnetFilters(s, iters)
            f.enable_photometric()
            for i in range(K):
                f.set_photo_gate(i, 1e-30 if m in ("one_in_8", "operator") and i % 8 == 0 else 1e30)
                f.set_state(i, st0[0])
            if m in ("idle", "one_in_8"):
                o = _capi.photo_refine_opts(levels=a.levels, max_iterations=a.trials, cov_scale=4.0)
                for i in range(K):
                    f.set_photo_refine(i, o)
            objs[m] = (e, s, f)
        oo = _capi.photo_refine_opts(levels=a.levels, max_iterations=a.trials, cov_scale=4.0) if "operator" in modes else None
        rng = np.random.default_rng(K)
        wall = {m: [] for m in modes}
        event = {m: [] for m in modes}
        flags = []
        t = 0.0
        for tick in range(a.warmup + a.ticks + 11):                      # (the reference gate opens after image 10: the ticks before it are not kept)
            t_new = t + 0.0325
            fr = np.repeat(pool[tick % len(pool)][None], K, 0)
            for (_, s, _) in objs.values():
                s.push(ids, fr, t=[t_new] * K)
            win = imu_window(rng, t)
            keep = tick >= a.warmup + 11
            for m in modes[tick % len(modes):] + modes[:tick % len(modes)]:
                e, s, f = objs[m]
                if tick == 0:                                             # one image per session so far: nothing to step
                    continue
                t0 = time.perf_counter()
                f.step(ids, [t_new] * K, [win] * K)
                ev = f.last_timing()["device_ms"]
                if m == "operator" and tick > 10:
                    pri = f.last_priors(K)[0][refused]
                    rec, lv = s.photo_align_robust(refused, pri, levels=a.levels, want_levels=True, max_iterations=a.trials)
                    st = f.get_state(refused)
                    for k, i in enumerate(refused):
                        m72, r_px, fl = np.zeros(72, np.float32), np.zeros(64), C.c_int32(0)
                        one = np.ascontiguousarray(rec[k]).reshape(1)
                        if rref.photo_refine_ref_measurement(C.c_void_p(one.ctypes.data), int(lv[k]["px"]["accepted"].sum()), C.byref(oo), C.c_double(params.k_net_cov),
                                                             C.c_void_p(m72.ctypes.data), C.c_void_p(r_px.ctypes.data), C.byref(fl)):
                            # (the refused state's offsets were reset with the step; the update is made on what the operator can still reach)
                            one_st = np.ascontiguousarray(st[k]).reshape(1)
                            rref.photo_refine_ref_update(C.c_void_p(one_st.ctypes.data), C.byref(params), C.c_void_p(m72.ctypes.data), 0, 1)
                            f.set_state(int(i), one_st[0])
                d = (time.perf_counter() - t0) * 1e3
                if keep:
                    wall[m].append(d)
                    event[m].append(ev)
                if keep and m == "one_in_8":
                    flags.append(f.last_refine(K)["flags"].copy())
            t = t_new
        out = {"K": K, "max_iekf_iteration": iters, "intervals": 16, "levels": a.levels, "trials": a.trials, "ticks": len(wall[modes[0]])}
        for m in modes:
            out[f"{m}_ms_p50"], out[f"{m}_ms_p10"], out[f"{m}_ms_p90"] = pct(wall[m], 50), pct(wall[m], 10), pct(wall[m], 90)
            out[f"{m}_event_ms_p50"], out[f"{m}_event_ms_p10"], out[f"{m}_event_ms_p90"] = pct(event[m], 50), pct(event[m], 10), pct(event[m], 90)
        if "gated" in modes and "idle" in modes:
            g, i_ = float(np.median(wall["gated"])), float(np.median(wall["idle"]))
            out["idle_minus_gated_ms"] = round(i_ - g, 3)
            out["idle_share_of_gated_tick"] = round((i_ - g) / g, 3)
        if "one_in_8" in modes and "idle" in modes:
            out["one_in_8_minus_idle_ms"] = round(float(np.median(wall["one_in_8"])) - float(np.median(wall["idle"])), 3)
        if "one_in_8" in modes and "operator" in modes:
            out["operator_minus_one_in_8_ms"] = round(float(np.median(wall["operator"])) - float(np.median(wall["one_in_8"])), 3)
        if flags:
            fl = np.stack(flags)
            out["one_in_8_asked_per_tick"] = round(float((fl & 1).astype(bool).sum(axis=1).mean()), 2)
            out["one_in_8_applied_per_tick"] = round(float((fl & 2).astype(bool).sum(axis=1).mean()), 2)
        print(json.dumps(out), flush=True)
        for (e, s, f) in objs.values():
            f.close(); s.close(); e.close()


if __name__ == "__main__":
    main()
