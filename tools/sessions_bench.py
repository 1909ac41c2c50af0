#!/usr/bin/env python3
"""Many cameras on one context (hnet_sessions, include/hnet.h): wall time per tick of K sessions over the replay fixture - every session pushes one frame, then
all K current pairs run as one sessions_infer - against the same K pairs as a loop of hnet_push_image + hnet_infer on one context (the per-camera interface).
One JSON line per K.  The device time of the session kernels (session_scatter / session_gather / session_remap) comes from a rocprofv3 --kernel-trace --stats run
of this tool (alone, no counters).
   python tools/sessions_bench.py [--k 1,8,64,256] [--ticks 30] [--warmup 5] [--raw]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", default="1,8,64,256")
    ap.add_argument("--ticks", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--variant", default="prior3")
    ap.add_argument("--raw", action="store_true", help="push 640 x 480 fisheye frames through push_raw instead of push")
    a = ap.parse_args()
    from cuahn_vio_amd import replay, weights
    from cuahn_vio_amd.homography_net import HnetEngine, HnetSessions
    ks = [int(x) for x in a.k.split(",")]
    blob = weights.pack_state_dict(weights.synthetic_state(0))
    fx = replay.load_fixture("indoor_forward_7")
    pool = np.stack([replay.render_frame(fx, 100 + j) for j in range(64)])
    priors = np.stack([replay.prior_offsets(fx, 100 + j) for j in range(64)]).astype(np.float64)
    kw = dict(variant=a.variant, mc_samples=16, dropout_p=0.05, mc_seed=1)
    use_prior = a.variant != "full"
    e = HnetEngine(blob, max_batch=max(ks), **kw)
    single = HnetEngine(blob, max_batch=1, **kw)
    L, h1 = single._L, single.handle
    fp = C.POINTER(C.c_float)
    mean1, cov1 = np.zeros(8, np.float32), np.zeros(64, np.float32)
    raw_pool = None
    if a.raw:
        # a fisheye 640 x 480 camera (uzhfpv.launch:75-82); a smooth pattern (the remap's cost does not depend on the content)
        y, x = np.mgrid[0:480, 0:640]
        raw_pool = np.stack([np.clip(128 + 60 * np.sin(x / 23.0 + j) * np.cos(y / 17.0), 0, 255).astype(np.uint8) for j in range(8)])
    for K in ks:
        s = HnetSessions(e, K)
        ids = np.arange(K, dtype=np.int32)
        if a.raw:
            cam = s.add_camera((275.46, 274.99, 315.96, 242.71), (-6.5e-06, -0.0104, 0.0149, -0.0056), 480, 640, fisheye=True)
            for i in range(K):
                s.bind_camera(i, cam)
        wall = []
        for t in range(a.warmup + a.ticks):
            sel = (np.arange(K) * 7 + t) % 64
            t0 = time.perf_counter()
            if a.raw:
                s.push_raw(ids, raw_pool[(np.arange(K) + t) % 8], np.full(K, 0.04 * t))
            else:
                s.push(ids, pool[sel], np.full(K, 0.04 * t))
            if t >= 1:
                s.infer(ids, priors[sel] if use_prior else None)
            t1 = time.perf_counter()
            if t >= a.warmup:
                wall.append((t1 - t0) * 1e3)
        dev_ms = s.last_timing()["device_ms"]
        s.close()
        # the per-camera interface: the same K pairs as K hnet_push_image + hnet_infer calls on one context
        loop = []
        for t in range(a.warmup + a.ticks):
            sel = (np.arange(K) * 7 + t) % 64
            t0 = time.perf_counter()
            for i in range(K):
                f = pool[sel[i]]
                L.hnet_push_image(h1, f.ctypes.data, 224, 320, 320, 0.04 * t)
                pr = (C.c_double * 8)(*priors[sel[i]]) if use_prior else None
                rc = L.hnet_infer(h1, pr, 0, mean1.ctypes.data_as(fp), cov1.ctypes.data_as(fp), None)
                assert rc == 0 or (t == 0 and i == 0)
            t1 = time.perf_counter()
            if t >= a.warmup:
                loop.append((t1 - t0) * 1e3)
        w, lp = float(np.median(wall)), float(np.median(loop))
        print(json.dumps({"tool": "sessions_bench", "variant": a.variant, "push": "raw" if a.raw else "u8", "k": K, "ticks": a.ticks,
                          "tick_ms_median": round(w, 4), "tick_ms_p90": round(float(np.percentile(wall, 90)), 4), "pairs_per_s": round(K / w * 1e3, 1),
                          "last_infer_device_ms": round(dev_ms, 4), "per_camera_loop_ms_median": round(lp, 4),
                          "per_camera_pairs_per_s": round(K / lp * 1e3, 1), "speedup": round(lp / w, 2)}), flush=True)
    e.close()
    single.close()


if __name__ == "__main__":
    main()
