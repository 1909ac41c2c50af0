#!/usr/bin/env python3
"""Wall and device time of hnet_sessions_keyframe_revisit and of a track with a keyframe map, on a GPU:
  python tools/keyframe_map_bench.py [--cameras 8 64] [--ticks 40] [--warmup 5] [--levels 3] [--iterations 6] [--capacity 3]
Per K cameras two sessions objects on one context, with and without a map.  Every tick pushes the next frame of an out-and-back path (4 seeds, cycled)
to all K sessions of both, then times, with the same options and max_age = 1 (every tick re-keys, so every tick stores a keyframe),
  track+map  hnet_sessions_keyframe_track on the object with a map,
  track      the same call on the object without one (the two in turn, same box, same tick),
  revisit    hnet_sessions_keyframe_revisit of the same sessions after the track (max_closure_px 1e-6: the alignment runs and the revisit is REJECTED,
             so that the next tick's track is the one the other object sees too; --attach lets it attach instead).
Wall: the call; device: hnet_sessions_last_keyframe_device_ms.  Medians over --ticks ticks after --warmup.  track+map - track is the price of the two
launches more (note, store); revisit - track the price of select against start and of the candidate's gather against the keyframe's."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cameras", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--ticks", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--levels", type=int, default=3)
    ap.add_argument("--iterations", type=int, default=6)
    ap.add_argument("--capacity", type=int, default=3)
    ap.add_argument("--attach", action="store_true")
    a = ap.parse_args()
    import keyframe_util as K
    from cuahn_vio_amd import _capi, weights
    from cuahn_vio_amd.homography_net import HnetEngine, HnetSessions
    blob = weights.pack_state_dict(weights.synthetic_state(0))
    seqs = [K.sequence("out-and-back", seed) for seed in (1, 2, 5, 11)]
    for n in a.cameras:
        e = HnetEngine(blob, variant="prior3", mc_samples=16, dropout_p=0.05, mc_seed=9, max_batch=n)
        with_map, without = HnetSessions(e, n), HnetSessions(e, n)
        for s in (with_map, without):
            s.enable_keyframes()
        with_map.enable_keyframe_map(a.capacity)
        ids = np.arange(n, dtype=np.int32)
        kw = dict(levels=a.levels, max_iterations=a.iterations)
        rows, seen = [], 0
        for t in range(a.warmup + a.ticks + 1):
            f = t % 8                                                  # frame 8 of the path is frame 0's pose: the path repeats
            frames = np.stack([seqs[i % 4][0][f] for i in range(n)])
            steps = np.stack([seqs[i % 4][2][f if f else 8] for i in range(n)])
            row = []
            for s in (with_map, without):
                s.push(ids, frames)
                t0 = time.perf_counter()
                s.keyframe_track(ids, steps, max_age=1, **kw)
                row += [(time.perf_counter() - t0) * 1e3, s.last_keyframe_device_ms()]
            t0 = time.perf_counter()
            rv = with_map.keyframe_revisit(ids, max_closure_px=0.0 if a.attach else 1e-6, **kw)
            row += [(time.perf_counter() - t0) * 1e3, with_map.last_keyframe_device_ms()]
            if t == 0:
                continue
            seen |= int(np.bitwise_or.reduce(rv["flags"]))
            rows.append(row)
        r = np.median(np.array(rows[a.warmup:]), axis=0)
        print(f"K = {n:3d}, levels={a.levels} K_trials={a.iterations} capacity={a.capacity}: track+map wall {r[0]:.4f} ms, device {r[1]:.4f} ms | track wall {r[2]:.4f} ms, "
              f"device {r[3]:.4f} ms | revisit wall {r[4]:.4f} ms, device {r[5]:.4f} ms | track+map - track: wall {r[0] - r[2]:+.4f} ms, device {r[1] - r[3]:+.4f} ms | "
              f"revisit - track: wall {r[4] - r[2]:+.4f} ms, device {r[5] - r[3]:+.4f} ms (revisit flags seen after the first tick: {seen}; "
              f"{_capi.RV_CLOSURE_ABOVE_MAX} = rejected after the alignment, {_capi.RV_ATTACHED} = attached)", flush=True)
        with_map.close()
        without.close()
        e.close()


if __name__ == "__main__":
    main()
